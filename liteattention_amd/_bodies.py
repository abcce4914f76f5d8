"""The generated kernel bodies: the one list of what the build generates (31 bodies, 3 ``*_consts.h`` beside the head_dim-128 fp8
ones) and the one way to run a generator. ``build.py``, ``tools/body_digest.py``, ``tools/asm_variants.py`` and the tests read this
table; ``tests/test_generated_bodies.py`` holds it against the ``#ifndef`` / ``#define`` pairs of the two shells. Stands alone (loaded
by path before the package can be imported) and is no build input: like ``build.py`` it is not hashed into ``la_build_info()``."""
from __future__ import annotations

import os
import subprocess
import sys
from typing import NamedTuple, Optional

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
X64, X64F8 = "gen_fwd_x64.py", "gen_fwd_x64_fp8.py"
X64_M16 = "gen_fwd_x64_m16.py"                 # head_dim 128 on the 16x16x32 MFMA (A/B build -DLA_X64_M16=1)
SHELL, SHELL_F8 = "la_fwd_kernel_x64.hip", "la_fwd_kernel_x64_fp8.hip"      # include the 16-bit / the fp8 bodies


class Body(NamedTuple):
    gen: str                        # generator script under csrc/
    head_dim: int                   # LA_X64_D / LA_X64F8_D
    dtype: str                      # bf16 / f16 (LA_X64_DTYPE) or fp8
    form: str                       # 16-bit: "" / "half" (LA_X64_FORM); fp8: the form of P, "" / "exp" / "lvalu" (last word of LA_X64F8_OPT)
    inc: str                        # output file
    macro: str                      # the shell's include macro
    consts_macro: Optional[str]     # fp8 head_dim 128: the macro of the <...>_consts.h the generator writes beside <...>_body.inc
    opt_var: str                    # environment variable that tunes this body alone in a variant build


BODIES = [Body(*row) for row in (
    (X64, 128, "bf16", "", "la_fwd_x64_body.inc", "LA_X64_BODY_INC", None, "LA_X64_OPT"),
    (X64, 128, "f16", "", "la_fwd_x64_f16_body.inc", "LA_X64_F16_BODY_INC", None, "LA_X64_OPT"),
    (X64, 64, "bf16", "", "la_fwd_x64_d64_body.inc", "LA_X64_D64_BODY_INC", None, "LA_X64_D64_OPT"),
    (X64, 64, "f16", "", "la_fwd_x64_d64_f16_body.inc", "LA_X64_D64_F16_BODY_INC", None, "LA_X64_D64_OPT"),
    (X64, 96, "bf16", "", "la_fwd_x64_d96_body.inc", "LA_X64_D96_BODY_INC", None, "LA_X64_D96_OPT"),
    (X64, 96, "f16", "", "la_fwd_x64_d96_f16_body.inc", "LA_X64_D96_F16_BODY_INC", None, "LA_X64_D96_OPT"),
    (X64, 192, "bf16", "", "la_fwd_x64_d192_body.inc", "LA_X64_D192_BODY_INC", None, "LA_X64_D192_OPT"),
    (X64, 192, "f16", "", "la_fwd_x64_d192_f16_body.inc", "LA_X64_D192_F16_BODY_INC", None, "LA_X64_D192_OPT"),
    (X64, 256, "bf16", "", "la_fwd_x64_d256_body.inc", "LA_X64_D256_BODY_INC", None, "LA_X64_D256_OPT"),
    (X64, 256, "f16", "", "la_fwd_x64_d256_f16_body.inc", "LA_X64_D256_F16_BODY_INC", None, "LA_X64_D256_OPT"),
    # skip lists per 128-row half (LA_FLAG_HALF_VOTE): the 256-row kernels
    (X64, 128, "bf16", "half", "la_fwd_x64_half_body.inc", "LA_X64_HALF_BODY_INC", None, "LA_X64_HALF_OPT"),
    (X64, 128, "f16", "half", "la_fwd_x64_half_f16_body.inc", "LA_X64_HALF_F16_BODY_INC", None, "LA_X64_HALF_OPT"),
    (X64, 64, "bf16", "half", "la_fwd_x64_d64_half_body.inc", "LA_X64_D64_HALF_BODY_INC", None, "LA_X64_D64_HALF_OPT"),
    (X64, 64, "f16", "half", "la_fwd_x64_d64_half_f16_body.inc", "LA_X64_D64_HALF_F16_BODY_INC", None, "LA_X64_D64_HALF_OPT"),
    (X64, 96, "bf16", "half", "la_fwd_x64_d96_half_body.inc", "LA_X64_D96_HALF_BODY_INC", None, "LA_X64_D96_HALF_OPT"),
    (X64, 96, "f16", "half", "la_fwd_x64_d96_half_f16_body.inc", "LA_X64_D96_HALF_F16_BODY_INC", None, "LA_X64_D96_HALF_OPT"),
    # fp8 on the block-scaled MFMA, three forms of P: "" the e4m3 byte computed directly, row sums from the matrix pipe; "exp" v_exp_f32
    # rounded by the hardware convert (LA_FLAG_FP8_MFMA_ROWSUM); "lvalu" that, and fp32 row sums on the VALU (the DEFAULT fp8 form)
    (X64F8, 128, "fp8", "", "la_fwd_x64_fp8_body.inc", "LA_X64F8_BODY_INC", "LA_X64F8_CONSTS_INC", "LA_X64F8_DEFAULT_OPT"),
    (X64F8, 128, "fp8", "exp", "la_fwd_x64_fp8_exp_body.inc", "LA_X64F8_EXP_BODY_INC", "LA_X64F8_EXP_CONSTS_INC", "LA_X64F8_EXP_OPT"),
    (X64F8, 128, "fp8", "lvalu", "la_fwd_x64_fp8_lvalu_body.inc", "LA_X64F8_LVALU_BODY_INC", "LA_X64F8_LVALU_CONSTS_INC", "LA_X64F8_LVALU_OPT"),
    (X64F8, 64, "fp8", "", "la_fwd_x64_fp8_d64_body.inc", "LA_X64F8_D64_BODY_INC", None, "LA_X64F8_D64_DEFAULT_OPT"),
    (X64F8, 64, "fp8", "exp", "la_fwd_x64_fp8_d64_exp_body.inc", "LA_X64F8_D64_EXP_BODY_INC", None, "LA_X64F8_D64_EXP_OPT"),
    (X64F8, 64, "fp8", "lvalu", "la_fwd_x64_fp8_d64_lvalu_body.inc", "LA_X64F8_D64_LVALU_BODY_INC", None, "LA_X64F8_D64_LVALU_OPT"),
    (X64F8, 96, "fp8", "", "la_fwd_x64_fp8_d96_body.inc", "LA_X64F8_D96_BODY_INC", None, "LA_X64F8_D96_DEFAULT_OPT"),
    (X64F8, 96, "fp8", "exp", "la_fwd_x64_fp8_d96_exp_body.inc", "LA_X64F8_D96_EXP_BODY_INC", None, "LA_X64F8_D96_EXP_OPT"),
    (X64F8, 96, "fp8", "lvalu", "la_fwd_x64_fp8_d96_lvalu_body.inc", "LA_X64F8_D96_LVALU_BODY_INC", None, "LA_X64F8_D96_LVALU_OPT"),
    (X64F8, 192, "fp8", "", "la_fwd_x64_fp8_d192_body.inc", "LA_X64F8_D192_BODY_INC", None, "LA_X64F8_D192_DEFAULT_OPT"),
    (X64F8, 192, "fp8", "exp", "la_fwd_x64_fp8_d192_exp_body.inc", "LA_X64F8_D192_EXP_BODY_INC", None, "LA_X64F8_D192_EXP_OPT"),
    (X64F8, 192, "fp8", "lvalu", "la_fwd_x64_fp8_d192_lvalu_body.inc", "LA_X64F8_D192_LVALU_BODY_INC", None, "LA_X64F8_D192_LVALU_OPT"),
    (X64F8, 256, "fp8", "", "la_fwd_x64_fp8_d256_body.inc", "LA_X64F8_D256_BODY_INC", None, "LA_X64F8_D256_DEFAULT_OPT"),
    (X64F8, 256, "fp8", "exp", "la_fwd_x64_fp8_d256_exp_body.inc", "LA_X64F8_D256_EXP_BODY_INC", None, "LA_X64F8_D256_EXP_OPT"),
    (X64F8, 256, "fp8", "lvalu", "la_fwd_x64_fp8_d256_lvalu_body.inc", "LA_X64F8_D256_LVALU_BODY_INC", None, "LA_X64F8_D256_LVALU_OPT"),
)]


def find(head_dim: int, dtype: str, form: str = "") -> Body:
    return next(b for b in BODIES if (b.head_dim, b.dtype, b.form) == (head_dim, dtype, form))


def m16(body: Body) -> Body:
    """-DLA_X64_M16=1 (A/B build): the two head_dim-128 16-bit bodies come from the 16x16x32 generator (its option variable tunes it)."""
    return body._replace(gen=X64_M16) if (body.gen, body.head_dim, body.form) == (X64, 128, "") else body


def generate(body: Body, out_dir: str, options: str = "", stdout=subprocess.DEVNULL, stderr=None) -> str:
    """Run ``body``'s generator into ``out_dir`` with the extra option words ``options`` ("a,b:2"). Returns the body's path. The
    generator sees the record's own LA_X64* variables and no other, whatever this process's environment holds."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("LA_X64")}
    if body.dtype == "fp8":
        env.update(LA_X64F8_D=str(body.head_dim), LA_X64F8_OPT=",".join(w for w in (options, body.form) if w))
    else:
        env.update(LA_X64_D=str(body.head_dim), LA_X64_DTYPE=body.dtype, LA_X64_FORM=body.form, LA_X64_OPT=options)
    path = os.path.join(out_dir, body.inc)
    subprocess.run([sys.executable, os.path.join(CSRC, body.gen), path], check=True, stdout=stdout, stderr=stderr, env=env)
    return path
