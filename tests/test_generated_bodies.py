"""CPU: static checks on the generated gfx950 bodies (liteattention_amd/csrc/gen_fwd_x64*.py). The bodies run inside a C++ shell
whose inline-asm statement declares what they clobber (v0-v222, s35-s95, every AGPR, m0, vcc, scc): a register outside that set
written by a body would silently corrupt compiler-owned state. Also pins the MFMA counts per step and that the head_dim-128 bodies of
the two 16-bit types differ in nothing but the MFMA / convert opcodes."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "liteattention_amd", "csrc")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bodies = _load("la_bodies_t", os.path.join(ROOT, "liteattention_amd", "_bodies.py"))      # the manifest, by path: importing the package needs the library
CASES = bodies.BODIES


def _case_id(b):
    return "-".join(x for x in (b.gen[:-3], str(b.head_dim), "" if b.dtype == "fp8" else b.dtype, b.form) if x)


def _generate(tmp_path, body, options=""):
    return open(bodies.generate(body, str(tmp_path), options)).read()


def _registers(text):
    """(max VGPR, max AGPR, set of SGPRs) named anywhere in the body."""
    vmax = amax = -1
    sgprs = set()
    for kind, lo, hi, single in re.findall(r"\b([vas])(?:\[(\d+):(\d+)\]|(\d+))\b", text):
        first, last = (int(single), int(single)) if single else (int(lo), int(hi))
        if kind == "v":
            vmax = max(vmax, last)
        elif kind == "a":
            amax = max(amax, last)
        else:
            sgprs.update(range(first, last + 1))
    return vmax, amax, sgprs


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_body_stays_inside_the_declared_clobbers(tmp_path, case):
    text = _generate(tmp_path, case)
    body = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith((";", "//")))
    vmax, amax, sgprs = _registers(body)
    assert 0 <= vmax <= 222, vmax                      # LA_X64_CLOBBERS: v0 .. v222
    assert amax <= 255
    assert sgprs and min(sgprs) >= 35 and max(sgprs) <= 95, (min(sgprs), max(sgprs))      # s32-s34 are ABI-reserved, s0-s31 the shell's
    assert "%0" in body and "%1" in body               # the two inputs: wave index, LDS address of the parameter block
    assert "s_setpc" not in body and "s_endpgm" not in body
    # every label is local to the asm statement (%= suffix): two instantiations in one translation unit must not collide
    for lab in re.findall(r"^\s*([.\w%=]+):\s*$", body, flags=re.M):
        assert lab.endswith("%="), lab


@pytest.mark.parametrize("D,per_phase", [(96, 24), (128, 32), (192, 24), (256, 32)])
def test_mfma_count_per_step(tmp_path, D, per_phase):
    """prologue QK of tile 0 (one phase) + two unrolled steps of (QK + PV): 5 phases of MFMAs."""
    text = _generate(tmp_path, bodies.find(D, "bf16"))
    assert text.count("v_mfma_f32_32x32x16_bf16") == 5 * per_phase
    assert "v_mfma_f32_32x32x16_f16" not in text


@pytest.mark.parametrize("D,qk,pv", [(64, 4, 4), (96, 8, 6), (128, 8, 8), (192, 6, 6), (256, 8, 8)])
@pytest.mark.parametrize("form", ["", "exp", "lvalu"])
def test_fp8_mfma_count_per_step(tmp_path, D, qk, pv, form):
    """fp8 bodies (gen_fwd_x64_fp8.py, LA_X64F8_D): prologue QK of tile 0 + two unrolled steps of (QK + PV [+ one row-sum MFMA per q-block in the
    matrix-pipe row-sum forms]); 64-row bodies (64 / 128) hold two q-blocks per wave, the 192 / 256 bodies one. The head_dim-192 body clamps the
    K tile's DMA source chunks to the 12 that exist."""
    text = _generate(tmp_path, bodies.find(D, "fp8", form))
    rowsum = 0 if form == "lvalu" else (2 if D <= 128 else 1)
    assert text.count("v_mfma_scale_f32_32x32x64_f8f6f4") == qk + 2 * (qk + pv + rowsum)
    assert ("v_min_u32" in text) == (D in (96, 192))
    assert text.count("s_barrier") == 2 + 2


def test_fp16_body_differs_only_in_the_type_dependent_opcodes(tmp_path):
    a = _generate(tmp_path, bodies.find(128, "bf16"))
    b = _generate(tmp_path, bodies.find(128, "f16"))
    norm = lambda t: t.replace("v_mfma_f32_32x32x16_bf16", "MFMA").replace("v_mfma_f32_32x32x16_f16", "MFMA") \
                      .replace("v_cvt_pk_bf16_f32", "CVT").replace("v_cvt_pk_f16_f32", "CVT")                      # noqa: E731
    la, lb = norm(a).splitlines(), norm(b).splitlines()
    assert len(la) == len(lb)
    assert [x for x, y in zip(la, lb) if x != y and not x.lstrip().startswith(("//", ";"))] == []


def test_two_waves_per_simd_body_of_head_dim_64_fits_two_waves(tmp_path):
    """The A/B body of round 4 (gen_fwd_x64.py LA_X64_OPT=w2, -DLA_D64_W2=1; profiles/r04_head_dim_64.md): an 8-wave workgroup with two
    waves per SIMD needs <= 256 registers per wave INCLUDING what the C++ shell keeps across the body: the body stays inside v0-v89 +
    a0-a79 (LA_X64W2_CLOBBERS), has 8 + 8 MFMAs per step and two loops (waves 0-3 / waves 4-7, the latter one QK ahead)."""
    text = _generate(tmp_path, bodies.find(64, "bf16"), "w2")
    body = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith((";", "//")))
    vmax, amax, sgprs = _registers(body)
    assert 0 <= vmax <= 89 and 0 <= amax <= 79, (vmax, amax)
    assert min(sgprs) >= 35 and max(sgprs) <= 95
    # group a: 2 steps x 16; group b: QK of tile 0 (8) + 2 steps x 16
    assert body.count("v_mfma_f32_32x32x16_bf16") == 2 * 16 + 8 + 2 * 16
    assert body.count("s_barrier") == 1 + 2 + 2          # prologue + one per step copy, both groups: every wave meets the same barriers
    shell = open(os.path.join(CSRC, "la_fwd_kernel_x64.hip")).read()
    clob = shell.split("#define LA_X64W2_CLOBBERS")[1].split("namespace la")[0]
    assert '"v89"' in clob and '"v90"' not in clob and '"a79"' in clob and '"a80"' not in clob


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_m16_body_stays_inside_the_declared_clobbers_and_has_the_16x16x32_counts(tmp_path, dtype):
    """The head_dim-128 body on v_mfma_f32_16x16x32 (gen_fwd_x64_m16.py, round 5; A/B build -DLA_X64_M16=1): same shell, same clobber
    set; 64 + 64 MFMAs per step (prologue QK + two unrolled steps = 5 phases of 64), no 32x32x16 MFMA, 64-bit VGPR tuples even-aligned."""
    text = _generate(tmp_path, bodies.m16(bodies.find(128, dtype)))
    assert "la_body_options: m16; wrong_results=0" in text.splitlines()[1]
    body = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith((";", "//")))
    vmax, amax, sgprs = _registers(body)
    assert 0 <= vmax <= 222 and amax <= 255 and min(sgprs) >= 35 and max(sgprs) <= 95
    assert max(int(hi) for _, hi in re.findall(r"\ba\[(\d+):(\d+)\]", body)) == 255 and max(int(hi) for _, hi in re.findall(r"\bv\[(\d+):(\d+)\]", body)) <= 222
    assert body.count(f"v_mfma_f32_16x16x32_{dtype}") == 5 * 64 and "32x32x16" not in body
    assert body.count("v_permlane16_swap_b32") >= 2 * 2 + 1                     # the transposing row reduction, twice per unrolled loop + prologue
    for lo in re.findall(r"\bv\[(\d+):(\d+)\]", body):
        assert int(lo[0]) % 2 == 0, lo                                             # gfx950: VGPR tuples must be 64-bit aligned
    for lab in re.findall(r"^\s*([.\w%=]+):\s*$", body, flags=re.M):
        assert lab.endswith("%="), lab


@pytest.mark.parametrize("gen,own_tag", [("gen_fwd_x64.py", ()), ("gen_fwd_x64_fp8.py", ()), ("gen_fwd_x64_m16.py", ("m16",))])
def test_every_schedule_only_word_is_an_option_the_generator_reads(gen, own_tag):
    """SCHEDULE_ONLY decides whether a body's tag says wrong_results=0: a word in it that no code reads is a promise about nothing.
    Read = `"word" in OPT` (or in a step's `opt = OPT | drop`) or `opt_val(OPT, "word", ...)`; `own_tag`: what the generator adds to
    the tag itself."""
    text = open(os.path.join(CSRC, gen)).read()
    listed = set(re.findall(r'"(\w+)"', re.search(r"^SCHEDULE_ONLY = \{(.*?)\}", text, flags=re.M | re.S).group(1)))
    read = set(re.findall(r'"(\w+)" (?:not )?in (?:OPT|opt)\b', text)) | set(re.findall(r'opt_val\(OPT, ["\'](\w+)["\']', text))
    assert listed and listed - read - set(own_tag) == set()
    assert set(own_tag) <= listed


def test_body_digest_product_cases_are_what_the_build_generates(tmp_path):
    """tools/body_digest.py (the byte-identity check of a generator refactor): its product cases are exactly the files
    build.generate_bodies writes - a new body cannot escape the check."""
    digest = _load("la_body_digest", os.path.join(ROOT, "tools", "body_digest.py"))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    cases = digest.product_cases(str(tmp_path / "a"))
    generated, _ = digest.build.generate_bodies(str(tmp_path / "b"), variant=False)
    consts = [p.replace("_body.inc", "_consts.h") for p in generated if os.path.exists(p.replace("_body.inc", "_consts.h"))]
    assert sorted(cases) == sorted("product/" + os.path.basename(p) for p in generated + consts)
    assert sorted(os.listdir(tmp_path / "b")) == sorted(os.path.basename(p) for p in cases.values()) and len(cases) == 34
    for case, path in cases.items():
        assert open(path, "rb").read() == open(tmp_path / "b" / os.path.basename(path), "rb").read(), case


def test_shell_digest_covers_the_shells_of_the_manifest(tmp_path):
    """tools/shell_digest.py (the gate for moving a piece of a shell into la_fwd_shell.h) compiles the shells the manifest names, and
    its reader takes a function's resource counts and mnemonic counts from device assembly."""
    digest = _load("la_shell_digest", os.path.join(ROOT, "tools", "shell_digest.py"))
    assert digest.SHELLS == [bodies.SHELL, bodies.SHELL_F8]
    asm = tmp_path / "k.s"
    asm.write_text("\t.text\n\t.type\tf,@function\nf: ; @f\n; %bb.0:\n\ts_nop 0\n.LBB0_1:\n\ts_nop 1\n\ts_endpgm\n\t.p2align 2\n.Lfunc_end0:\n"
                   "; Kernel info:\n; TotalNumSgprs: 8\n; NumVgprs: 3\n; NumAgprs: 0\n; ScratchSize: 0\n"
                   "\t.amdgpu_metadata\n---\namdhsa.kernels:\n  - .agpr_count:     0\n    .args:\n      - .offset:         0\n"
                   "    .group_segment_fixed_size: 0\n    .name:           f\n    .private_segment_fixed_size: 0\n    .sgpr_count:     8\n"
                   "    .sgpr_spill_count: 5\n    .vgpr_count:     3\n    .vgpr_spill_count: 0\namdhsa.target:   amdgcn-amd-amdhsa--gfx950\n")
    rec = digest.digest(str(asm))["f"]
    assert rec["mnemonics"] == {"s_nop": 2, "s_endpgm": 1} and rec["total"] == 3
    assert (rec["vgpr_count"], rec["sgpr_count"], rec["sgpr_spill_count"], rec["private_segment_fixed_size"]) == (3, 8, 5, 0)


def _shell_macros(shell):
    """({macro: default file} of the `#ifndef NAME` / `#define NAME "file"` pairs of body / consts includes, [macros the shell #includes])."""
    text = open(os.path.join(CSRC, shell)).read()
    pairs = re.findall(r'^#ifndef (\w+_(?:BODY|CONSTS)_INC)\b.*\n#define (\w+) "([^"]+)"', text, flags=re.M)
    assert all(a == b for a, b, _ in pairs) and len({a for a, _, _ in pairs}) == len(pairs), pairs
    return {a: f for a, _, f in pairs}, re.findall(r"^#include (\w+_(?:BODY|CONSTS)_INC)\b", text, flags=re.M)


def _shell_wants():
    """{shell: {macro: default file}} by the manifest."""
    want = {bodies.SHELL: {}, bodies.SHELL_F8: {}}
    for b in bodies.BODIES:
        macros = want[bodies.SHELL_F8 if b.dtype == "fp8" else bodies.SHELL]
        macros[b.macro] = b.inc
        if b.consts_macro:
            macros[b.consts_macro] = b.inc.replace("_body.inc", "_consts.h")
    return want


def test_the_manifest_and_the_shells_name_the_same_bodies():
    """A variant build points a shell at its own bodies with -D<MACRO>="<path>": a macro the shell does not know would compile, include
    the tree's default body and measure the product against itself. So: (a) each shell's (macro, default file) pairs are the
    manifest's records of that shell, no more and no fewer; (b) the shell includes every macro it defines."""
    for shell, macros in _shell_wants().items():
        defined, included = _shell_macros(shell)
        assert defined == macros, shell                                              # (a)
        assert set(defined) <= set(included), set(defined) - set(included)          # (b)


def test_a_variant_build_passes_one_define_per_manifest_macro(tmp_path, monkeypatch):
    """(c) with every option variable unset, a variant generation passes exactly one -D per manifest macro, each naming a file that
    exists (a test of its own: it runs the 31 generators, the two static checks above do not)."""
    for k in [k for k in os.environ if k.startswith("LA_X64")]:
        monkeypatch.delenv(k)
    build = _load("la_build_t3", os.path.join(ROOT, "liteattention_amd", "build.py"))
    generated, macros = build.generate_bodies(str(tmp_path), variant=True)
    passed = dict(re.fullmatch(r'-D(\w+)="(.+)"', m).groups() for m in macros)
    assert len(passed) == len(macros) == 34 and all(os.path.isfile(p) for p in passed.values())
    assert {m: os.path.relpath(p, str(tmp_path)) for m, p in passed.items()} == {m: f for ms in _shell_wants().values() for m, f in ms.items()}
    assert [os.path.basename(p) for p in generated] == [b.inc for b in bodies.BODIES]
