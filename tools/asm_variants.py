"""Builds A/B variants of the hand-scheduled kernels: one library per generator-option setting, under build_variants/.

    python tools/asm_variants.py x_base=x64: x_nodma=x64:nodma f8_base=x64f8: ...
      name=x64:<opts>    the head_dim-128 bf16 body with the option words <opts>
      name=x64f8:<opts>  the head_dim-128 fp8 body of the form of P that <opts> names (exp / lvalu, else the default), with its consts
      name=x64d<D>:<opts> the bf16 body of head_dim <D> (64, 96, 192, 256)
    Each is one record of the manifest (liteattention_amd/_bodies.py) generated into build_variants/<name>.gen/ by its runner: the
    generator sees <opts> and no LA_X64* variable of the caller. Every other body is the tree's (build the product first).
    (GPU box)  LITEATTENTION_AMD_LIB=$PWD/build_variants/<name>.so python tools/abl_bench.py
Ablation variants compute wrong results; they only price a component (HISTORY.md section 4).
"""
import os, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "liteattention_amd", "csrc")
OUT = os.path.join(ROOT, "build_variants")
sys.path.insert(0, ROOT)


def build_one(spec):
    from liteattention_amd.build import SOURCES, _bodies, _build_record
    name, _, opt = spec.partition("=")
    kind, _, opt = opt.partition(":")
    if kind == "x64f8":                   # (bench with --dtype fp8) the generator checks the body's name against its form of P
        words = opt.split(",")
        form = next((f for f in ("lvalu", "exp") if f in words), "")
        body, opt = _bodies.find(128, "fp8", form), ",".join(w for w in words if w != form)
    elif kind == "x64":
        body = _bodies.find(128, "bf16")
    elif kind in ("x64d64", "x64d96", "x64d192", "x64d256"):      # the other head dims of the bf16 generator (bench with tools/d64_bench.py / tools/d256_bench.py <D>)
        body = _bodies.find(int(kind[4:]), "bf16")
    else:
        raise SystemExit(f"{spec}: options must start with x64: (bf16), x64d256: (bf16 head_dim 256) or x64f8: (fp8)")
    gen_dir = os.path.join(OUT, name + ".gen")
    os.makedirs(gen_dir, exist_ok=True)
    macros = [f'-D{body.macro}="{_bodies.generate(body, gen_dir, opt)}"']
    if body.consts_macro:                 # the constants the generator wrote with this body, not the tree's
        macros.append(f'-D{body.consts_macro}="{os.path.join(gen_dir, body.inc.replace("_body.inc", "_consts.h"))}"')
    so = os.path.join(OUT, f"{name}.so")
    info = _build_record([os.path.join(gen_dir, body.inc)], (), True)          # la_build_info() of the variant: its options, and wrong_results=1 for pricing bodies
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           f'-DLA_BUILD_INFO="{info}"'] + macros + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", so]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return so


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    with ThreadPoolExecutor(4) as ex:
        for so in ex.map(build_one, sys.argv[1:]):
            print(so)
