#!/usr/bin/env python
"""CPU: digest of what the compiler makes of the two C++ shells around the generated bodies (la_fwd_kernel_x64.hip,
la_fwd_kernel_x64_fp8.hip) - the gate for moving a piece of a shell: same registers, no scratch, no more instructions.

    python tools/shell_digest.py MANIFEST            write the manifest (the device assembly is kept in MANIFEST.files/)
    python tools/shell_digest.py --check MANIFEST    compare: every differing symbol with the mnemonics whose counts moved

The product bodies are generated into a temporary directory and each shell is compiled to device assembly with the build's own
flags. Per function symbol (kernels and the __noinline__ helpers) the manifest holds the resource counts of the metadata (helpers:
of the function's resource footer), the count of each mnemonic in its text and the total. Exit status of --check: 0 = every symbol
identical, 1 = only mnemonic multisets moved, 2 = a HARD condition is broken: scratch or VGPR spills anywhere, vgpr / agpr / sgpr
count or LDS size not the manifest's, more SGPR spills or more instructions than the manifest's."""
import collections
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("la_build", os.path.join(ROOT, "liteattention_amd", "build.py"))   # by path: the package
build = importlib.util.module_from_spec(_spec)                                                                   # import needs the .so
_spec.loader.exec_module(build)
bodies = build._bodies
SHELLS = [bodies.SHELL, bodies.SHELL_F8]
EQUAL = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size")
ZERO = ("private_segment_fixed_size", "vgpr_spill_count")
META = EQUAL + ZERO + ("sgpr_spill_count",)
FOOTER = {"NumVgprs": "vgpr_count", "NumAgprs": "agpr_count", "TotalNumSgprs": "sgpr_count", "ScratchSize": "private_segment_fixed_size"}


def compile_shell(shell, gen_dir, out_dir):
    macros = []
    for b in bodies.BODIES:
        macros.append(f'-D{b.macro}="{os.path.join(gen_dir, b.inc)}"')
        if b.consts_macro:
            macros.append(f'-D{b.consts_macro}="{os.path.join(gen_dir, b.inc.replace("_body.inc", "_consts.h"))}"')
    asm = os.path.join(out_dir, os.path.splitext(shell)[0] + ".s")
    cmd = [build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", build.INCLUDE, "-I", build.CSRC,
           '-DLA_BUILD_INFO="digest"'] + macros + ["--cuda-device-only", "-S", os.path.join(build.CSRC, shell), "-o", asm]
    res = subprocess.run(cmd, check=False, stderr=subprocess.PIPE, text=True)      # (warnings of the asm bodies' clobber lists: not shown)
    if res.returncode != 0:
        sys.stderr.write(res.stderr)
        raise RuntimeError(f"hipcc failed on {shell} with exit status {res.returncode} (diagnostics above)")
    return asm


def digest(asm_path):
    """{symbol: {resource counts, "mnemonics": {mnemonic: count}, "total": n}} of one device assembly file."""
    text = open(asm_path).read()
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n", text, re.M):
        sym = m.group(1)
        start = text.index(f"{sym}:", m.end())
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, start).start()
        nxt = text.find(",@function\n", end)
        counts = collections.Counter()
        for line in text[start:end].splitlines():
            word = line.split(None, 1)[0] if line.strip() else ""
            if line[:1] in ("\t", " ") and word and word[0] not in ".;" and not word.endswith(":"):
                counts[word] += 1
        rec = {"mnemonics": dict(sorted(counts.items())), "total": sum(counts.values())}
        footer = text[end:nxt if nxt > 0 else len(text)]
        for key, val in re.findall(r"^; (\w+): (\d+)\s*$", footer, re.M):
            if key in FOOTER:
                rec[FOOTER[key]] = int(val)
        out[sym] = rec
    meta = text[text.index("amdhsa.kernels:"):text.index("\namdhsa.target:")]
    for block in meta.split("\n  - ")[1:]:
        name = re.search(r"^    \.name:\s*(\S+)", block, re.M).group(1)            # (four blanks: the kernel's own keys, not its arguments')
        for key in META:
            out[name][key] = int(re.search(rf"^(?:    )?\.{key}:\s*(\d+)", block, re.M).group(1))
    return out


def run_all(keep):
    gen_dir = os.path.join(keep, "bodies")
    os.makedirs(gen_dir)
    build.generate_bodies(gen_dir, variant=False)
    with ThreadPoolExecutor(max_workers=len(SHELLS)) as ex:
        return dict(zip(SHELLS, (digest(a) for a in ex.map(lambda s: compile_shell(s, gen_dir, keep), SHELLS))))


def compare(want, got):
    """Prints every differing symbol. Returns (symbols whose multiset or counts moved, broken hard conditions)."""
    moved = hard = 0
    for shell in SHELLS:
        for sym in sorted(set(want[shell]) | set(got[shell])):
            old, new = want[shell].get(sym), got[shell].get(sym)
            if old is None or new is None:
                print(f"HARD {shell} {sym}: {'new symbol' if old is None else 'symbol is gone'}")
                hard += 1
                continue
            broken = [f"{k} {new[k]} != 0" for k in ZERO if new.get(k, 0) != 0]
            broken += [f"{k} {old.get(k)} -> {new.get(k)}" for k in EQUAL if old.get(k) != new.get(k)]
            broken += [f"{k} {old.get(k, 0)} -> {new.get(k, 0)}" for k in ("sgpr_spill_count", "total") if new.get(k, 0) > old.get(k, 0)]
            for b in broken:
                print(f"HARD {shell} {sym}: {b}")
            hard += len(broken)
            delta = {k: (old["mnemonics"].get(k, 0), new["mnemonics"].get(k, 0)) for k in set(old["mnemonics"]) | set(new["mnemonics"])
                     if old["mnemonics"].get(k, 0) != new["mnemonics"].get(k, 0)}
            soft = [f"{k} {old.get(k)} -> {new.get(k)}" for k in ("sgpr_spill_count", "total") if old.get(k) != new.get(k)]
            if delta or soft:
                moved += 1
                print(f"DIFFERS {shell} {sym}: " + ", ".join(soft + [f"{k} {a} -> {b}" for k, (a, b) in sorted(delta.items())]))
    return moved, hard


def main(argv):
    check = argv[:1] == ["--check"]
    manifest = os.path.abspath(argv[-1])
    with tempfile.TemporaryDirectory(prefix="shell_digest.") as tmp:
        keep = tmp if check else manifest + ".files"
        got = run_all(keep)
    n = sum(len(v) for v in got.values())
    if not check:
        json.dump(got, open(manifest, "w"), indent=0, sort_keys=True)
        print(f"{manifest}: {n} symbols of {len(SHELLS)} shells")
        return 0
    moved, hard = compare(json.load(open(manifest)), got)
    print(f"{n} symbols, {moved} differ from {manifest}, {hard} hard conditions broken")
    return 2 if hard else 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
