#!/usr/bin/env python
"""CPU: digest of everything the body generators (liteattention_amd/csrc/gen_fwd_x64*.py) can write - the proof that a generator
refactor changes no kernel: same bytes, same kernel.

    python tools/body_digest.py MANIFEST            write {case: sha256} (a case whose generator raises: "error"); the generated
                                                    files are kept in MANIFEST.files/ for the line-by-line comparison
    python tools/body_digest.py --check MANIFEST    compare: every differing case with its first differing line; exit status 1

Cases: product/<file> - what build.generate_bodies(dir, variant=False) writes (bodies and *_consts.h); ab/* - the A/B bodies (the
16x16x32 body in both types, the two-waves-per-SIMD body of head_dim 64); opt/<generator>/<form>/<word> - every option word a
generator reads (`"word" in OPT`, `opt_val(OPT, "word", ...)`), one at a time, per head dim of the generator."""
import hashlib
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
bodies = build._bodies                   # the manifest: every case below is one of its records, with option words
VALUES = dict(x=3, cap1=2, cap2=2, align=6, pad4=2, pad4b=1, halfskip=4, mfma16="both", dmapol="nt", tau=4, safe=2)
X64_FORMS = {"d64": bodies.find(64, "bf16"), "d128": bodies.find(128, "bf16"), "d256": bodies.find(256, "bf16"), "half": bodies.find(128, "bf16", "half")}


def option_words(gen):
    text = open(os.path.join(bodies.CSRC, gen)).read()
    return sorted(set(re.findall(r'"(\w+)" (?:not )?in OPT\b', text)) | set(re.findall(r'opt_val\(OPT, ["\'](\w+)["\']', text)))


def generator_cases():
    """(case, manifest record, option words)"""
    m16 = bodies.m16(bodies.find(128, "bf16"))
    cases = [(f"ab/m16-{t}", bodies.m16(bodies.find(128, t)), "") for t in ("bf16", "f16")] + [("ab/d64-w2", bodies.find(64, "bf16"), "w2")]
    word = lambda w: f"{w}:{VALUES[w]}" if w in VALUES else w                                                   # noqa: E731
    for w in option_words(bodies.X64):
        cases += [(f"opt/gen_fwd_x64/{form}/{w}", body, word(w)) for form, body in X64_FORMS.items()]
    for w in option_words(bodies.X64F8):
        form = w if w in ("exp", "lvalu") else ""       # a form word selects that form's record: the generator checks the body's name against its form of P
        cases += [(f"opt/gen_fwd_x64_fp8/d{d}/{w}", bodies.find(d, "fp8", form), "" if form else word(w)) for d in (64, 128, 192)]
    cases += [(f"opt/gen_fwd_x64_m16/d128/{w}", m16, word(w)) for w in option_words(m16.gen)]
    return cases


def product_cases(keep):
    """{case: path} of a product generation into keep/product."""
    d = os.path.join(keep, "product")
    os.makedirs(d)
    build.generate_bodies(d, variant=False)
    return {"product/" + n: os.path.join(d, n) for n in sorted(os.listdir(d))}


def run_all(keep):
    files = product_cases(keep)
    h = hashlib.sha256()
    for case in sorted(files):
        h.update(os.path.basename(files[case]).encode() + b"\0" + open(files[case], "rb").read())
    print(f"product: {len(files)} files, sha256 {h.hexdigest()[:16]}", file=sys.stderr)

    def one(c):
        case, body, words = c
        d = os.path.join(keep, case)
        os.makedirs(d)
        try:
            return case, bodies.generate(body, d, words, stderr=subprocess.DEVNULL)
        except subprocess.CalledProcessError:
            return case, None
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        files.update(ex.map(one, generator_cases()))
    return files


def kept(keep, case):
    """The file of `case` under `keep` (product: the file itself; else the one file of the case's directory), or None."""
    p = os.path.join(keep, case)
    return p if os.path.isfile(p) else next((os.path.join(p, n) for n in os.listdir(p)), None) if os.path.isdir(p) else None


def main(argv):
    check = argv[:1] == ["--check"]
    manifest = os.path.abspath(argv[-1])
    with tempfile.TemporaryDirectory(prefix="body_digest.") as tmp:
        keep = tmp if check else manifest + ".files"
        files = run_all(keep)
        digest = {c: hashlib.sha256(open(p, "rb").read()).hexdigest() if p else "error" for c, p in sorted(files.items())}
        n_err = sum(v == "error" for v in digest.values())
        if not check:
            json.dump(digest, open(manifest, "w"), indent=0)
            print(f"{manifest}: {len(digest)} cases, {n_err} raise")
            return 0
        want, bad = json.load(open(manifest)), 0
        for case in sorted(set(want) | set(digest)):
            old, new = want.get(case, "missing"), digest.get(case, "missing")
            if old == new:
                continue
            bad += 1
            msg = f"{old[:12]} -> {new[:12]}"
            ref = kept(manifest + ".files", case)
            if ref and files.get(case):
                a, b = open(ref).read().splitlines(), open(files[case]).read().splitlines()
                n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                msg = f"line {n + 1}: {a[n:n + 1]} -> {b[n:n + 1]}"
            print(f"DIFFERS {case}: {msg}")
        print(f"{len(digest)} cases, {n_err} raise, {bad} differ from {manifest}")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
