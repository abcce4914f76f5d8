"""CPU: what every entry point of the C-ABI checks, fills and launches, held to a recording.

``liteattention_amd/csrc/la_api.hip`` holds no device code. ``tests/cabi_launches/recorder.cpp`` links it, compiled host-only, with
stand-ins for every launcher and size helper, runs each case of its table without a GPU and prints, per case, the return code,
``la_last_hip_error()``, ``la_fwd_workspace_bytes`` of the same block and every argument and parameter-struct field of every launch,
in order. ``tests/golden/cabi_launches.json`` holds that output as one digest per case (``python tests/test_cabi_launches_cpu.py
OUT.json`` writes it, ``--full OUT.json`` the text itself); it was recorded BEFORE la_fwd's body was rearranged into check / fill / dispatch with one workspace layout and one loop over runs, and
holds on both sides. The size helpers are stand-ins there: the real ones are pinned by tests/test_walk_bound_cpu.py, not here."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from liteattention_amd import build as la_build  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "cabi_launches.json")
WALK_BOUNDS = os.path.join(ROOT, "tests", "golden", "walk_bounds.json")
RECORDER = os.path.join(ROOT, "tests", "cabi_launches", "recorder.cpp")
CODES = {"LA_OK": 0, "LA_ERR_NULL_ARG": -1, "LA_ERR_STRUCT_SIZE": -2, "LA_ERR_DTYPE": -3, "LA_ERR_HEAD_DIM": -4, "LA_ERR_SHAPE": -5,
         "LA_ERR_STRIDE": -6, "LA_ERR_TILE_MISMATCH": -7, "LA_ERR_LISTS": -8, "LA_ERR_UNSUPPORTED": -9, "LA_ERR_LAUNCH": -10,
         "LA_ERR_SEQLEN": -11, "LA_ERR_WORKSPACE": -12, "LA_ERR_Q_WINDOW": -13}


def build_recorder(out, extra=()):
    """The stand-alone program: recorder.cpp + la_api.hip, host code only, with the library build's include paths and standard."""
    cmd = [la_build._hipcc(), "--offload-host-only", "-x", "hip", "-O1", "-std=c++17", "-I", la_build.INCLUDE, "-I", la_build.CSRC,
           *extra, RECORDER, os.path.join(la_build.CSRC, "la_api.hip"), "-o", out]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    return out


def record(binary):
    done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-4000:])
    return done


def _sha(obj, n=12):
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:n]


def digest(rec):
    """The recording as it is committed: one digest per case (everything but its name: code, HIP error, workspace bytes, every launch
    record) in the order of the table, one of the names, one of the legend, one per (dtype, head dim) group of the workspace grid.
    The full text is the recorder's own output: ``python tests/test_cabi_launches_cpu.py --full OUT.json`` on two trees, then diff."""
    grid = {}
    for name, row in rec["workspace_grid"].items():
        grid.setdefault(" ".join(name.split()[:2]), []).append([name, row])
    return {"split_bounds": rec["split_bounds"], "legend": _sha(rec["legend"]), "names": _sha([c["name"] for c in rec["cases"]]),
            "workspace_grid_seqlen_k": rec["workspace_grid_seqlen_k"], "workspace_grid": {k: _sha(v) for k, v in grid.items()},
            "cases": [_sha({k: v for k, v in c.items() if k != "name"}) for c in rec["cases"]]}


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    return json.loads(record(build_recorder(str(tmp_path_factory.mktemp("cabi_launches") / "recorder"))).stdout)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_every_case_matches_the_recording(recording, golden):
    got = digest(recording)
    assert got["legend"] == golden["legend"] and got["names"] == golden["names"] and len(got["cases"]) == len(golden["cases"])
    moved = [c for c, g, w in zip(recording["cases"], got["cases"], golden["cases"]) if g != w]
    assert not moved, f"{len(moved)} cases moved (now; the recorded text: see digest()):\n" + "\n".join(json.dumps(c) for c in moved[:10])


def test_workspace_bytes_grid_matches_the_recording(recording, golden):
    got = digest(recording)
    assert got["workspace_grid_seqlen_k"] == golden["workspace_grid_seqlen_k"]
    moved = [k for k, v in golden["workspace_grid"].items() if got["workspace_grid"].get(k) != v]
    assert not moved and list(got["workspace_grid"]) == list(golden["workspace_grid"]), \
        {k: v for k, v in recording["workspace_grid"].items() if " ".join(k.split()[:2]) in moved}


def test_a_case_name_states_its_code(recording):
    """'-> LA_ERR_X' in a case's name is the code and 'passes' is LA_OK (the codes themselves are in the digests): the table can be
    read without the numbers."""
    for c in recording["cases"]:
        m = re.search(r"-> (LA_\w+)", c["name"])
        if m:
            assert c["rc"] == CODES[m.group(1)], c["name"]
            if m.group(1) not in ("LA_OK", "LA_ERR_LAUNCH"):
                assert c["launches"] == [], c["name"]                                  # on error nothing has been launched
        elif "passes" in c["name"]:
            assert c["rc"] == 0 and c["launches"], c["name"]


def test_the_split_cases_sit_on_the_pinned_walk_bounds(recording, golden):
    bounds = json.load(open(WALK_BOUNDS))
    for dtype, dims in golden["split_bounds"].items():
        for head_dim, seqlen_k in dims.items():
            assert bounds[dtype][head_dim] == seqlen_k
    by_name = {c["name"]: c for c in recording["cases"]}
    for tag in ("bf16 d256", "bf16 d128", "e4m3 d256", "e4m3 d64"):
        per_run = 2 if tag.startswith("e4m3") else 1
        assert len(by_name[f"la_fwd: {tag} dense the bound -> one launch"]["launches"]) == per_run
        assert len(by_name[f"la_fwd: {tag} dense bound + 1 keys -> 2 runs + combine"]["launches"]) == 2 * per_run + 1
        assert len(by_name[f"la_fwd: {tag} dense twice the bound + 1 keys -> 3 runs + combine"]["launches"]) == 3 * per_run + 1


def test_the_recorder_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path, golden):
    """A plain executable: the sanitizer runtimes are linked into it, nothing is preloaded."""
    binary = build_recorder(str(tmp_path / "recorder_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    done = record(binary)
    assert done.stderr == "", done.stderr[-4000:]
    assert digest(json.loads(done.stdout))["cases"] == golden["cases"]


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        text = record(build_recorder(os.path.join(tmp, "recorder"))).stdout
    if sys.argv[1] == "--full":
        open(sys.argv[2], "w").write(text)
    else:
        d = digest(json.loads(text))
        cases = d.pop("cases")
        body = json.dumps(d, indent=1)[:-2] + ',\n "cases": [\n' + ",\n".join(
            "  " + ", ".join(f'"{c}"' for c in cases[i:i + 10]) for i in range(0, len(cases), 10)) + "\n ]\n}\n"
        open(sys.argv[1], "w").write(body)
