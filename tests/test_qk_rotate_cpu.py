"""CPU: head rotation of the q / k prologue - the three `_rot` entry points under ABI 9 and their own validation rules (all answered
before any HIP call, so no device is needed), `head_rotation`, and the orthogonality of the matrix the references multiply by."""
import ctypes
import subprocess
import sys

import pytest
import torch

from liteattention_amd import _cabi

import test_token_order_cpu as mapped

ROT_SIZE = ctypes.sizeof(_cabi.LaHeadRotation)


def test_the_three_entry_points_and_the_struct_agree_with_the_header(tmp_path):
    lib = _cabi.load()
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    for name, struct in mapped.ENTRIES:                                # (declared == exported == bound: tests/test_cabi.py)
        assert name + "_rot" in _cabi.EXPORTED_SYMBOLS
        assert [t._type_ for t in getattr(lib, name + "_rot").argtypes[:3]] == [struct, _cabi.LaRowMap, _cabi.LaHeadRotation]
    c = tmp_path / "layout.c"
    c.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{mapped.HEADER}"\nint main(void){{'
                 'printf("%zu %zu %zu\\n", sizeof(la_head_rotation), offsetof(la_head_rotation, reserved), '
                 'offsetof(la_head_rotation, signs)); return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(tmp_path / "layout"), str(c)], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ROT_SIZE, _cabi.LaHeadRotation.reserved.offset, _cabi.LaHeadRotation.signs.offset]


@pytest.mark.parametrize("entry,struct", mapped.ENTRIES)
@pytest.mark.parametrize("case,want", [
    (dict(null_rot=True), _cabi.LA_ERR_NULL_ARG),
    (dict(rot_size=ROT_SIZE - 8), _cabi.LA_ERR_STRUCT_SIZE),
    (dict(head_dim=96), _cabi.LA_ERR_HEAD_DIM),
    (dict(head_dim=192), _cabi.LA_ERR_HEAD_DIM),
    (dict(head_dim=32), _cabi.LA_ERR_HEAD_DIM),
    (dict(signs=0x70002), _cabi.LA_ERR_STRIDE),
    (dict(head_dim=96, batch=0), _cabi.LA_ERR_SHAPE),                # the head_dim rule sits with head_dim: behind the sizes
])
def test_first_failing_check_without_a_device(entry, struct, case, want):
    case = dict(case)
    a = mapped._valid_args(struct)
    r = _cabi.LaHeadRotation()
    r.struct_size, r.signs = case.pop("rot_size", ROT_SIZE), case.pop("signs", 0x70000)
    null_rot = case.pop("null_rot", False)
    for k, v in case.items():
        setattr(a, k, v)
    for m in (None, ctypes.byref(mapped._valid_map())):                # without and with a row map
        assert getattr(_cabi.load(), entry + "_rot")(ctypes.byref(a), m, None if null_rot else ctypes.byref(r), None) == want


def test_head_rotation_is_cached_signed_and_checked_before_any_launch(monkeypatch):
    import liteattention_amd as L
    r = L.head_rotation(128, seed=3)
    assert L.head_rotation(128, seed=3) is r and L.head_rotation(128, seed=4) is not r
    assert r.signs.dtype == torch.float32 and r.signs.shape == (128,) and bool((r.signs.abs() == 1).all()) and bool((r.signs < 0).any())
    assert bool((L.head_rotation(64, signs=False).signs == 1).all())
    with pytest.raises(ValueError):
        L.head_rotation(96)
    launched = []
    monkeypatch.setattr(sys.modules["liteattention_amd.qk_prep"], "_call", lambda *a, **k: launched.append(a))
    x = mapped._fake(torch.zeros(1, 4, 2, 64).bfloat16())              # a CPU tensor that says it lives on a GPU: checks run, no launch
    bad = ((r, ValueError), (L.HeadRotation(torch.ones(64).double()), ValueError), (torch.ones(64), TypeError),
           (L.HeadRotation(torch.ones(64, device="meta")), ValueError))      # length, dtype, not a rotation, device
    for rot, exc in bad:
        for fn in (L.qk_prep, L.qk_prep_fp8, L.qk_prep_amax, L.qk_prep_smooth, L.qk_prep_colmean):
            with pytest.raises(exc):
                fn(x, None, 1e-6, None, rotate=rot)
    with pytest.raises(ValueError):
        L.qk_prep_reference(x, rotate=r)
    assert not launched
    L.qk_prep(x, None, 1e-6, None, rotate=L.head_rotation(64))
    assert launched[0][0] == "la_qk_prep_rot" and launched[0][5]._obj.signs == L.head_rotation(64).signs.data_ptr()


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("signs", [True, False])
def test_the_reference_rotation_leaves_every_score_alone(D, signs):
    """a, b = the references of q and k with `rotate=`, c, d without: a b^T == c d^T to fp64 rounding, so M is orthogonal; and M is the
    matrix the header pins, H[i][j] = (-1)^popcount(i & j) with the signs on its rows."""
    import liteattention_amd as L
    g = torch.Generator().manual_seed(D)
    q, k = torch.randn(1, 7, 1, D, generator=g), torch.randn(1, 7, 1, D, generator=g)
    tables = L.rope_tables((1, 3, 3), D)
    rot = L.head_rotation(D, seed=1, signs=signs)
    a, b = (L.qk_prep_reference(t, None, 1e-6, tables, norm="head", rotate=rot)[0, :, 0] for t in (q, k))
    c, d = (L.qk_prep_reference(t, None, 1e-6, tables, norm="head")[0, :, 0] for t in (q, k))
    assert (a @ b.T - c @ d.T).abs().max().item() <= 1e-12 * D
    M = sys.modules["liteattention_amd.qk_prep"].rotation_matrix(rot)
    assert M[5, D - 3].item() == pytest.approx(rot.signs[5].item() * (-1) ** bin(5 & (D - 3)).count("1") / D ** 0.5, rel=1e-15)
