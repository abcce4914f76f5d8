"""CPU: the far-address layouts of tests/far_cases.py are what tests/test_gpu_far_addresses.py needs them to be. Everything runs on
``device="meta"`` views and int64 index arithmetic: nothing large is allocated.

Per axis, dtype and head dim: the far offsets exceed 2^32 bytes (2^32 elements where the axis says so); all four 32-bit truncation images
of EVERY element whose image differs from its offset lie inside the allocation, on the 0xFF fill or on an element of another row / head /
batch of the SAME operand (so a truncating body can neither fault nor read the right data by accident); every truncation kind moves some
element of every operand (so it is seen); the four views do not overlap; every stride passes ``layout_cases.strides_ok``."""
import pytest
import torch

import far_cases as fc
import layout_cases as lc
from far_cases import F8

DTYPES = [torch.bfloat16, torch.float16, F8]
HEAD_DIMS = [64, 96, 128, 192, 256]
CASES = [(ax, dt, D) for ax in fc.AXES for dt in DTYPES for D in HEAD_DIMS]


def _id(c):
    return f"{c[0]}-{str(c[1]).split('.')[-1]}-d{c[2]}"


def _owner_table(case):
    """(sorted absolute byte addresses of every byte of every view, operand index of each, row id of each): row id = the flat index over
    every dimension but the last, i.e. (batch,) row, head."""
    addr, op_i, row = [], [], []
    for i, n in enumerate(fc.OPERANDS):
        o = case.ops[n]
        a = o.rel_bytes() + o.base
        rows = torch.arange(a[..., 0].numel(), dtype=torch.int64).view(a.shape[:-1]).unsqueeze(-1).expand(a.shape)
        for byte in range(o.es):
            addr.append((a + byte).reshape(-1))
            op_i.append(torch.full((a.numel(),), i, dtype=torch.int64))
            row.append(rows.reshape(-1))
    addr, op_i, row = torch.cat(addr), torch.cat(op_i), torch.cat(row)
    order = torch.argsort(addr)
    return addr[order], op_i[order], row[order]


@pytest.mark.parametrize("case_id", CASES, ids=_id)
def test_layout_is_far_wrap_safe_and_disjoint(case_id):
    axis, dtype, D = case_id
    case = fc.FarCase(axis, dtype, D)
    assert case.nbytes <= fc.MAX_BYTES < 15 * 10 ** 9 and case.nbytes % 16 == 0
    buf = torch.empty(case.nbytes, dtype=torch.uint8, device="meta")
    views = case.views(buf)
    for n, vw in views.items():
        o = case.ops[n]
        assert vw.device.type == "meta" and vw.dtype == (fc.out_dtype(dtype) if n == "out" else dtype)
        assert tuple(vw.shape) == o.shape and vw.stride() == o.strides and vw.storage_offset() * o.es == o.base
        assert lc.strides_ok(vw, dtype == F8 and n != "out"), n
        assert o.base >= fc.ORIGIN and o.extent() <= case.nbytes
    assert tuple(views["q"].shape) == tuple(views["out"].shape) and tuple(views["k"].shape) == tuple(views["v"].shape)
    assert views["q"].shape[-2] == case.H and views["k"].shape[-2] == case.Hk and case.H % case.Hk == 0

    # ---- the four views do not overlap (nor does a view overlap itself)
    addr, op_i, row = _owner_table(case)
    assert bool((addr[1:] > addr[:-1]).all())

    # ---- what is far
    for n in fc.OPERANDS:
        o = case.ops[n]
        x = o.rel_bytes()
        if axis == "batch":
            assert int(x[1].min()) >= 1 << 33 and int(x[1].min()) // o.es >= 1 << 32 and int(x[0].max()) < 1 << 31
        elif axis == "head":
            assert int(x[:, :, 1].min()) >= 1 << 33 and int(x[:, :, 1].min()) // o.es >= 1 << 32 and int(x[:, :, 0].max()) < 1 << 31
        elif axis == "rows":
            assert o.byte_strides[1] == fc.KV_PITCH
            assert int(x[:, 64:].min()) >= 1 << 32 and int(x[:, 128:].min()) >= 1 << 33 and int(x[:, 128:].min()) // o.es >= 1 << 32
            assert x[:, 128:].shape[1] == 22
        else:
            assert o.byte_strides[0] == fc.KV_PITCH
            cu = case.cu_seqlens().tolist()
            assert cu == [0, 70, 130, 150] and cu[-1] == o.shape[0]
            assert cu[1] * o.byte_strides[0] > 1 << 32 and cu[2] * o.byte_strides[0] > 1 << 33
            assert cu[2] * o.strides[0] >= 1 << 32                                         # ELEMENTS, for every dtype

    # ---- the images of every element
    for i, n in enumerate(fc.OPERANDS):
        o = case.ops[n]
        x = o.rel_bytes()
        own_row = torch.arange(x[..., 0].numel(), dtype=torch.int64).view(x.shape[:-1]).unsqueeze(-1).expand(x.shape)
        for kind, img in fc.images(x, o.es).items():
            moved = img != x
            assert bool(moved.any()), (n, kind)                        # this truncation is seen on this operand
            assert not bool(moved[x < (1 << 31)].any())                # (an offset below 2^31 is its own image)
            if kind.startswith("bytes"):
                assert bool(moved[case.far_mask(n)].all()), (n, kind)  # every far element moves under a truncated byte offset
            a = (img + o.base)[moved]
            src_row = own_row[moved]
            assert int(a.min()) >= 0 and int(a.max()) + o.es <= case.nbytes, (n, kind, int(a.min()), int(a.max()))
            for byte in (0, o.es - 1):
                pos = torch.searchsorted(addr, a + byte).clamp(max=addr.numel() - 1)
                hit = addr[pos] == a + byte                            # else: the 0xFF fill
                assert bool((op_i[pos][hit] == i).all()), (n, kind, "lands in another operand")
                assert bool((row[pos][hit] != src_row[hit]).all()), (n, kind, "lands in its own row")


def test_one_allocation_holds_every_case():
    """The GPU test allocates ``MAX_BYTES`` once: 2^32 in front + 150 rows of 2^26 bytes + one pitch of fill behind them (14.4 GB;
    2^32 + 2^33 = 12.9 GB is the least that keeps the images of a 2-byte element offset inside)."""
    assert fc.KV_PITCH == 1 << 26 and fc.ORIGIN == 1 << 32
    assert (1 << 32) + (1 << 33) < fc.MAX_BYTES <= (1 << 32) + (fc.S + 1) * fc.KV_PITCH
    assert all(fc.FarCase(ax, dt, D).nbytes <= fc.MAX_BYTES for ax, dt, D in CASES)


def test_the_pitch_is_the_bound_of_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define\s+LA_MAX_KV_ROW_STRIDE_BYTES\s+(\d+)", open(os.path.join(root, "include", "lite_attention_amd.h")).read())
    assert m and int(m.group(1)) == fc.KV_PITCH


def test_images_and_fill_scan():
    x = torch.tensor([0, 6, (1 << 31) + 2, (1 << 32) + 4, (1 << 33) + 8, 3 << 32], dtype=torch.int64)
    im = fc.images(x, 2)
    assert im["bytes_u32"].tolist() == [0, 6, (1 << 31) + 2, 4, 8, 0]
    assert im["bytes_i32"].tolist() == [0, 6, -(1 << 31) + 2, 4, 8, 0]
    assert im["elems_u32"].tolist() == [0, 6, (1 << 31) + 2, (1 << 32) + 4, 8, 1 << 32]
    assert im["elems_i32"].tolist() == [0, 6, (1 << 31) + 2, -(1 << 32) + 4, 8, -(1 << 32)]
    buf = torch.full((4096,), fc.FILL, dtype=torch.uint8)
    assert fc.all_fill(buf, chunk=512)
    buf[4095] = 0xFE
    assert not fc.all_fill(buf, chunk=512)
    for dt in (torch.bfloat16, torch.float16, F8):                     # the fill is NaN in every type
        assert bool(torch.full((16,), fc.FILL, dtype=torch.uint8).view(dt).float().isnan().all())
