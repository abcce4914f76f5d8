"""Layout / neighbour helpers of tests/test_gpu_layout_poison.py (no GPU needed; checked by tests/test_layout_cases_cpu.py).

``embed`` places a logical (B, S, H, D) tensor - or a packed (T, H, D) one - as a strided VIEW inside a larger buffer whose every other
element is *poison*; ``embed_out`` builds the strided `out` view inside a buffer of *canary* bits. Nothing in the forward depends on an
address, so a launch on the views must give the bits of the launch on contiguous tensors, leave the canary alone and leave the poison
unread (NaN / inf / the largest finite value of the type would show in the result: `0 * NaN`, a moved row maximum) and unwritten.

All fills and comparisons work on the raw 16- / 8-bit patterns (``raw``), so NaN patterns compare and e4m3 needs no arithmetic."""
import torch

F8 = torch.float8_e4m3fn
IN_LAYOUTS = ("wide_rows", "bhsd", "packed_qkv", "batch0")
OUT_LAYOUTS = ("head_slice", "bhsd")
POISONS = ("nan", "huge", "inf")
# (even flat index of the buffer, odd flat index): the sign alternates along the last dimension
POISON_BITS = {
    (torch.bfloat16, "nan"): (0x7FC0, 0xFFC0), (torch.bfloat16, "huge"): (0x7F7F, 0xFF7F), (torch.bfloat16, "inf"): (0x7F80, 0xFF80),
    (torch.float16, "nan"): (0x7E00, 0xFE00), (torch.float16, "huge"): (0x7BFF, 0xFBFF), (torch.float16, "inf"): (0x7C00, 0xFC00),
    (F8, "nan"): (0x7F, 0xFF), (F8, "huge"): (0x7E, 0xFE),              # e4m3fn has no infinity; S.1111.111 is its NaN, S.1111.110 = 448
}
CANARY_BITS = 0x3C5A          # a finite 16-bit pattern (bf16 0.0133, fp16 1.088) no attention output of these tests is filled with


def raw_dtype(dtype):
    return torch.uint8 if dtype == F8 else torch.int16


def raw(t):
    """The tensor's bits as integers (same shape and strides)."""
    return t.view(raw_dtype(t.dtype)) if t.dtype in (F8, torch.bfloat16, torch.float16) else t


def _signed16(bits):
    return bits - 0x10000 if bits >= 0x8000 else bits


def poison_bits(dtype, poison):
    """The two bit patterns (even / odd flat index), as values of ``raw_dtype(dtype)``."""
    a, b = POISON_BITS[(dtype, poison)]
    return (a, b) if dtype == F8 else (_signed16(a), _signed16(b))


def fill_pattern(buf_raw, even, odd):
    flat = buf_raw.view(-1)
    flat[0::2] = even
    flat[1::2] = odd


def buffer_shape(shape, layout, lead=0, trail=0):
    """Physical shape of the buffer that holds a logical (B, S, H, D) tensor in `layout` (the leading batch dimension is kept for packed
    (T, H, D) tensors too: they are embedded as B = 1)."""
    B, S, H, D = shape
    if layout == "wide_rows":
        return (B, lead + S + trail, H, 2 * D)
    if layout == "bhsd":
        return (B, H, S + trail, D)
    if layout == "packed_qkv":
        return (B, S + trail, 3, H, D)
    if layout == "batch0":
        return (1, S + trail, H, D)
    if layout == "head_slice":                     # `out` only
        return (B, S + 2, H + 2, D)
    raise ValueError(layout)


def view_of(buf, shape, layout, lead=0, trail=0, which=0):
    """The logical (B, S, H, D) view into a buffer of ``buffer_shape``: no copy, no expansion (``batch0`` gives its one (1, S, H, D) image;
    ``embed`` expands it). `which`: 0 / 1 / 2 = the q / k / v slice of ``packed_qkv``."""
    B, S, H, D = shape
    if layout == "wide_rows":
        return buf[:, lead:lead + S, :, :D]
    if layout == "bhsd":
        return buf[:, :, :S].permute(0, 2, 1, 3)
    if layout == "packed_qkv":
        return buf[:, :S, which]
    if layout == "batch0":
        return buf[:, :S]
    if layout == "head_slice":
        return buf[:, 1:S + 1, 1:H + 1]
    raise ValueError(layout)


def embed(t, layout, poison, lead=0, trail=0):
    """(buffer, view): `view` has t's shape, dtype and bits and the strides of `layout`; every element of `buffer` outside it is poison.
    t: (B, S, H, D), or packed (T, H, D). ``packed_qkv`` takes a tuple (q, k, v) of equal shapes and returns (buffer, (qv, kv, vv));
    ``batch0`` takes a tensor whose batch entries are all equal (or B = 1) and returns the image expanded with batch stride 0."""
    ts = tuple(t) if layout == "packed_qkv" else (t,)
    packed = ts[0].dim() == 3
    ts = [x.unsqueeze(0) if packed else x for x in ts]
    shape, dtype = tuple(ts[0].shape), ts[0].dtype
    assert all(tuple(x.shape) == shape and x.dtype == dtype for x in ts)
    buf = torch.empty(buffer_shape(shape, layout, lead, trail), dtype=raw_dtype(dtype), device=ts[0].device)
    fill_pattern(buf, *poison_bits(dtype, poison))
    views = []
    for i, x in enumerate(ts):
        vw = view_of(buf, shape, layout, lead, trail, which=i)
        if layout == "batch0":
            assert all(torch.equal(raw(x[b]), raw(x[0])) for b in range(shape[0])), "batch0 embeds ONE image"
            vw.copy_(raw(x[:1]))
            vw = vw.expand(shape)
        else:
            vw.copy_(raw(x))
        vw = vw.view(dtype)
        views.append(vw.squeeze(0) if packed else vw)
    buf = buf.view(dtype)
    return (buf, tuple(views)) if layout == "packed_qkv" else (buf, views[0])


def embed_out(shape, dtype, layout, device, trail=0):
    """(buffer, view) for `out`: a (B, S, H, D) - or packed (T, H, D) - view with the strides of `layout` into a buffer of canary bits."""
    packed = len(shape) == 3
    shape4 = (1, *shape) if packed else tuple(shape)
    buf = torch.full(buffer_shape(shape4, layout, 0, trail), _signed16(CANARY_BITS), dtype=torch.int16, device=device)
    vw = view_of(buf, shape4, layout, 0, trail).view(dtype)
    return buf.view(dtype), (vw.squeeze(0) if packed else vw)


def covered(shape, layout, lead=0, trail=0, n_views=1, device="cpu"):
    """bool tensor of ``buffer_shape``: True where one of the views of the layout lives."""
    shape4 = (1, *shape) if len(shape) == 3 else tuple(shape)
    cov = torch.zeros(buffer_shape(shape4, layout, lead, trail), dtype=torch.bool, device=device)
    for i in range(n_views):
        view_of(cov, shape4, layout, lead, trail, which=i).fill_(True)
    return cov


def untouched_outside(buf, cov, even, odd):
    """Every element of `buf` outside `cov` still holds the fill pattern (even / odd flat index)."""
    want = torch.empty(buf.shape, dtype=raw_dtype(buf.dtype), device=buf.device)
    fill_pattern(want, even, odd)
    return bool((raw(buf)[~cov] == want[~cov]).all())


def canary_intact(buf, cov):
    c = _signed16(CANARY_BITS)
    return untouched_outside(buf, cov, c, c)


def strides_ok(view, is_fp8_input):
    """The library's rule (la_api.hip la_fwd): every batch / row / head stride non-negative and a multiple of 8 elements (16 for e4m3
    q / k / v), unit stride on the last dimension, base pointer 16-byte aligned."""
    gran = 16 if is_fp8_input else 8
    return (view.stride(-1) == 1 and all(s >= 0 and s % gran == 0 for s in view.stride()[:-1])
            and view.data_ptr() % 16 == 0)


# ------------------------------------------------------------------------------------------- hand-built read lists (list launches)
LIST_S, LIST_KT = 600, 10                          # 600 keys: ten 64-key tiles, the last one of 24 keys
SKIPPED_TILES = (2, 5)                             # in no row
LIST_RANGES = [9, 6, 4, 3, 1, 0]                   # three descending ranges (both ends inclusive): tiles 9 8 7 6 | 4 3 | 1 0
HALF_TILE = 7                                      # half-vote case: listed by the first half of every workgroup item only
HALF0_RANGES = LIST_RANGES
HALF1_RANGES = [9, 8, 6, 6, 4, 3, 1, 0]            # the same set without tile 7
MUST_DO_KEYS = [400, 200]                          # the 1-D must-do row: keys 200 .. 400 (reference order: start > end)


def list_rows(ranges_per_row, B, H, k_tiles=LIST_KT, dtype=torch.int32):
    """[B, H, Qt, k_tiles + 1] read list whose q-tile m holds ``ranges_per_row[m]`` = [start0, end0, ...]: row [L, start0, end0, ..., 0 ...]."""
    Qt = len(ranges_per_row)
    out = torch.zeros(B, H, Qt, k_tiles + 1, dtype=dtype)
    for m, r in enumerate(ranges_per_row):
        assert len(r) <= k_tiles
        out[:, :, m, 0] = len(r)
        out[:, :, m, 1:1 + len(r)] = torch.tensor(r, dtype=dtype)
    return out


def tile_rows(tile, block_n=64, S=LIST_S):
    """The valid key rows of a tile."""
    return slice(tile * block_n, min(S, (tile + 1) * block_n))


def poison_rows(t, rows, poison):
    """A copy of (B, S, H, D) `t` with the key rows `rows` (slices) overwritten by poison (alternating sign along the last dimension)."""
    out = t.clone()
    even, odd = poison_bits(t.dtype, poison)
    r = raw(out)
    for sl in rows:
        r[:, sl, :, 0::2] = even
        r[:, sl, :, 1::2] = odd
    return out
