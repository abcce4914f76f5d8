"""Far-address layouts of tests/test_gpu_far_addresses.py (no GPU needed; checked by tests/test_far_cases_cpu.py on ``device="meta"``).

Every offset of the forward path is 64-bit by contract. A ``FarCase`` places q, k, v and `out` as ``as_strided`` views into ONE allocation of
about 14.4 GB, so that some of each operand's elements lie more than 2^32 bytes (2^32 ELEMENTS where the axis says so) from the operand's
base pointer - through one address term per axis:

* ``batch``   B = 2, H = 2, Hk = 1: batch 1 lies 2^33 bytes behind batch 0 (2^33 for every dtype: `out` is 16-bit for e4m3 inputs too);
* ``head``    B = 1, H = Hk = 2, rows of a head next to each other (bhsd-like): head 1 lies 2^33 bytes behind head 0;
* ``rows``    B = 1, H = Hk = 2, the row pitch is ``KV_PITCH`` = 2^26 bytes, the largest K / V row stride la_fwd accepts
              (LA_MAX_KV_ROW_STRIDE_BYTES, include/lite_attention_amd.h): rows 64 .. 149 lie past 2^32 bytes, rows 128 .. 149 past 2^33;
* ``packed``  (150, H = 2, Hk = 1, D) with the same row pitch and three sequences of 70 / 60 / 20 rows: sequence 1 starts past 2^32
              bytes, sequence 2 past 2^33 - the ``cu_seqlens`` row offset carries the distance.

Sq = Sk = 150 everywhere: three 64-key tiles with a ragged last one, one q-tile (two 128-row ones). The four operands are interleaved
INSIDE the row pitch (q, k, v, out at a quarter of the pitch each), so every operand has every far row.

The allocation is filled with byte 0xFF first: NaN in bf16 (0xFFFF), fp16 (0xFFFF) and e4m3 (0xFF), so the fill is poison for the inputs and
canary for the output at once.

Wrap-safety (a condition on the layout, proved per case by the CPU test; not a measurement). A body that builds a byte offset X >= 0 in
32 bits reads or writes at base + one of four images of X:

    u32(X)                in [0, 2^32)          i32(X)                in [-2^31, 2^31)
    es * u32(X / es)      in [0, es * 2^32)     es * i32(X / es)      in [-es * 2^31, es * 2^31)         (es = element size, at most 2)

With every operand's base at ``ORIGIN`` = 2^32 bytes or a little more into the allocation, and the allocation at least base + 2^33 long
(2^32 + 2^33 = 12.9 GB; the ``rows`` pitch makes it 2^32 + 150 * 2^26 = 14.4 GB), all four images of every element stay inside the
allocation: such a body gives WRONG NUMBERS - it lands on the 0xFF fill, or on another row / head / batch of the same operand, whose random
values differ - and never faults. (A stray WRITE lands on the fill or on another output row; both are seen.)"""
import torch

F8 = torch.float8_e4m3fn
AXES = ("batch", "head", "rows", "packed")
ORIGIN = 1 << 32                     # bytes in front of the first operand: the negative images of a 2-byte element offset reach -2^32
FAR = 1 << 33                        # the batch / head distance, bytes
KV_PITCH = 1 << 26                   # bytes: LA_MAX_KV_ROW_STRIDE_BYTES
S = 150
PACKED_LENS = (70, 60, 20)
FILL = 0xFF
OPERANDS = ("q", "k", "v", "out")


def out_dtype(dtype):
    return torch.bfloat16 if dtype == F8 else dtype


class Operand:
    """One view: dtype, logical shape, ELEMENT strides, and the byte offset of its first element in the allocation."""

    def __init__(self, dtype, shape, byte_strides, base):
        self.dtype, self.shape, self.base, self.es = dtype, tuple(shape), base, dtype.itemsize
        assert all(s % self.es == 0 for s in byte_strides) and base % 16 == 0
        self.byte_strides = tuple(byte_strides)
        self.strides = tuple(s // self.es for s in byte_strides)

    def view(self, buf):
        """The view into `buf` (1-D uint8, any device)."""
        return buf.view(self.dtype).as_strided(self.shape, self.strides, self.base // self.es)

    def rel_bytes(self):
        """int64 tensor of the view's shape: each element's byte offset from the view's first element - the X a kernel computes."""
        x = torch.zeros(self.shape, dtype=torch.int64)
        for dim, (n, s) in enumerate(zip(self.shape, self.byte_strides)):
            idx = [1] * len(self.shape)
            idx[dim] = n
            x = x + (torch.arange(n, dtype=torch.int64) * s).view(idx)
        return x

    def extent(self):
        """One past the last byte of the view, from the start of the allocation."""
        return self.base + sum((n - 1) * s for n, s in zip(self.shape, self.byte_strides)) + self.es


def images(x, es):
    """The four 32-bit truncation images of the byte offsets `x` (int64, multiples of es): u32 / i32 of the byte offset, u32 / i32 of the
    element offset scaled back to bytes."""
    def u32(t):
        return t & 0xFFFFFFFF

    def i32(t):
        return ((t + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    e = x // es
    return {"bytes_u32": u32(x), "bytes_i32": i32(x), "elems_u32": u32(e) * es, "elems_i32": i32(e) * es}


class FarCase:
    def __init__(self, axis, dtype, D):
        assert axis in AXES
        self.axis, self.dtype, self.D, self.packed = axis, dtype, D, axis == "packed"
        self.B = 2 if axis == "batch" else 1
        self.H = 2
        self.Hk = 1 if axis in ("batch", "packed") else 2
        self.Sq = self.Sk = S
        es, odt = dtype.itemsize, out_dtype(dtype)
        if axis in ("rows", "packed"):
            pitch, slot = KV_PITCH, KV_PITCH // 4               # q | k | v | out inside the pitch; the heads of an operand side by side
            head = {n: D * (2 if n == "out" else es) for n in OPERANDS}
            batch = 0
        elif axis == "batch":
            slot = self.H * D * 2                                 # the 16-bit row of all heads (e4m3 rows use the first half)
            pitch = 4 * slot
            head = {n: D * (2 if n == "out" else es) for n in OPERANDS}
            batch = FAR
        else:                                                     # head: (B, H, S, D)-like, the rows of a head next to each other
            slot = D * 2
            pitch = 4 * slot
            head = {n: FAR for n in OPERANDS}
            batch = 0
        self.pitch = pitch
        self.ops = {}
        for i, n in enumerate(OPERANDS):
            dt = odt if n == "out" else dtype
            heads = self.H if n in ("q", "out") else self.Hk
            rows = self.Sq if n in ("q", "out") else self.Sk
            shape, strides = (rows, heads, D), (pitch, head[n], dt.itemsize)
            if not self.packed:
                shape, strides = (self.B, *shape), (batch, *strides)
            self.ops[n] = Operand(dt, shape, strides, ORIGIN + i * slot)
        # long enough for every element and for base + es * 2^32 of every operand (the largest positive image), in whole 16-byte units,
        # plus one row pitch of fill behind the last row (a read one row past the end would be wrong, it need not be a fault)
        need = max(max(o.extent(), o.base + (o.es << 32)) for o in self.ops.values())
        self.nbytes = (need + 15) // 16 * 16 + KV_PITCH

    @property
    def id(self):
        return self.axis

    def views(self, buf):
        """{"q", "k", "v", "out"} -> view into `buf` (1-D uint8 of at least ``nbytes``)."""
        assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.numel() >= self.nbytes
        return {n: o.view(buf) for n, o in self.ops.items()}

    def logical_shape(self, name):
        return self.ops[name].shape

    def cu_seqlens(self):
        assert self.packed
        return torch.tensor([0, *torch.tensor(PACKED_LENS).cumsum(0).tolist()], dtype=torch.int32)

    def far_mask(self, name, limit=1 << 32):
        """bool tensor of the operand's shape: the elements `limit` bytes or more from the operand's base."""
        return self.ops[name].rel_bytes() >= limit


MAX_BYTES = max(FarCase(ax, dt, 256).nbytes for ax in AXES for dt in (torch.bfloat16, F8))


def inputs(case, seed):
    """CPU q, k, v of the case's logical shapes: ``randn``, so distinct per batch, head and row."""
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(*case.logical_shape(n), generator=g).to(case.dtype) for n in ("q", "k", "v")}


def all_fill(buf, chunk=1 << 30):
    """Every byte of `buf` (1-D uint8, a multiple of 8 bytes long) is FILL; scanned in chunks of `chunk` bytes."""
    words = buf.view(torch.int64)
    step = chunk // 8
    return all(bool((words[i:i + step] == -1).all()) for i in range(0, words.numel(), step))
