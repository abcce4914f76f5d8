"""GPU: la_output_error (liteattention_amd.calibration.output_error) against torch in fp64.

Tolerances. The four sums differ from torch's only in the order of the additions: both add exact fp64 terms (the difference of two
bf16 / fp16 / fp32 values and its square are exact or correctly rounded in fp64), n terms in any order agree to n 2^-53 relative of
the sum of magnitudes, and every term here is non-negative; with n <= 10^6 per bin that is 1.2e-10: asserted at 1e-9 relative. The
maximum and the non-finite count involve no rounding: exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
SHAPES = [(2, 300, 3, 128), (1, 257, 2, 64), (1, 64, 1, 8), (1, 513, 2, 80), (1, 130, 2, 256)]


def _cal():
    from liteattention_amd import calibration
    return calibration


def ref_stats(out, ref, rpb):
    """torch fp64: (B, H, nbins, 6) of the header's la_error_stat."""
    o, r = out.double(), ref.double()
    fin = torch.isfinite(o) & torch.isfinite(r)
    zero = torch.zeros((), dtype=torch.float64, device=o.device)
    d, rz = torch.where(fin, o - r, zero), torch.where(fin, r, zero)
    B, S, H, D = o.shape
    nb = -(-S // rpb)

    def bins(x, how):                                      # (B, S, H, D) -> (B, H, nbins)
        x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, nb * rpb - S)).reshape(B, nb, rpb, H, D).permute(0, 3, 1, 2, 4).reshape(B, H, nb, -1)
        return x.sum(-1) if how == "sum" else x.amax(-1)

    return torch.stack([bins(d.abs(), "sum"), bins(rz.abs(), "sum"), bins(d * d, "sum"), bins(rz * rz, "sum"), bins(d.abs(), "max"),
                        bins((~fin).double(), "sum")], dim=-1)


def check(got, want):
    assert got.shape == want.shape and got.dtype == torch.float64
    torch.testing.assert_close(got[..., :4], want[..., :4], rtol=1e-9, atol=0.0)
    assert torch.equal(got[..., 4:], want[..., 4:])


def make(shape, dtype, seed, dev, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(shape, generator=g)).to(dtype).to(dev)


@pytest.mark.parametrize("shape", SHAPES)
def test_grid_of_shapes_bins_and_dtype_pairs_matches_torch_fp64(shape):
    cal, dev = _cal(), torch.device("cuda", 0)
    B, S, H, D = shape
    base = make(shape, torch.float32, 1, dev)
    noise = make(shape, torch.float32, 2, dev, 0.03)
    for odt in DTYPES:
        for rdt in DTYPES:
            out, ref = (base + noise).to(odt), base.to(rdt)
            for rpb in (S, 256, 64, 1):
                es = cal.output_error(out, ref, rows_per_bin=rpb)
                assert es.stats.shape == (B, H, -(-S // rpb), 6)
                want = ref_stats(out, ref, rpb)
                check(es.stats, want)
                assert (want[..., 0] > 0).all() and (want[..., 5] == 0).all()
    # the reductions over bins, and the default bin
    es = cal.output_error(out, ref)
    assert es.rows_per_bin == min(S, 256)
    want = ref_stats(out, ref, S)[:, :, 0]
    torch.testing.assert_close(es.rel_l1, want[..., 0] / want[..., 1], rtol=1e-9, atol=0.0)
    torch.testing.assert_close(es.rel_l2, (want[..., 2] / want[..., 3]).sqrt(), rtol=1e-9, atol=0.0)
    assert torch.equal(es.max_abs, want[..., 4]) and torch.equal(es.nonfinite, torch.zeros(B, H, dtype=torch.int64, device=dev))
    wb = ref_stats(out, ref, es.rows_per_bin)
    torch.testing.assert_close(es.per_bin("rel_l1"), wb[..., 0] / wb[..., 1], rtol=1e-9, atol=0.0)
    assert torch.equal(es.per_bin("max_abs"), wb[..., 4])


def test_strided_operands():
    cal, dev = _cal(), torch.device("cuda", 0)
    B, S, H, D = 2, 300, 2, 128
    wide_o = make((B, S, 5, D), torch.bfloat16, 3, dev)
    wide_r = make((B, 2 * S, 3, D), torch.float32, 4, dev)
    out = wide_o[:, :, 1:3]                                 # a head slice of a wider tensor
    ref = wide_r[:, ::2, 1:3]                               # ... against every other row of another one: different strides, another dtype
    assert not out.is_contiguous() and not ref.is_contiguous() and out.stride() != ref.stride()
    for rpb in (S, 64):
        check(cal.output_error(out, ref, rows_per_bin=rpb).stats, ref_stats(out, ref, rpb))
        check(cal.output_error(ref, out, rows_per_bin=rpb).stats, ref_stats(ref, out, rpb))
    packed = make((B, S, 3, H, D), torch.float16, 5, dev)   # a packed qkv-like layout: (B, S, 3, H, D)[:, :, 2]
    check(cal.output_error(packed[:, :, 2], out, rows_per_bin=256).stats, ref_stats(packed[:, :, 2], out, 256))
    with pytest.raises(ValueError):
        cal.output_error(out.transpose(2, 3), ref.transpose(2, 3))        # the last dimension is not contiguous
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        cal.output_error(wide_o[:, :, :, 4:68], wide_o[:, :, :, 0:64])      # rows that start 8 bytes into a 16-byte line


@pytest.mark.parametrize("odt,rdt", [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float16)])
def test_non_finite_elements_are_counted_once_and_left_out(odt, rdt):
    cal, dev = _cal(), torch.device("cuda", 0)
    B, S, H, D, rpb = 2, 300, 3, 128, 64
    out, ref = make((B, S, H, D), odt, 6, dev), make((B, S, H, D), rdt, 7, dev)
    clean = cal.output_error(out, ref, rows_per_bin=rpb).stats.clone()
    nan, inf = float("nan"), float("inf")
    o2, r2 = out.clone(), ref.clone()
    o2[0, 5, 1, 7], o2[0, 6, 1, 0], o2[0, 7, 1, 127] = nan, inf, -inf            # in out            (batch 0, head 1, bin 0): 3
    r2[1, 70, 2, 9], r2[1, 71, 2, 10] = nan, -inf                                 # in ref            (batch 1, head 2, bin 1): 2
    o2[1, 299, 0, 64], r2[1, 299, 0, 64] = inf, inf                               # in both, same place (batch 1, head 0, bin 4): 1, not 2
    o2[1, 298, 0, 3], r2[1, 298, 0, 3] = nan, 1.0
    r2[1, 298, 0, 4] = inf                                                        # ... and two more in that bin: 3
    got = cal.output_error(o2, r2, rows_per_bin=rpb).stats
    check(got, ref_stats(o2, r2, rpb))
    touched = torch.zeros(B, H, 5, dtype=torch.bool, device=dev)
    touched[0, 1, 0] = touched[1, 2, 1] = touched[1, 0, 4] = True
    assert got[..., 5][touched].tolist() == [3.0, 3.0, 2.0] and (got[..., 5][~touched] == 0).all()
    assert torch.equal(got[~touched], clean[~touched])                            # every other head and bin: bit for bit the clean run
    assert torch.isfinite(got).all()
    es = cal.output_error(o2, r2, rows_per_bin=rpb)
    assert es.nonfinite.tolist() == [[0, 3, 0], [3, 0, 2]] and torch.isfinite(es.rel_l1).all()


def test_neighbours_are_not_read_and_every_stat_is_written():
    from liteattention_amd import _cabi
    cal, dev = _cal(), torch.device("cuda", 0)
    B, S, H, D, rpb = 2, 130, 2, 64, 64
    dts = {torch.bfloat16: _cabi.LA_DTYPE_BF16, torch.float32: _cabi.LA_DTYPE_FP32}
    for odt, rdt in ((torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)):
        big_o = torch.full((B + 2, S + 2, H + 2, D), float("nan"), dtype=odt, device=dev)
        big_r = torch.full((B + 2, S + 2, H + 2, D), float("nan"), dtype=rdt, device=dev)
        out, ref = big_o[1:-1, 1:-1, 1:-1], big_r[1:-1, 1:-1, 1:-1]
        out.copy_(make((B, S, H, D), odt, 8, dev))
        ref.copy_(make((B, S, H, D), rdt, 9, dev))
        nb = -(-S // rpb)
        stats = torch.full((B * H * nb * 6 + 12,), float("nan"), dtype=torch.float64, device=dev)     # 6 guard values on either side
        rc = _cabi.load().la_output_error(out.data_ptr(), dts[odt], *out.stride()[:3], ref.data_ptr(), dts[rdt], *ref.stride()[:3],
                                          B, S, H, D, rpb, stats[6:].data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == _cabi.LA_OK
        body = stats[6:-6].view(B, H, nb, 6)
        assert not torch.isnan(body).any() and (body[..., 5] == 0).all()
        assert torch.isnan(stats[:6]).all() and torch.isnan(stats[-6:]).all()      # and nothing beside them
        check(body, ref_stats(out.contiguous(), ref.contiguous(), rpb))
        check(cal.output_error(out, ref, rows_per_bin=rpb).stats, body)


def test_launches_are_bit_reproducible_also_on_a_side_stream():
    cal, dev = _cal(), torch.device("cuda", 0)
    out, ref = make((2, 1300, 3, 128), torch.bfloat16, 10, dev), make((2, 1300, 3, 128), torch.float32, 11, dev)
    for rpb in (1300, 256):
        a = cal.output_error(out, ref, rows_per_bin=rpb).stats
        b = cal.output_error(out, ref, rows_per_bin=rpb).stats
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            c = cal.output_error(out, ref, rows_per_bin=rpb).stats
        torch.cuda.current_stream(dev).wait_stream(side)
        assert torch.equal(a, b) and torch.equal(a, c)
        # the same rows seen through another layout (a head slice of a wider copy): the order of the additions follows the shape alone
        wide = torch.zeros(2, 1300, 5, 128, dtype=torch.bfloat16, device=dev)
        wide[:, :, 1:4] = out
        assert torch.equal(cal.output_error(wide[:, :, 1:4], ref, rows_per_bin=rpb).stats, a)


def test_identical_inputs_give_exact_zeros():
    cal, dev = _cal(), torch.device("cuda", 0)
    for dt in DTYPES:
        x = make((1, 257, 2, 64), dt, 12, dev)
        st = cal.output_error(x, x.clone(), rows_per_bin=64).stats
        assert (st[..., [0, 2, 4, 5]] == 0).all() and (st[..., 1] > 0).all() and (st[..., 3] > 0).all()
        check(st, ref_stats(x, x, 64))
    # the same VALUES in another element type are the same numbers: bf16 values held in fp32
    xb = make((1, 257, 2, 64), torch.bfloat16, 13, dev)
    st = cal.output_error(xb, xb.float(), rows_per_bin=257).stats
    assert (st[..., [0, 2, 4, 5]] == 0).all()


def test_wrapper_refuses_what_the_kernel_does_not_take():
    cal, dev = _cal(), torch.device("cuda", 0)
    x = make((1, 64, 1, 8), torch.bfloat16, 14, dev)
    with pytest.raises(ValueError):
        cal.output_error(x, x[:, :32])
    with pytest.raises(ValueError):
        cal.output_error(x.cpu(), x.cpu())
    with pytest.raises(TypeError):
        cal.output_error(x.double(), x.double())
    with pytest.raises(ValueError, match="multiple of 8"):
        cal.output_error(x[..., :4], x[..., :4])
