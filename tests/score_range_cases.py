"""Score staircases for tests/test_gpu_score_range.py (no GPU needed; checked by tests/test_score_range_cases_cpu.py).

Every hand-scheduled forward body keeps O and the row sums relative to a reference maximum m_ref that follows the true running maximum
m_true only when some row of its WAVE has m_true > m_ref + tau (log2 units): then every row of the wave takes alpha = exp2(m_ref - m_true),
l *= alpha, O *= alpha, m_ref = m_true (gen_blocks.rare_rescale_block / rescale_o_block). ``staircase_qkv`` builds inputs whose row maxima
climb a prescribed staircase over the walked key tiles, so that this rare code runs at the product's own tau, and ``lazy_walk`` is the
fp64 model of it the CPU test reads the events from.

The inputs: q_i = g_i u + a n_i, k_j = b_tile(j) u + a n_j with u in {+-1}^D and the noise n made orthogonal to u before the cast, so the
score of (row i, key j) in log2 units is g_i * level(tile of j) up to a noise term of about 0.1 (b u is written in four digits, one
per quarter of the head dim, each exact in e4m3: ``_digits``). Key tile t is
walked at position KT - 1 - t (lists run from the last tile down), level(position) is the cumulative sum of ``steps(tau)``.

16-bit: b = level / (sqrt(D) log2 e) under the default softmax scale D^-0.5. e4m3: per-head q / k / v descales that differ between the
heads with q_descale * k_descale = P_h / sqrt(D), i.e. c = log2 e * P_h / D and b = level / (log2 e * P_h) whatever the head dim: the
elements stay below 32 where e4m3 still has steps of 2, and tau / c (what the kernel compares with) differs per head."""
import math

import torch

F8 = torch.float8_e4m3fn
SQ, SK, H, BN = 300, 792, 2, 64
KT = -(-SK // BN)                       # 13 key tiles, the last of 24 keys
LOG2E = math.log2(math.e)
GAINS = (1.0, 0.5, 0.0, -1.0, 0.25, 1.0, 0.75, -0.5)          # mixed rows, by row % 8
DESC_GAINS = (-1.0, -0.5, -0.25, -0.75)                        # descending rows, by row % 4
FLAT_ROWS, DESC_ROWS = slice(128, 192), slice(256, 300)
MIXED_ROWS = (slice(0, 128), slice(192, 256))
TAUS = {"s8": 8.0, "s2": 2.0, "s32": 32.0}                     # schedule name -> the tau it is built around
FP8_PRODUCT = (8.0, 10.5)                                      # P_h: sqrt(D) * q_descale * k_descale of head h
FP8_V_DESCALE = (0.5, 1.25)


def steps(tau):
    """Growth of a gain-1 row per walked position 1 .. 12 of the dense walk, in log2 units (position 0 is level 0):
    1: one step in (tau, tau + 1): a trigger at position 1;  2, 3: two sub-tau steps, the second crosses tau through the accumulated lag;
    4: a step above 2 tau;  5: flat;  6: 165 - alpha underflows to 0;  7: flat;  8: a tile 100 below the maximum;  9: back at the maximum
    (no growth);  10, 11: two sub-tau steps that stay below tau together;  12: a sub-tau step that crosses it: a trigger at the last position."""
    return [tau + 0.5, 0.6 * tau, 0.6 * tau, 2.0 * tau + 4.0, 0.0, 165.0, 0.0, -100.0, 100.0, 0.45 * tau, 0.45 * tau, 0.6 * tau]


def levels(schedule):
    """Level per walked position 0 .. KT - 1 (log2 units, gain 1)."""
    out = [0.0]
    for s in steps(TAUS[schedule]):
        out.append(out[-1] + s)
    assert len(out) == KT
    return out


def row_gains():
    g = torch.tensor(GAINS, dtype=torch.float64)[torch.arange(SQ) % 8]
    g[FLAT_ROWS] = 0.0
    g[DESC_ROWS] = torch.tensor(DESC_GAINS, dtype=torch.float64)[torch.arange(DESC_ROWS.start, DESC_ROWS.stop) % 4]
    return g


NDIG = 4                                # the level of a key is written in NDIG "digits", one per block of D / NDIG head-dim columns


def _orthogonal_noise(n, D, u, g):
    """randn (n, D) with the component along u removed in every digit block, so that the noise of q does not see the levels of k."""
    x = torch.randn(n, D, generator=g, dtype=torch.float64).view(n, NDIG, D // NDIG)
    ub = u.view(NDIG, D // NDIG)
    return (x - (x * ub).sum(-1, keepdim=True) * ub / (D // NDIG)).reshape(n, D)


def _digits(x):
    """x (n,) -> (n, NDIG) e4m3-representable values that sum to x to about 16 bits: greedy rounding of the remainder. A level of 350 log2
    units next to steps of 1 needs more than the 4 bits of one e4m3 element (or the 8 of bf16): each digit is exact in every input type."""
    out, rem = [], x.clone()
    for _ in range(NDIG):
        d = rem.float().to(F8).double()
        out.append(d)
        rem = rem - d
    return torch.stack(out, dim=1)


def staircase_qkv(dtype, D, schedule, noise=None, seed=1):
    """(q, k, v, descales): q (1, SQ, H, D), k, v (1, SK, H, D) already cast to `dtype` on the CPU; descales = {} for the 16-bit types,
    the three (1, H) fp32 per-head descales for e4m3."""
    noise = (0.125 if dtype == F8 else 0.25) if noise is None else noise
    g = torch.Generator().manual_seed(seed + D)
    u = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).to(torch.float64)
    lv = torch.tensor(levels(schedule), dtype=torch.float64).flip(0)             # per key tile
    lv_keys = lv.repeat_interleave(BN)[:SK]
    gains = row_gains()
    qs, ks, vs = [], [], []
    ds = {}
    if dtype == F8:
        prod = torch.tensor(FP8_PRODUCT, dtype=torch.float64) / math.sqrt(D)
        qd = torch.tensor([1.5, 0.75], dtype=torch.float64)
        ds = {"q_descale": qd.float()[None], "k_descale": (prod / qd).float()[None], "v_descale": torch.tensor(FP8_V_DESCALE)[None]}
    for h in range(H):
        unit = LOG2E * (FP8_PRODUCT[h] if dtype == F8 else math.sqrt(D))        # log2 units of one unit of b at gain 1
        qs.append(gains[:, None] * u[None] + noise * _orthogonal_noise(SQ, D, u, g))
        b = _digits(lv_keys * NDIG / unit).repeat_interleave(D // NDIG, dim=1)                   # (SK, D): digit i on the columns of block i
        ks.append(b * u[None] + noise * _orthogonal_noise(SK, D, u, g))
        v = torch.randn(SK, D, generator=g, dtype=torch.float64)
        vs.append(v / FP8_V_DESCALE[h] if dtype == F8 else v)
    q, k, v = [torch.stack(x, dim=1)[None].float().to(dtype) for x in (qs, ks, vs)]
    return q, k, v, ds


def log2_scale(D, ds, h, softmax_scale=None):
    """c of head h: score * c is in log2 units (fp64 of what the kernels form in fp32)."""
    c = (D ** -0.5 if softmax_scale is None else softmax_scale) * LOG2E
    if ds:
        c *= float(ds["q_descale"][0, h]) * float(ds["k_descale"][0, h])
    return c


def scores_log2(q, k, ds, h, softmax_scale=None):
    """(SQ, SK) fp64 scores of head h in log2 units, from the cast inputs."""
    return (q[0, :, h].double() @ k[0, :, h].double().T) * log2_scale(q.shape[-1], ds, h, softmax_scale)


def v_f64(v, ds, h):
    return v[0, :, h].double() * (float(ds["v_descale"][0, h]) if ds else 1.0)


# ---------------------------------------------------------------------------------------------------------------- read lists
# ranges of key tiles (start, end inclusive, descending). Position = KT - 1 - tile.
LIST_H0 = [12, 10, 8, 8, 6, 3, 1, 0]        # positions 0 1 2 | 4 | 6 7 8 9 | 11 12: a trigger on the first tile after a gap (4, 6), one at the last position
LIST_H1 = [12, 11, 8, 8, 5, 3, 1, 1]        # positions 0 1 | 4 | 7 8 9 | 11: ends on a sub-tau step - the walk finishes with a lag
LIST_H0_LATE = [11, 10, 8, 8, 6, 3, 1, 0]   # the same without the first position: q-tile 1 (the second half of a half-vote workgroup)
LIST_H1_LATE = [11, 11, 8, 8, 5, 3, 1, 1]   #   starts from the empty state; its first tile is a trigger step of the half that began at position 0


def list_ranges(h, m):
    """Ranges of head h, q-tile m: q-tile 1 starts one position late."""
    return ((LIST_H0, LIST_H0_LATE), (LIST_H1, LIST_H1_LATE))[h][1 if m == 1 else 0]


def read_lists(block_m):
    """int32 (1, H, Qt, KT + 1) read lists."""
    qt = -(-SQ // block_m)
    out = torch.zeros(1, H, qt, KT + 1, dtype=torch.int32)
    for h in range(H):
        for m in range(qt):
            r = list_ranges(h, m)
            out[0, h, m, 0] = len(r)
            out[0, h, m, 1:1 + len(r)] = torch.tensor(r, dtype=torch.int32)
    return out


def walk_of(ranges):
    return [t for i in range(0, len(ranges), 2) for t in range(ranges[i], ranges[i + 1] - 1, -1)]


DENSE_WALK = list(range(KT - 1, -1, -1))


def finite_thr(schedule):
    """Threshold of the finite-thr list launch: between the margins of the positions where nothing grows (about 0: the zero rows of the
    ragged last q-tile give exactly 0, so the descending q-tile drops every tile it may) and the smallest sub-tau step of the rising rows
    (0.45 tau is never walked alone by these lists; 0.6 tau is)."""
    return 0.4 * TAUS[schedule]


# ---------------------------------------------------------------------------------------------------------------- fp64 model
def lazy_walk(s2, v, walk, tau, group, rows=None, fault=None):
    """fp64 online softmax over the key tiles `walk` with the bodies' lazy reference maximum. s2: (rows, SK) scores in log2 units;
    v: (SK, Dv); `group` rows share one trigger decision (a wave: 64 rows at head dims <= 128, 32 above); rows [r0, r1) of the problem
    (a q-tile; waves are counted from r0). fault: None or (kind, position) with kind
      "o_once"   alpha not applied to O at the trigger of that position,
      "o_never"  alpha applied to l but never to O,
      "lse_true" the LSE formed from m_true while the sums are relative to m_ref.
    Returns (o, lse (natural log), trace) with trace[p] = dict(step, lag_before, own, wave) per walked position p >= 1."""
    r0, r1 = rows if rows is not None else (0, s2.shape[0])
    s2 = s2[r0:r1]
    n = s2.shape[0]
    grp = torch.arange(n) // group
    ngrp = int(grp.max()) + 1
    m_true = m_ref = l = O = None
    trace = [None]
    for p, t in enumerate(walk):
        keys = slice(t * BN, min((t + 1) * BN, SK))
        S = s2[:, keys]
        m_loc = S.max(dim=1).values
        if p == 0:
            m_true, m_ref = m_loc.clone(), m_loc.clone()
            l, O = torch.zeros(n, dtype=torch.float64), torch.zeros(n, v.shape[1], dtype=torch.float64)
        else:
            new = torch.maximum(m_true, m_loc)
            step, lag_before = new - m_true, m_true - m_ref
            m_true = new
            own = m_true > m_ref + tau
            wave = torch.zeros(ngrp, dtype=torch.bool).index_put_((grp,), own, accumulate=True)[grp]
            alpha = torch.where(wave, torch.exp2(m_ref - m_true), torch.ones_like(m_ref))
            l = l * alpha
            if not (fault == ("o_once", p) or (fault is not None and fault[0] == "o_never")):
                O = O * alpha[:, None]
            m_ref = torch.where(wave, m_true, m_ref)
            trace.append(dict(step=step, lag_before=lag_before, own=own, wave=wave))
        P = torch.exp2(S - m_ref[:, None])
        l = l + P.sum(dim=1)
        O = O + P @ v[keys]
    base = m_true if (fault is not None and fault[0] == "lse_true") else m_ref
    return O / l[:, None], (base + torch.log2(l)) * math.log(2.0), trace


def dense_f64(s2, v, walk=None):
    """Plain fp64 softmax over the keys of the walked tiles: (o, lse)."""
    keys = torch.cat([torch.arange(t * BN, min((t + 1) * BN, SK)) for t in (walk or DENSE_WALK)])
    s = s2[:, keys] * math.log(2.0)
    return torch.softmax(s, dim=1) @ v[keys], torch.logsumexp(s, dim=1)


def uniform_reference(v, ds, bm, listed):
    """O = mean of V over the walked keys, LSE = ln of their number (fp64): (1, SQ, H, D), (1, H, SQ)."""
    D = v.shape[-1]
    o, lse = torch.empty(1, SQ, H, D, dtype=torch.float64), torch.empty(1, H, SQ, dtype=torch.float64)
    for h in range(H):
        vh = v_f64(v, ds, h)
        for m in range(-(-SQ // bm)):
            walk = walk_of(list_ranges(h, m)) if listed else DENSE_WALK
            keys = torch.cat([torch.arange(t * BN, min((t + 1) * BN, SK)) for t in walk])
            rows = slice(m * bm, min((m + 1) * bm, SQ))
            o[0, rows, h] = vh[keys].mean(dim=0)
            lse[0, h, rows] = math.log(len(keys))
    return o, lse


def events(trace, tau):
    """Which of the events a - e some row shows on a walk (trace of ``lazy_walk``): dict name -> bool."""
    last = len(trace) - 1
    ev = dict(a=False, b=False, c=False, d=False, e_first=False, e_last=False)
    for p in range(1, last + 1):
        t = trace[p]
        st, lag, own = t["step"], t["lag_before"], t["own"]
        if tau > 0:
            ev["a"] |= bool(((lag > 0) & (lag < tau) & (st > 0) & (st < tau) & own).any())
            ev["b"] |= bool(((lag == 0) & (st > tau) & (st < tau + 1) & own).any())
        ev["c"] |= bool(((st > 2 * tau) & (st < 160) & own).any())
        ev["d"] |= bool(((st >= 160) & own).any())
    ev["e_first"] = bool(trace[1]["own"].any())
    ev["e_last"] = bool(trace[last]["own"].any())
    return ev
