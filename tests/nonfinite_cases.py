"""Inputs and expectations of tests/test_gpu_nonfinite.py (no GPU needed; proved by tests/test_nonfinite_cases_cpu.py).

Non-finite data a launch legitimately READS must stay in the results that depend on it. Three families:

A  whole heads of K, V, K and V, or Q are poison for a seeded half of the (batch, head) pairs; the *twin* is the same input with finite
   randn data in those heads (the base tensors: the poisoned input is made from the twin, so the two differ nowhere else).
B  inside one item: three V elements (B1), three query rows (B2), one key row (B3) of one head.
C  is about the caller's workspace and needs no inputs of its own.

Poison patterns are ``layout_cases.POISON_BITS`` (the sign alternates along the head dimension); every comparison is on raw bits.
``softmax64`` is the plain fp64 softmax the finite / non-finite expectations come from."""
import collections

import torch

import layout_cases as lc
from layout_cases import F8

KINDS = ("nan", "inf", "huge")
BN = 64                                            # key tile of every body


def kinds(dtype):
    """The poison kinds the type has (e4m3fn has no infinity)."""
    return [p for p in KINDS if (dtype, p) in lc.POISON_BITS]


def pattern(dtype, kind, D, device="cpu"):
    """(D,) raw bit patterns of one poisoned row."""
    even, odd = lc.poison_bits(dtype, kind)
    pat = torch.empty(D, dtype=lc.raw_dtype(dtype), device=device)
    pat[0::2] = even
    pat[1::2] = odd
    return pat


def softmax64(q, k, v, descales=None, scale=None, keys=None):
    """Plain softmax attention in fp64: (out (B, Sq, H, D), lse (B, H, Sq)). q (B, Sq, H, D); k, v (B, Sk, Hk, D) of any float type;
    ``descales``: the e4m3 per-(batch, kv head) factors; ``keys``: bool (Sk,), the keys a read list walks (None: all)."""
    qf, kf, vf = [x.to(torch.float32).double() for x in (q, k, v)]
    g = qf.shape[2] // kf.shape[2]
    kf, vf = kf.repeat_interleave(g, dim=2), vf.repeat_interleave(g, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", qf, kf) * (q.shape[-1] ** -0.5 if scale is None else scale)
    if descales:
        qd, kd, vd = [descales[n].double().repeat_interleave(g, dim=1) for n in ("q_descale", "k_descale", "v_descale")]
        s = s * (qd * kd)[:, :, None, None]
        vf = vf * vd[:, None, :, None]
    if keys is not None:
        s, vf = s[..., keys], vf[:, keys]
    lse = torch.logsumexp(s, dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", torch.exp(s - lse[..., None]), vf)
    return out, lse


# --------------------------------------------------------------------------------------------------- family A: poisoned heads
A_H, A_HK = 4, 2                                   # GQA: H = 2 Hk
A_KEY_LENS = (1, 13, 65, 130, 203, 300, 560)
A_SK_MAX = lc.LIST_S                               # 600: the list launches reuse the ranges of layout_cases (ten tiles)
A_RAGGED = 44                                      # query rows of the second, ragged q-tile
A_SQ_MAX = 256 + A_RAGGED
A_TARGETS = ("k", "v", "kv", "q")
FINITE_THR = -3.0                                  # the library's default threshold
Expect = collections.namedtuple("Expect", "out lse")      # out: "nonfinite" | "zero"; lse: "nonfinite" | "twin" (the twin's bits) | "neg_inf"


def walk_len(sk):
    """Tiles a dense walk over `sk` keys has."""
    return -(-sk // BN)


def a_seqlen_q(item_rows):
    """Two q-tiles of `item_rows` rows, the second one ragged."""
    return item_rows + A_RAGGED


def a_base(D, B, dtypes, seed=0):
    """{dtype: (q (B, A_SQ_MAX, H, D), k, v (B, A_SK_MAX, Hk, D), descales)}: the twin. Batch entry b comes from its own seed, so the
    first entries do not depend on B; every launch takes the leading rows [:Sq], [:Sk] of these. One fp32 randn draw serves all types."""
    shapes = ((A_SQ_MAX, A_H, D), (A_SK_MAX, A_HK, D), (A_SK_MAX, A_HK, D))
    out = {dt: [torch.empty((B, *s), dtype=dt) for s in shapes] for dt in dtypes}
    ds = torch.empty(B, 3, A_HK)
    g = torch.Generator()
    for b in range(B):
        g.manual_seed((seed * 1009 + D) * 100003 + b)
        for i, s in enumerate(shapes):
            x = torch.randn(*s, generator=g)
            for dt in dtypes:
                lc.raw(out[dt][i])[b] = lc.raw(x.to(dt))
        ds[b] = 0.5 + torch.rand(3, A_HK, generator=g)
    names = ("q_descale", "k_descale", "v_descale")
    return {dt: (*out[dt], {n: ds[:, i].contiguous() for i, n in enumerate(names)} if dt == F8 else {}) for dt in dtypes}


def a_poisoned_kv(B, seed=1):
    """bool (B, Hk): one seeded kv head of the two per batch entry - half of the pairs, neither set empty in any entry."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, A_HK, dtype=torch.bool)
    m[torch.arange(B), torch.randint(0, A_HK, (B,), generator=g)] = True
    return m


def a_poisoned_q(B, seed=2):
    """bool (B, H): two seeded query heads of the four per batch entry."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, A_H, generator=g).argsort(dim=1).argsort(dim=1) < A_H // 2


def a_poisoned_heads(target, B):
    """bool (B, H): the query heads whose result depends on the poison of `target`."""
    return a_poisoned_q(B) if target == "q" else a_poisoned_kv(B).repeat_interleave(A_H // A_HK, dim=1)


def poison_heads(t, mask, kind):
    """A copy of (B, S, Hx, D) `t` with every element of the heads ``mask`` (B, Hx) poison."""
    pat = pattern(t.dtype, kind, t.shape[-1], t.device)
    return torch.where(mask.to(t.device)[:, None, :, None], pat, lc.raw(t)).view(t.dtype)


def a_poison(q, k, v, target, kind):
    """The poisoned (q, k, v) of a family-A case; the arguments are the twin."""
    B = q.shape[0]
    if target == "q":
        return poison_heads(q, a_poisoned_q(B), kind), k, v
    m = a_poisoned_kv(B)
    return q, (poison_heads(k, m, kind) if "k" in target else k), (poison_heads(v, m, kind) if "v" in target else v)


def a_expectation(target, kind, encoded=False):
    """What the GPU test asserts on a POISONED head (None: nothing). NaN only: with `huge` fp32 accumulation legitimately overflows where
    fp64 does not, and what alternating infinities add up to is not what this family is about. The LSE does not depend on V.
    ``encoded``: the e4m3 bodies with the byte-encoded P (LA_FP8_P=encoded) - there the hardware decides: v_cvt_pk_u8_f32 turns a NaN
    score into byte 0, P = 0, so a key with a NaN score is a key that is not there; a row without keys has out = 0 and lse = -inf
    (with V NaN as well, out is 0 x NaN)."""
    if kind != "nan":
        return None
    if encoded and target != "v":
        return Expect("nonfinite" if target == "kv" else "zero", "neg_inf")
    return Expect("nonfinite", "twin" if target == "v" else "nonfinite")


# packed batch: poisoned sequences of 560 keys alternate with clean ones of 13, 65 and 130 keys
P_LONG, P_SHORT = 560, (13, 65, 130)


def packed_lens(n_seq):
    """(key lengths, poisoned flags) of `n_seq` sequences: 560* 13 560* 65 560* 130 560* 13 ... (* = every K / V row poison)."""
    lens = [P_LONG if i % 2 == 0 else P_SHORT[(i // 2) % len(P_SHORT)] for i in range(n_seq)]
    return lens, [i % 2 == 0 for i in range(n_seq)]


def cu(lens):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)


def pack(t, lens):
    """(sum lens, Hx, D): the leading rows [:lens[b]] of every batch entry of (B, S, Hx, D) `t`, packed."""
    return torch.cat([t[b, :n] for b, n in enumerate(lens)])


def packed_row_mask(lens, flags):
    """bool (sum lens,): rows of the flagged sequences."""
    return torch.cat([torch.full((n,), bool(f)) for n, f in zip(lens, flags)])


def poison_packed_rows(t, rows, kind):
    """A copy of packed (T, Hx, D) `t` with the rows ``rows`` (bool (T,)) poison in every head."""
    pat = pattern(t.dtype, kind, t.shape[-1], t.device)
    return torch.where(rows.to(t.device)[:, None, None], pat, lc.raw(t)).view(t.dtype)


# ------------------------------------------------------------------------------------------ family B: inside one item
B_B, B_H, B_HK, B_SQ, B_SK = 2, 4, 2, 300, 203     # the shape of layout_cases' SHAPES[2]: four key tiles, ragged on both sides
B_BATCH, B_KV_HEAD, B_Q_HEAD = 0, 0, 1             # where the poison sits: the FIRST items, everything after them is clean
B2_ROWS = (0, 129, B_SQ - 1)
B3_KEY = 69
B_LIST_RANGES = [3, 3, 1, 0]                       # read list of every q-tile: tiles 3 | 1 0 - every poisoned key is walked, tile 2 is not


def b1_positions(D):
    """(key, column) of the three poisoned V elements."""
    return ((B_SK - 1, 0), (69, D - 1), (0, D // 2))


def b_listed_keys():
    keys = torch.zeros(B_SK, dtype=torch.bool)
    for t in (3, 1, 0):
        keys[lc.tile_rows(t, BN, B_SK)] = True
    return keys


def b_heads_on_kv():
    """bool (B, H): the query heads that read the poisoned kv head."""
    m = torch.zeros(B_B, B_H, dtype=torch.bool)
    g = B_H // B_HK
    m[B_BATCH, B_KV_HEAD * g:(B_KV_HEAD + 1) * g] = True
    return m


def b_inputs(dtype, D, seed=0):
    """(q, k, v, descales) on the CPU."""
    g = torch.Generator().manual_seed(seed * 1009 + B_SQ * 7 + B_SK + D)
    q = torch.randn(B_B, B_SQ, B_H, D, generator=g).to(dtype)
    k, v = [torch.randn(B_B, B_SK, B_HK, D, generator=g).to(dtype) for _ in range(2)]
    ds = {n: 0.5 + torch.rand(B_B, B_HK, generator=g) for n in ("q_descale", "k_descale", "v_descale")} if dtype == F8 else {}
    return q, k, v, ds


def b1_poison_v(v, kind):
    out = v.clone()
    pat = pattern(v.dtype, kind, v.shape[-1], v.device)
    for key, col in b1_positions(v.shape[-1]):
        lc.raw(out)[B_BATCH, key, B_KV_HEAD, col] = pat[col]
    return out


def b2_poison_q(q, kind):
    out = q.clone()
    for row in B2_ROWS:
        lc.raw(out)[B_BATCH, row, B_Q_HEAD] = pattern(q.dtype, kind, q.shape[-1], q.device)
    return out


def b3_poison_k(k):
    out = k.clone()
    lc.raw(out)[B_BATCH, B3_KEY, B_KV_HEAD] = pattern(k.dtype, "nan", k.shape[-1], k.device)
    return out


def nonfinite_masks(q, k, v, ds, keys=None):
    """(out (B, Sq, H, D), lse (B, H, Sq)) bool: where the plain fp64 softmax is NOT finite on exactly these inputs."""
    o, lse = softmax64(q, k, v, ds, keys=keys)
    return ~torch.isfinite(o), ~torch.isfinite(lse)


# ------------------------------------------------------------------------------------------------------ B4: the merge, directly
C_SPLITS, C_B, C_S, C_H, C_D = 3, 2, 37, 3, 64
C_LSE_AT = (1, 0, 5, 1)                            # (split, batch, row, head) of the NaN LSE
C_OUT_AT = (2, 1, 36, 0, 7)                        # (split, batch, row, head, column) of the NaN partial-output element


def combine_partials(dtype, seed=5):
    """(out_partial (n, B, S, H, D) `dtype`, lse_partial fp32, logical (n, B, S, H) with the row dimension contiguous)."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(C_SPLITS, C_B, C_S, C_H, C_D, generator=g).to(dtype)
    lse = torch.randn(C_SPLITS, C_B, C_H, C_S, generator=g).transpose(-1, -2)
    return o, lse


def combine_poison(o, lse, which):
    """which = "lse" or "out": one NaN in one split of one row. Returns (out_partial, lse_partial, (batch, row, head))."""
    o, lse = o.clone(), lse.clone()
    if which == "lse":
        lse[C_LSE_AT] = float("nan")
        return o, lse, C_LSE_AT[1:]
    o[C_OUT_AT] = float("nan")
    return o, lse, C_OUT_AT[1:4]
