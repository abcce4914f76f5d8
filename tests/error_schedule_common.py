"""Shared by tests/test_error_schedule_cpu.py and tests/test_gpu_error_schedule.py: the workload, the bound rule and the CPU backend
of ``calibrate_error_schedule`` built on ``oracle.qkskip_fwd`` (no test in here).

Workload: ``helpers.fragmented_qkv(1, 1024, 2, 128, seed=3, step=t, steps=4)``, tiles 256 x 64 (Qt = 4, Kt = 16: 128 tiles), 4 steps.
Metric: relative L1 per head against the dense output of the same step, worst head.
Bounds: e_hi[t] = the error of the CONSTANT threshold -0.001 at step t (a baseline on code that existed before the calibrator, never
the calibrator's own output); bounds[t] = (0.1, 0.25, 0.5)[t - 1] * e_hi[t] for t = 1 ... 3. Step 0 reads the list of all tiles, so its
output is the dense one up to the rounding of the result: two bf16 roundings of one value differ by at most one ulp, 2^-7 relative,
per element, hence bounds[0] = 2^-7 (the oracle reproduces its dense result exactly there: error 0)."""
import torch

from helpers import fragmented_qkv

B, S, H, D, SEED, STEPS = 1, 1024, 2, 128, 3, 4
BM, BN = 256, 64
QT, KT = S // BM, S // BN
HI_THR = -0.001
BOUND_FACTORS = (0.1, 0.25, 0.5)
BOUND_STEP0 = 2.0 ** -7
GRID = (-6.0, -5.0, -4.5, -4.0, -3.5)


def qkv_cpu(t):
    return fragmented_qkv(B, S, H, D, seed=SEED, step=t, steps=STEPS)


def bounds_from(e_hi):
    return [BOUND_STEP0] + [f * e for f, e in zip(BOUND_FACTORS, e_hi[1:])]


def rel_l1_worst_head(out, ref):
    """torch fp64: max over (batch, head) of sum|out - ref| / sum|ref|."""
    o, r = out.detach().cpu().double(), ref.detach().cpu().double()
    return float(((o - r).abs().sum(dim=(1, 3)) / r.abs().sum(dim=(1, 3))).max())


class OracleBackend:
    """The seven methods ``calibrate_error_schedule`` asks of a backend, on the CPU oracle."""

    def __init__(self):
        from oracle import oracle as orc
        self.orc = orc
        self.md = orc.expand_must_do_ref([0, 0], BN, KT + 1)
        self.reset()

    def reset(self):
        self.lists = [self.orc.init_skip_list_ref(B, QT, KT, H)[0].contiguous() for _ in range(2)]     # [read, write] by phase
        self.phase = 0

    def snapshot(self):
        return [x.clone() for x in self.lists], self.phase

    def restore(self, snap):
        self.lists, self.phase = [x.clone() for x in snap[0]], snap[1]

    def step(self, t, thr):
        q, k, v = qkv_cpu(t)
        rd, wr = self.lists[self.phase], self.lists[1 - self.phase]
        o, _, _ = self.orc.qkskip_fwd(q, k, v, block_m=BM, block_n=BN, read_list=rd, write_list=wr, must_do_list=self.md, thr=thr)
        self.phase = 1 - self.phase
        return o

    def dense(self, t):
        q, k, v = qkv_cpu(t)
        return self.orc.qkskip_fwd(q, k, v, block_m=BM, block_n=BN)[0]

    def error(self, out, ref):
        return rel_l1_worst_head(out, ref)

    def skip_fraction(self):
        return 1.0 - self.orc.listed_tiles(self.lists[self.phase]) / (B * H * QT * KT)


def run_thresholds(backend, thresholds):
    """Steps 0 ... STEPS - 1 at ``thresholds[t]`` from a fresh state: (error of every step against dense, skip fraction of the list
    every step READ, skip fraction of the list the last step wrote)."""
    backend.reset()
    errs, skips = [], []
    for t in range(STEPS):
        skips.append(backend.skip_fraction())
        errs.append(backend.error(backend.step(t, thresholds[t]), backend.dense(t)))
    return errs, skips, backend.skip_fraction()


def best_constant(backend, bounds):
    """The constant of GRID that meets every bound and skips most at the last step: (thr, skip fraction of the last read list)."""
    best = None
    for thr in GRID:
        errs, skips, _ = run_thresholds(backend, [thr] * STEPS)
        if all(e <= b for e, b in zip(errs, bounds)) and (best is None or skips[-1] > best[1]):
            best = (thr, skips[-1])
    return best
