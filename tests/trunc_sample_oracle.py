"""Float64 restatement of the truncated sampling contract (include/set_hip.h SetSampleOpts: temperature, top-k, top-p) on top
of oracle/philox_np, and the fixtures the GPU tests draw from.  tests/test_truncated_sampling_cpu.py pins it to brute force by
sorting and asserts, on the oracle alone, that every fixture keeps its top-p target clear of a group boundary and (nearly) every
draw clear of a CDF boundary — so tests/test_hip_truncated_sampling.py may demand exact kept sets and pinned draws."""
import numpy as np

from oracle import philox_np

NEUTRAL = (1.0, 0, 1.0)
BOUNDARY_MIN = 1e-4            # no fixture row's top-p target lies closer than this to a group boundary (fraction of the mass)
MARGIN_MIN = 1e-5              # a draw closer than this to a CDF boundary may legitimately become `alt`
MARGIN_SHARE = 0.01            # at most this share of a fixture's draws may be that close


def scaled(logits, temperature):
    """y = x * (1.0f / T) as the kernel forms it: float32 product with the float32 reciprocal"""
    inv = np.float32(1.0) / np.float32(temperature)
    return (np.asarray(logits, np.float32) * inv).astype(np.float32)


def kept_set(y, top_k, top_p):
    """y (R, V) -> (kept (R, V) bool, dist (R,)).  top-k (off at 0 or >= V): every y >= the top_k-th largest.  top-p (off at 1)
    over what top-k kept: value groups in descending order until their mass reaches top_p * M, the crossing group included
    whole.  dist = |top_p - c / M| for the nearest cumulative mass c at a boundary BETWEEN two value groups (inf without one,
    or with top-p off).  Comparisons are on values, so -0.0 and +0.0 are one group."""
    y = np.asarray(y, np.float64)
    R, V = y.shape
    kept = np.ones((R, V), bool)
    dist = np.full(R, np.inf)
    if 0 < top_k < V:
        tk = -np.partition(-y, top_k - 1, axis=1)[:, top_k - 1]
        kept = y >= tk[:, None]
    if top_p < 1.0:
        for r in range(R):
            m = np.exp(y[r] - y[r].max())
            vals, inv = np.unique(y[r][kept[r]], return_inverse=True)          # ascending; -0.0 == +0.0 merge
            gm = np.bincount(inv, weights=m[kept[r]], minlength=len(vals))[::-1]
            cum = np.cumsum(gm)
            M = cum[-1]
            g = int(np.searchsorted(cum, top_p * M, side="left"))              # first group with cum >= top_p * M
            g = min(g, len(vals) - 1)
            kept[r] &= y[r] >= vals[::-1][g]
            if len(vals) > 1:
                dist[r] = float(np.abs(top_p - cum[:-1] / M).min())
    return kept, dist


def enumeration(V, reg):
    """the kernel's fixed order of the vocabulary: register path thread tid owns (tid + 256 q) * 4 + e; generic path tid + 256 i"""
    if reg:
        nq = -(-V // 1024)
        order = np.array([(tid + 256 * q) * 4 + e for tid in range(256) for q in range(nq) for e in range(4)])
    else:
        ni = -(-V // 256)
        order = np.array([tid + 256 * i for tid in range(256) for i in range(ni)])
    return order[order < V]


class Draw:
    """ids / margin / alt (B,) as philox_np.categorical_draw defines them; kept, dist, lse (R,), logp (R, V) of the distinct rows"""


def truncated_draw(logits, opts, seed, offset, t=0, reg=True, row_of=None):
    """The truncated pick for rows b < B, row b holding logits[row_of[b]] (row_of None: one row each).  logits (R, V) float32 as
    the kernel forms them (slabs summed in index order, bias added, in float32); opts = (temperature, top_k, top_p)."""
    T, top_k, top_p = opts
    y = scaled(logits, T).astype(np.float64)
    R, V = y.shape
    row_of = np.arange(R) if row_of is None else np.asarray(row_of)
    B = len(row_of)
    d = Draw()
    d.kept, d.dist = kept_set(y, top_k, top_p)
    ymax = y.max(1, keepdims=True)
    with np.errstate(divide="ignore"):
        pe = np.where(d.kept, np.exp(y - ymax), 0.0)
        d.lse = ymax[:, 0] + np.log(pe.sum(1))
        d.logp = np.where(d.kept, y - d.lse[:, None], -np.inf)
    order = enumeration(V, reg)
    u = philox_np.sample_uniform(seed, offset, np.arange(B), t).astype(np.float64)
    d.ids, d.margin, d.alt = np.zeros(B, np.int64), np.zeros(B), np.zeros(B, np.int64)
    per_row = {}
    for b in range(B):
        r = int(row_of[b])
        if r not in per_row:
            words = order[d.kept[r][order]]                                    # kept words in enumeration order
            per_row[r] = (words, np.cumsum(pe[r][words]))
        words, cdf = per_row[r]
        target = u[b] * cdf[-1]
        j = min(int(np.searchsorted(cdf, target, side="right")), len(words) - 1)
        lo = cdf[j - 1] if j else 0.0
        d.ids[b] = words[j]
        d.margin[b] = min(target - lo, cdf[j] - target) / cdf[-1]
        below = (target - lo) < (cdf[j] - target)
        d.alt[b] = words[max(j - 1, 0)] if below else words[min(j + 1, len(words) - 1)]
    return d


# ------------------------------------------------------------------------------------------- fixtures of the GPU tests
def slab_sum32(slabs, bias):
    """the kernel's float32 logit: slab 0, + slab 1, ..., + bias"""
    x = np.asarray(slabs[0], np.float32).copy()
    for s in slabs[1:]:
        x = (x + np.asarray(s, np.float32)).astype(np.float32)
    return x if bias is None else (x + np.asarray(bias, np.float32)[None]).astype(np.float32)


GRID_R, GRID_B = 8, 64
GRID_V = [(203, 204), (203, 205), (1024, 1024), (1028, 1028), (9490, 9492), (12288, 12288), (12292, 12292)]      # (V, ld)
GRID_N = [1, 3]
GRID_T = [0.5, 1.0, 2.0]


def grid_options(V):
    return ([(k, 1.0) for k in (1, 2, 5, 64, V - 1, V, V + 7)] + [(0, p) for p in (1e-6, 0.5, 0.9)] +
            [(64, p) for p in (1e-6, 0.5, 0.9)])


# (V, n) -> seed of grid_case where seed 0 leaves a top-p target or a draw too close to a boundary (the conditions are asserted
# on the oracle alone by tests/test_truncated_sampling_cpu.py)
GRID_SEED = {(203, 1): 1, (1028, 3): 1, (12292, 3): 1}


def grid_case(V, n, seed=None):
    """8 distinct rows of V logits as n slabs (+ bias): a head of 12 (rows 6, 7: 40) words 0.3 .. 1.2 apart above a normal tail
    30 below, so that the top-p targets fall between well-separated head boundaries at every temperature of the grid while
    top-k cuts through the tail.  Rows 0 .. 3 and 6, 7 have mixed signs, rows 4 and 5 are negative throughout."""
    seed = GRID_SEED.get((V, n), 0) if seed is None else seed
    rng = np.random.default_rng([V, n, seed])
    x = rng.standard_normal((GRID_R, V)) - 30.0
    for r in range(GRID_R):
        h = min(40 if r >= 6 else 12, V // 2)
        idx = rng.choice(V, h, replace=False)
        x[r, idx] = 6.0 - np.cumsum(rng.uniform(0.3, 1.2, h))
    x[4:6] -= 50.0
    bias = rng.standard_normal(V).astype(np.float32)
    parts = [rng.standard_normal((GRID_R, V)).astype(np.float32) for _ in range(n - 1)]
    rest = x - sum(p.astype(np.float64) for p in parts) - bias[None].astype(np.float64)
    slabs = np.stack([rest.astype(np.float32)] + parts)
    return slabs, bias, slab_sum32(slabs, bias)


def is_reg(V, ld, stride=0):
    """rows the pick kernels read as float4 into registers (a 16-byte-aligned base is the caller's business)"""
    return V <= 12288 and ld % 4 == 0 and stride % 4 == 0


SPECIAL = {"reg": (1028, 1028, [5, 300, 1025, 640, 77]), "generic": (203, 205, [5, 150, 201, 64, 77])}      # V, ld, words a .. e
SPECIAL_B = 4096
SPECIAL_OPTS = [(1.0, 3, 1.0), (0.5, 3, 1.0), (1.0, 0, 0.9), (2.0, 3, 0.9)]


def special_rows(V, words):
    """Four rows of integer logits in one slab without bias (so that -0.0 arrives as it is), every other word in -9 .. -4:
    row 0: a, b at 2, c at +0.0, d at -0.0 — the third largest value is a zero, both zeros stay;
    row 1: a, b at 3, c, d, e at 2 — a tie group of three across the boundary of top_k = 3;
    row 2: row 1 minus 20, negative throughout;
    row 3: a at 20, nothing else above 0 — one word alone holds more than 0.9 of the mass at any temperature up to 2."""
    a, b, c, d, e = words
    rng = np.random.default_rng(V)
    x = rng.integers(-9, -3, size=(4, V)).astype(np.float32)
    x[0, [a, b]] = 2.0
    x[0, c], x[0, d] = 0.0, -0.0
    x[1, [a, b]] = 3.0
    x[1, [c, d, e]] = 2.0
    x[2] = x[1] - 20.0
    x[3] = np.minimum(x[3], 0.0)
    x[3, a] = 20.0
    assert np.signbit(x[0, d]) and not np.signbit(x[0, c])
    return x


CHI_CASES = [(203, 204, 3), (9490, 9490, 1)]                 # (V, ld, seed)
CHI_OPTS = (0.7, 20, 0.9)


def chi_row(V, seed):
    rng = np.random.default_rng([V, seed, 77])
    row = (rng.standard_normal(V) * 2.0).astype(np.float32)
    row[rng.integers(0, V, 5)] += 4.0
    return row


ROLLOUT_OPTS = (0.8, 5, 0.95)
