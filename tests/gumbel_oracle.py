"""Float64 restatement of the Gumbel-max draw (include/set_hip.h "Gumbel-max draw", csrc/philox.h): the noise from the Philox
words, the perturbed scores, the pick and its top-two gap.  Test infrastructure: only tests/ import this module."""
import numpy as np

from oracle import philox_np


def noise_of_words(r):
    """g = -log(-log(u)), u = (r + 1/2) 2^-32, for uint32 words r, in float64.  -log(u) is taken as -log1p(-(1 - u)) in the upper
    half, where 1 - u = (2^32 - r - 1/2) 2^-32 is exact in float64: no cancellation at either end."""
    r = np.asarray(r, dtype=np.uint64).astype(np.float64)
    lo = r < 2.0 ** 31
    E = np.empty_like(r)
    E[lo] = -np.log((r[lo] + 0.5) * 2.0 ** -32)
    E[~lo] = -np.log1p(-((2.0 ** 32 - r[~lo] - 0.5) * 2.0 ** -32))
    return -np.log(E)


def words(seed, offset, row, t, V):
    """the uint32 word behind every vocabulary word v < V of (row, t): output word v & 3 of Philox4x32-10 with
    key (seed_lo, seed_hi) and counter (row, t + 256 ((v >> 2) + 1), offset_lo, offset_hi)"""
    assert 0 <= t <= 255 and V <= (1 << 26) - 4
    nq = (V + 3) // 4
    j = np.arange(nq, dtype=np.uint64)
    ctr = np.stack([np.full_like(j, row), np.uint64(t) + np.uint64(256) * (j + np.uint64(1)),
                    np.full_like(j, offset & 0xFFFFFFFF), np.full_like(j, (offset >> 32) & 0xFFFFFFFF)], 1)
    w = philox_np.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return w.reshape(-1)[:V]


def noise(seed, offset, rows, t, V):
    """(len(rows), V) float64 noise of timestep t"""
    return np.stack([noise_of_words(words(seed, offset, int(r), t, V)) for r in rows])


def scaled(logits, inv_t=1.0):
    """y = fl32(x * inv_t): the device scales in float and rounds the product"""
    return (np.asarray(logits, np.float32) * np.float32(inv_t)).astype(np.float32)


def draw(logits, seed, offset, t, inv_t=1.0, rows=None):
    """Gumbel-max draw of every row of logits (B, V) at timestep t.  Returns (ids (B,), gap (B,), second (B,), logp (B,), lse (B,)):
    the first maximum of s = y + g, the distance of the two largest perturbed scores, the word that holds the second largest,
    and log_softmax(y)[id] / log-sum-exp of y in float64."""
    B, V = logits.shape
    rows = np.arange(B) if rows is None else np.asarray(rows)
    y = scaled(logits, inv_t).astype(np.float64)
    s = y + noise(seed, offset, rows, t, V)
    ids = s.argmax(1)                                    # numpy: the first maximum
    top = np.partition(s, V - 2, axis=1)[:, V - 2:] if V > 1 else np.stack([s[:, 0] - np.inf, s[:, 0]], 1)
    gap = top[:, 1] - top[:, 0]
    s2 = s.copy()
    s2[np.arange(B), ids] = -np.inf
    second = s2.argmax(1)
    m = y.max(1)
    lse = m + np.log(np.exp(y - m[:, None]).sum(1))
    return ids, gap, second, y[np.arange(B), ids] - lse, lse


def chi_square_pvalue(counts, p):
    """the statistic of tests/test_hip_sampling.py: observed counts against n p, words sorted by probability and merged into
    bins of expected count >= 8; returns (chi2, bins, p-value).  Its level there: p-value > 1e-4."""
    from scipy import stats
    n = counts.sum()
    order = np.argsort(-p)
    exp_sorted, obs_sorted = p[order] * n, counts[order]
    bins_e, bins_o, ce, co = [], [], 0.0, 0
    for e, o in zip(exp_sorted, obs_sorted):
        ce += e
        co += o
        if ce >= 8.0:
            bins_e.append(ce)
            bins_o.append(co)
            ce, co = 0.0, 0
    if ce > 0:
        bins_e[-1] += ce
        bins_o[-1] += co
    chi2 = float((((np.array(bins_o) - np.array(bins_e)) ** 2) / np.array(bins_e)).sum())
    return chi2, len(bins_e), float(stats.chi2.sf(chi2, len(bins_e) - 1))


SEVEN_WORDS = np.array([1.5, -0.5, 0.25, 2.0, -2.0, 0.0, 1.0], np.float32)     # the 7-word distribution of the chi-square tests
