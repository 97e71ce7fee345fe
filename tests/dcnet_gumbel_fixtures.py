"""Fixtures shared by tests/test_dcnet_gumbel_cpu.py and tests/test_hip_dcnet_gumbel_persistent.py: the inputs of DCNet's
persistent Gumbel launch test (`dcnet_full_b4` weights, random ragged previous captions per case), the seeds, and the numpy
oracle's own Gumbel rollout (oracle/dcnet_np.py SeqState / step with tests/gumbel_oracle.py draw).

Cases: 1 and 4 rows take the resident kernel variant (B <= 4, T = 18 <= PDEC_TREG = 20); 5 rows — the five samples of ONE image,
all rows share a previous caption — and 8 rows the general one; "2pad" = 2 rows whose previous captions are padded with zero
columns to T = 24 (above PDEC_TREG, below PDEC_TMAX = 32; lengths unchanged): few rows on the general variant."""
import numpy as np

import gumbel_oracle as GO
from gumbel_fixtures import NEAR_TIE_FRACTION, OFFSET  # noqa: F401  (OFFSET = 7 << 40 = rng.offset(rng.SITE_ROLLOUT))
from oracle import cases, dcnet_np as DN

CASE = "dcnet_full_b4"
MAX_LEN = 6
CASES = (1, 4, 5, 8, "2pad")
ROWS = {1: 1, 4: 4, 5: 5, 8: 8, "2pad": 2}
PAD_T = 24
# fc.bias[<end>] += END_BOOST[case]: rows finish inside MAX_LEN at different steps, one at the first; one seed per case.  Both
# chosen on the oracle alone (tests/test_dcnet_gumbel_cpu.py)
END_BOOST = {1: 7.0, 4: 8.0, 5: 8.0, 8: 5.0, "2pad": 7.0}
SEEDS = {1: 1, 4: 9, 5: 73, 8: 7, "2pad": 5}
TEMPERATURE = {1: 1.0, 4: 1.0, 5: 1.0, 8: 0.5, "2pad": 1.0}


def inv_t(case):
    return float(np.float32(1.0) / np.float32(TEMPERATURE[case]))


def gap_limit(case):
    """gumbel_fixtures.gap_limit for this case's temperature: the two routes' logits agree to 1e-4 (so the gap of y + g moves by at
    most 4e-4 inv_t: two words, two routes) plus four times the noise bound 1e-5"""
    return 4e-4 * inv_t(case) + 4e-5


def inputs(case):
    """(prev (B, T), plen (B, 1)) as numpy: random ragged previous captions; the 5-row case repeats one caption five times, the
    padded case appends zero columns up to PAD_T"""
    d = cases.build_dcnet(CASE)
    T, B = d["prev"].shape[1], ROWS[case]
    n = 1 if case == 5 else B
    rs = np.random.RandomState(400 + (77 if case == "2pad" else B))
    plen = rs.randint(1, T + 1, size=(n, 1)).astype(np.int64)
    prev = rs.randint(4, 9000, size=(n, T)).astype(np.int64)
    for i in range(n):
        prev[i, plen[i, 0]:] = 0
    if case == 5:
        prev, plen = np.repeat(prev, 5, 0), np.repeat(plen, 5, 0)
    if case == "2pad":
        prev = np.concatenate([prev, np.zeros((B, PAD_T - T), np.int64)], 1)
    return np.ascontiguousarray(prev), np.ascontiguousarray(plen)


def boosted_state(d, case, boost=None):
    sd = dict(d["sd"])
    sd["fc.bias"] = sd["fc.bias"].copy()
    sd["fc.bias"][int(d["wm"]["<end>"])] += np.float32(END_BOOST[case] if boost is None else boost)
    return sd


def oracle_rollout(d, case, seed=None, boost=None):
    """The numpy model's free-running Gumbel rollout of a case.  Returns seq (B, MAX_LEN) and the list of (row, step, top-two gap
    of y + g) of every decision of a live row."""
    prev, plen = inputs(case)
    B = ROWS[case]
    seed = SEEDS[case] if seed is None else seed
    P = DN.cast_params(boosted_state(d, case, boost))
    start, end = int(d["wm"]["<start>"]), int(d["wm"]["<end>"])
    S = DN.SeqState(P, prev, plen)
    it = np.full((B,), start, np.int64)
    seq = np.zeros((B, MAX_LEN), np.int64)
    unf = None
    gaps = []
    for t in range(MAX_LEN):
        logits = DN.step(S, it)
        ids, gap, _, _, _ = GO.draw(logits, seed, OFFSET, t, inv_t(case))
        live = np.ones(B, bool) if unf is None else unf
        gaps += [(b, t, float(gap[b])) for b in range(B) if live[b]]
        it = ids.copy()
        it[it == end] = 0
        unf = (it > 0) if t == 0 else (unf & (it > 0))
        it = it * unf
        seq[:, t] = it
        if unf.sum() == 0:
            break
    return seq, gaps


def finish_steps(seq):
    """the step at which every row ended (MAX_LEN: it did not)"""
    return [int((r == 0).argmax()) if (r == 0).any() else MAX_LEN for r in seq]
