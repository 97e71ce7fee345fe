"""Fixtures shared by tests/test_gumbel_sampling_cpu.py and tests/test_hip_gumbel_sampling.py: the inputs of the persistent
Gumbel launch test (the shapes tests/test_hip_persistent_decode.py uses for the greedy launch: `editnet_full_b4` weights, random
features, ragged previous captions), the seeds, and the numpy oracle's own Gumbel rollout."""
import numpy as np

import gumbel_oracle as GO
from oracle import cases, editnet_np as EN

CASE = "editnet_full_b4"
MAX_LEN = 6
END_BOOST = {1: 7.0, 5: 5.0, 16: 7.0}  # fc.bias[<end>] += END_BOOST[B]: rows finish inside MAX_LEN at different steps, one at the first
ROWS = (1, 5, 16)
OFFSET = 7 << 40                      # rng.offset(rng.SITE_ROLLOUT)
SEEDS = {1: 31, 5: 31, 16: 31}        # one seed per row count (chosen on the oracle alone: test_gumbel_sampling_cpu.py, test 4)
TEMPERATURE = {1: 1.0, 5: 0.5, 16: 1.0}
NEAR_TIE_FRACTION = 0.02              # cap on "either word" acceptances among all (row, step) decisions of the test


def inv_t(B):
    return float(np.float32(1.0) / np.float32(TEMPERATURE[B]))


def gap_limit(B):
    """a step is "either word" below this top-two gap of the perturbed scores: the two routes' logits agree to 1e-4 (so the gap
    of y + g moves by at most 4e-4 inv_t: two words, two routes) plus four times the noise bound 1e-5"""
    return 4e-4 * inv_t(B) + 4e-5


def inputs(B):
    """(prev (B, T), plen (B, 1), X (B, R, F)) as numpy: test_hip_persistent_decode.py's random rows"""
    d = cases.build_editnet(CASE)
    T, R, F = d["prev"].shape[1], d["X"].shape[1], d["X"].shape[2]
    rs = np.random.RandomState(200 + B)
    plen = rs.randint(1, T + 1, size=(B, 1)).astype(np.int64)
    prev = rs.randint(4, 9000, size=(B, T)).astype(np.int64)
    for i in range(B):
        prev[i, plen[i, 0]:] = 0
    X = np.abs(np.random.RandomState(300 + B).randn(B, R, F)).astype(np.float32)
    return prev, plen, X


def boosted_state(d, B):
    sd = dict(d["sd"])
    sd["fc.bias"] = sd["fc.bias"].copy()
    sd["fc.bias"][int(d["wm"]["<end>"])] += np.float32(END_BOOST[B])
    return sd


def oracle_rollout(d, B):
    """The numpy model's free-running Gumbel rollout of fixture B.  Returns seq (B, MAX_LEN) and the list of (row, step, top-two
    gap) of every decision of a live row."""
    prev, plen, X = inputs(B)
    P = EN.cast_params(boosted_state(d, B))
    start, end = int(d["wm"]["<start>"]), int(d["wm"]["<end>"])
    S = EN.SeqState(P, X, prev, plen)
    it = np.full((B,), start, np.int64)
    seq = np.zeros((B, MAX_LEN), np.int64)
    unf = None
    gaps = []
    for t in range(MAX_LEN):
        logits = EN.step(S, it)
        ids, gap, _, _, _ = GO.draw(logits, SEEDS[B], OFFSET, t, inv_t(B))
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


# ---- the chosen logits of the per-step pick test (test 6)
PICK_SEED = 99


def pick_logits(V, rows):
    rs = np.random.RandomState(1000 + V + rows)
    lg = (rs.standard_normal((rows, V)) * 2.0).astype(np.float32)
    lg[:, rs.randint(0, V, 3)] += 3.0                    # a few heavy words
    return lg
