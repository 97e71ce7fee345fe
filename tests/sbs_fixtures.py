"""Fixtures shared by tests/test_sbs_cpu.py, tests/test_hip_sbs_pick.py and tests/test_hip_sbs_search.py: shapes, seeds, chosen
logits, the tolerance of phi / G and the near-tie gap of the stochastic beam search pick (include/set_hip.h set_sbs_pick_f32)."""
import numpy as np

import gumbel_fixtures as GF
from gumbel_oracle import SEVEN_WORDS

OFFSET = GF.OFFSET                    # rng.offset(rng.SITE_ROLLOUT)
END = 3                               # <end> of the chosen-logits fixtures
STEPS = 3                             # consecutive steps of every direct fixture: finished slots carry over

# ---- tolerance and gap (the issue's recipe) -------------------------------------------------------------------------
# MEASURED: max |device - float64 oracle| of G and of phi over every step of every DIRECT fixture below (tests/test_hip_sbs_pick.py
# prints both), on an MI355X: 3.33e-6 and 2.2e-6, recorded rounded up.  TOL = 4 x the larger one: the margin covers logf /
# log1pf / expf differences between boxes and compiler versions.  G_MEASURED is far below 1e-4, the project's logits tolerance.
G_MEASURED = 3.4e-6
PHI_MEASURED = 2.3e-6
TOL = 4.0 * max(G_MEASURED, PHI_MEASURED)
GAP = 2.0 * TOL                       # two scores each off by TOL can swap: a pick with oracle neighbours closer than this may be either
NEAR_TIE_FRACTION = 0.02              # cap on picks accepted that way, among all picks of a test
MARGIN = 10.0 * GAP                   # what every direct fixture keeps between adjacent candidates (tests/test_sbs_cpu.py, test 3)

# ---- direct fixtures: name -> (V, ld, k, NI, temperature, seed).  ld % 4 == 0 and V <= 12288: the register path; otherwise the
# scalar path.  The seeds were chosen on the oracle alone (the smallest seed >= 1 whose three steps keep every adjacent pair of
# candidates 0.01 apart and carry a finished slot into a later step).
DIRECT = {
    "v255_k3_ni3":      (255, 256, 3, 3, 1.0, 1),
    "v255_k1_ni1":      (255, 256, 1, 1, 0.5, 1),
    "v1027_k8_ni1":     (1027, 1028, 8, 1, 0.5, 1),
    "v1027_k3_ni3_sc":  (1027, 1027, 3, 3, 1.0, 1),
    "v4099_k3_ni1":     (4099, 4100, 3, 1, 1.0, 1),
    "v4099_k8_ni3":     (4099, 4100, 8, 3, 0.5, 2),
    "v12289_k3_ni1_sc": (12289, 12292, 3, 1, 1.0, 2),
    "v12289_k8_ni3_sc": (12289, 12289, 8, 3, 0.5, 8),
}
# the same logits on both row-read paths: (V, k, NI, temperature, seed, padded ld)
LAYOUT = {"v1027": (1027, 3, 3, 1.0, 1, 1028), "v4099": (4099, 8, 1, 0.5, 1, 4100)}


def inv_t(temperature):
    return float(np.float32(1.0) / np.float32(temperature))


def step_logits(name, t, V, rows, temperature=1.0):
    """(rows, V) chosen logits of step t (gumbel_fixtures.pick_logits' style: normal words, a few heavy ones) with <end> at about
    a quarter of each row's mass, so that slots finish at different steps"""
    rs = np.random.RandomState((7919 * sum(map(ord, name)) + 31 * t + V) % (2 ** 31))
    lg = (rs.standard_normal((rows, V)) * 2.0).astype(np.float32)
    lg[:, rs.randint(0, V, 3)] += 3.0
    y = lg.astype(np.float64) * inv_t(temperature)
    y[:, END] = -np.inf
    m = y.max(1)
    lse = m + np.log(np.exp(y - m[:, None]).sum(1))
    lg[:, END] = ((lse - 1.1) * temperature).astype(np.float32)
    return lg


def direct_logits(name):
    V, _, k, NI, T, _ = DIRECT[name]
    return [step_logits(name, t, V, NI * k, T) for t in range(STEPS)]


def layout_logits(name):
    V, k, NI, T, _, _ = LAYOUT[name]
    return [step_logits("layout_" + name, t, V, NI * k, T) for t in range(STEPS)]


# ---- edge rows: V = 255, k = 3, one image, three steps ------------------------------------------------------------------
EDGE_V, EDGE_K, EDGE_SEED = 255, 3, 1


def edge_minus_inf():
    """every second word (and <end>) is impossible in every row: they are never picked"""
    out = []
    for t in range(STEPS):
        lg = step_logits("edge_inf", t, EDGE_V, EDGE_K)
        lg[:, 0::2] = -np.inf
        lg[:, END] = -np.inf
        out.append(lg)
    return out


def edge_one_word():
    """step 0: one possible word (two dead slots follow); step 1: two possible words, one of them <end> (fewer than k finite
    candidates again, and a finished slot); step 2: <end> alone, so every slot is finished afterwards"""
    lg = [np.full((EDGE_K, EDGE_V), -np.inf, np.float32) for _ in range(STEPS + 1)]
    lg[0][:, 7] = 0.25
    lg[1][:, 9] = 1.0
    lg[1][:, END] = 0.5
    lg[2][:, END] = -2.0
    lg[3][:, 11] = 0.0                                   # a fourth step on a closed image: a no-op
    return lg


def edge_closed_and_open():
    """two images in one launch, four steps: image 0 is edge_one_word's (closed after step 2, a no-op at step 3), image 1 stays
    open on chosen logits"""
    return [np.concatenate([a, step_logits("edge_mixed", t, EDGE_V, EDGE_K)]) for t, a in enumerate(edge_one_word())]


MIXED_SEED = 1


# ---- one-launch statistics: NI images of gumbel_oracle.SEVEN_WORDS, k = 2, step 0
STAT_NI, STAT_SEED = 4000, 2024


def stat_counts(pairs):
    """counts of the 42 ordered pairs and their probabilities p_a p_b / (1 - p_a)"""
    y = SEVEN_WORDS.astype(np.float64)
    p1 = np.exp(y) / np.exp(y).sum()
    keys = [(a, b) for a in range(7) for b in range(7) if a != b]
    p = np.array([p1[a] * p1[b] / (1.0 - p1[a]) for a, b in keys])
    index = {ab: i for i, ab in enumerate(keys)}
    counts = np.zeros(len(keys), np.int64)
    for ab in pairs:
        counts[index[tuple(int(x) for x in ab)]] += 1
    return counts, p


# ---- the searches of tests/test_hip_sbs_search.py: the gumbel_fixtures models with the <end> boost
SEARCH_MAX_STEPS = 6
SEARCH_END_BOOST = {1.0: 8.0, 0.8: 8.0, 0.5: 6.0}     # fc.bias[<end>] += this, by temperature: sequences end inside 6 steps, not all at once
SEARCH_SEED = {("editnet", 3, 1): 101, ("editnet", 5, 2): 102, ("dcnet", 3, 2): 103, ("dcnet", 5, 1): 104}
SEARCH_TEMPERATURE = {("editnet", 3, 1): 1.0, ("editnet", 5, 2): 0.5, ("dcnet", 3, 2): 1.0, ("dcnet", 5, 1): 0.5}

# ---- the table "model" of the distribution test: three words + <end>, logits a fixed function of the prefix
TABLE_V, TABLE_END, TABLE_STEPS, TABLE_K, TABLE_DRAWS = 4, 3, 3, 2, 4000


def table_logits(prefix):
    h = 1.0
    for i, w in enumerate(prefix):
        h = h * 1.7 + (w + 1) * (i + 2)
    return (np.array([0.6, -0.2, 0.3, 0.0]) + 0.8 * np.sin(h + np.arange(4) * 1.3)).astype(np.float32)


def table_leaves():
    """every sequence the 3-step search can return with its log-probability: {tuple(tokens): logp}"""
    out = {}

    def walk(prefix, lp):
        y = table_logits(prefix).astype(np.float64)
        ls = y - np.log(np.exp(y).sum())
        for w in range(TABLE_V):
            seq = prefix + (w,)
            if w == TABLE_END or len(seq) == TABLE_STEPS:
                out[seq] = lp + ls[w]
            else:
                walk(seq, lp + ls[w])
    walk((), 0.0)
    return out
