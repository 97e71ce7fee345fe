"""Fixtures shared by tests/test_sbs_trunc_cpu.py, tests/test_hip_sbs_trunc_pick.py and tests/test_hip_sbs_trunc_search.py: the
stochastic beam search pick under top-k / top-p (include/set_hip.h set_sbs_pick_opts_f32, set_sbs_pick_ensemble_opts_f32).
The float64 restatement is tests/sbs_trunc_oracle.py."""
import numpy as np

import sbs_ensemble_fixtures as E
import sbs_fixtures as F
import sbs_oracle as SO
import sbs_trunc_oracle as TS
import trunc_sample_oracle as TO

OFFSET, END, STEPS = F.OFFSET, F.END, F.STEPS

# ---- tolerance and gap (the recipe of sbs_fixtures.py) -----------------------------------------------------------------
# MEASURED: max |device - float64 oracle| of G and of phi over every step of every DIRECT and ENS_DIRECT fixture below
# (tests/test_hip_sbs_trunc_pick.py prints both), on an MI355X: 4.35e-6 and 5.36e-7, recorded rounded up.  TOL = 4 x the larger
# one; GAP = twice that.
G_MEASURED = 4.4e-6
PHI_MEASURED = 5.4e-7
TOL = 4.0 * max(G_MEASURED, PHI_MEASURED)
GAP = 2.0 * TOL                       # two scores each off by TOL can swap
SEPARATION = 0.01                     # what every fixture keeps between adjacent candidates, the first loser included; >= 10 GAP
BOUNDARY_MIN = TO.BOUNDARY_MIN        # no row's top-p target lies closer than this (fraction of the mass) to a group boundary
# the ensemble's kept set is taken on l, which the device forms in float32 (error below TOL): the smallest kept l and the largest
# l cut lie at least this far apart in every row, so that the float64 L gives the same set.  One model: y is the same float32
# number on both sides and any positive distance will do.
CUT_GAP_MIN = 1e-4

# ---- direct fixtures: name -> (V, ld, k, NI, temperature, seed, top_k, top_p); three consecutive steps each.  ld % 4 == 0 and
# V <= 12288: the register path; otherwise the scalar path.  The seeds were chosen on the oracle alone by first_seed(): the
# smallest seed >= 1 whose three steps keep every adjacent pair of candidates SEPARATION apart and every top-p target
# BOUNDARY_MIN clear of a group boundary and, for k > 1, finish a slot.  v255_k8_ni1_k2: top_k = 2 under 8 slots, dead slots.
DIRECT = {
    "v203_k3_ni3_sc_k5":   (203, 203, 3, 3, 1.0, 2, 5, 1.0),
    "v255_k1_ni1_p":       (255, 256, 1, 1, 0.5, 1, 0, 0.9),
    "v255_k3_ni3_kp":      (255, 256, 3, 3, 1.0, 3, 5, 0.9),
    "v255_k8_ni1_k2":      (255, 256, 8, 1, 1.0, 1, 2, 1.0),
    "v1023_k3_ni1_kp":     (1023, 1024, 3, 1, 1.0, 2, 5, 0.9),       # either side of 256 threads x one quad, on both paths
    "v1023_k3_ni1_sc_kp":  (1023, 1025, 3, 1, 1.0, 3, 5, 0.9),
    "v1025_k3_ni1_kp":     (1025, 1028, 3, 1, 1.0, 3, 5, 0.9),
    "v1025_k3_ni1_sc_kp":  (1025, 1026, 3, 1, 1.0, 1, 5, 0.9),
    "v1027_k8_ni1_p":      (1027, 1028, 8, 1, 0.5, 1, 0, 0.9),
    "v1027_k3_ni3_sc_kp":  (1027, 1027, 3, 3, 1.0, 2, 5, 0.9),
    "v4099_k3_ni1_k5":     (4099, 4100, 3, 1, 1.0, 2, 5, 1.0),
    "v4099_k8_ni3_p":      (4099, 4100, 8, 3, 0.5, 2, 0, 0.9),
    "v12289_k3_ni1_sc_p":  (12289, 12292, 3, 1, 1.0, 2, 0, 0.9),
    "v12289_k8_ni3_sc_kp": (12289, 12292, 8, 3, 0.5, 18, 5, 0.9),
}
# the same logits on both row-read paths: (V, k, NI, temperature, seed, padded ld, top_k, top_p)
LAYOUT = {"v1027": (1027, 3, 3, 1.0, 2, 1028, 5, 0.9), "v4099": (4099, 8, 1, 0.5, 3, 4100, 0, 0.9)}
# the ensemble: two shapes, each on both paths (ENS_LAYOUT: one set of logits on both)
ENS_DIRECT = {
    "v255_k3_ni2_kp":      (255, 256, 3, 2, 1.0, 2, 5, 0.9),
    "v255_k3_ni2_sc_p":    (255, 255, 3, 2, 0.5, 2, 0, 0.9),
    "v1027_k8_ni1_p":      (1027, 1028, 8, 1, 0.5, 1, 0, 0.9),
    "v1027_k8_ni1_sc_k5":  (1027, 1027, 8, 1, 1.0, 1, 5, 1.0),
}
ENS_LAYOUT = ("v1027_k8_ni1_p", 1027, 1028)


def is_reg(V, ld):
    return V <= 12288 and ld % 4 == 0


HEAD = 12


def step_logits(name, t, V, rows, temperature=1.0):
    """(rows, V) chosen logits of step t in the style of trunc_sample_oracle.grid_case: per row a head of HEAD words, 0.3 .. 1.2
    apart in y = x / temperature, the last word of the vocabulary the second of them (at V % 4 != 0 it sits in the ragged last quad,
    next to the padding: counts, masses, the log-sum-exp and the candidates all depend on it) and <end> the third, above a normal
    tail 30 below.  A top-p target then falls between
    well-separated head boundaries (the tail's boundaries all lie within 1e-9 of the whole mass) while top-k cuts through the
    head; sbs_fixtures.step_logits' tail of thousands of comparable words would put a boundary within 1e-4 of any target."""
    rs = np.random.RandomState((7919 * sum(map(ord, name)) + 31 * t + V) % (2 ** 31))
    y = rs.standard_normal((rows, V)) - 30.0
    for r in range(rows):
        idx = rs.choice(np.setdiff1d(np.arange(V), [END, V - 1]), HEAD, replace=False)
        idx[1], idx[2] = V - 1, END
        y[r, idx] = 6.0 - np.cumsum(rs.uniform(0.3, 1.2, HEAD))
    return (y * temperature).astype(np.float32)


def direct_logits(name):
    V, _, k, NI, T = DIRECT[name][:5]
    return [step_logits("trunc_" + name, t, V, NI * k, T) for t in range(STEPS)]


def layout_logits(name):
    V, k, NI, T = LAYOUT[name][:4]
    return [step_logits("trunc_layout_" + name, t, V, NI * k, T) for t in range(STEPS)]


def ens_logits(name):
    V, _, k, NI, T = ENS_DIRECT[name][:5]
    return [(step_logits("trunc_" + name + "_e", t, V, NI * k, T), step_logits("trunc_" + name + "_d", t, V, NI * k, T))
            for t in range(STEPS)]


def oracle_run(Ls, NI, k, T, seed, top_k, top_p, end=END):
    """sbs_trunc_oracle.search over given per-step logits (a list of arrays: one model; of pairs: the ensemble)"""
    return TS.search(lambda t, st: Ls[t], NI, k, len(Ls), seed, OFFSET, end, F.inv_t(T), top_k, top_p, temperature=T)


def good(Ls, NI, k, T, seed, top_k, top_p, end=END, finish=True):
    states, infos = oracle_run(Ls, NI, k, T, seed, top_k, top_p, end)
    ens = isinstance(Ls[0], tuple)
    return (TS.smallest_margin(infos) >= SEPARATION and TS.smallest_dist(infos) >= BOUNDARY_MIN and
            (not ens or TS.smallest_gap(infos) >= CUT_GAP_MIN) and
            (not finish or k == 1 or any(st.fin[s] and st.G[s] > -np.inf for st in states for s in range(k))))


def first_seed(Ls, NI, k, T, top_k, top_p, end=END, finish=True):
    seed = 1
    while not good(Ls, NI, k, T, seed, top_k, top_p, end, finish):
        seed += 1
    return seed


# ---- hand-built rows: trunc_sample_oracle.special_rows (integer logits, exact ties) as step 0 of one image with 8 slots, so
# that every kept word is a candidate.  name -> (row of special_rows, top_k, top_p, the words the pick must return, as a set)
SPECIAL_K = 8
SPECIAL = {
    "tie_group_across_top_k": (1, 3, 1.0, "abcde"),      # a, b at 3; c, d, e at 2: the third largest value is a tie of three
    "both_zeros":             (0, 3, 1.0, "abcd"),       # a, b at 2; c = +0.0, d = -0.0: one value group
    "one_word_over_top_p":    (3, 0, 0.9, "a"),          # a alone holds more than 0.9: one candidate, phi' = phi_j exactly
    "negative_ties":          (2, 3, 0.9, None),         # row 1 minus 20 under both options: against the oracle only
}
SPECIAL_SEED = {(p, n): (2 if n in ("tie_group_across_top_k", "negative_ties") else 1) for p in ("reg", "generic") for n in SPECIAL}


def special_logits(path, name):
    """(logits (8, V) float32: SPECIAL_K copies of the row, V, ld, the expected words or None)"""
    V, ld, words = TO.SPECIAL[path]
    row, _, _, want = SPECIAL[name]
    x = TO.special_rows(V, words)[row]
    by = dict(zip("abcde", words))
    return np.tile(x, (SPECIAL_K, 1)), V, ld, (None if want is None else sorted(by[c] for c in want))


# ---- rows with -inf words under truncation: sbs_fixtures.edge_minus_inf with both options
EDGE_OPTS = (5, 0.9)
EDGE_SEED = 1

# ---- the searches of tests/test_hip_sbs_trunc_search.py: `editnet_small` / `dcnet_small` and their pair; the <end> boost of
# tests/test_hip_sbs_search.py is not needed (nothing has to finish); (kind, n, NI) -> the torch.manual_seed of the call
SEARCH_MAX_STEPS = F.SEARCH_MAX_STEPS
SEARCH_TOP_P = 0.9
# (kind, n, NI) -> (the torch.manual_seed of the call, temperature).  The seeds were found by one scan on an MI355X (the replay's
# margins can only be known from the route's own logits, which are deterministic for the golden weights): the first seed >= 401
# whose replay keeps every adjacent pair of candidates 10 GAP apart, every top-p target BOUNDARY_MIN clear of a group boundary
# and, for the ensemble, every cut CUT_GAP_MIN wide; tests/test_hip_sbs_trunc_search.py asserts the same of the one recorded
# seed.  The small models spread their mass over most of the 203 words, so most seeds land some row within 1e-4 of a boundary;
# 120 seeds gave EditNet no clear replay at temperature 0.5, and the ones below at these temperatures.
SEARCH = {("editnet", 3, 1): (416, 1.0), ("dcnet", 5, 1): (402, 0.5), ("ensemble", 3, 2): (419, 1.0)}

# ---- the table model of sbs_fixtures.py under top-p: inclusion and importance weights on the oracle alone
TABLE_TOP_P = 0.8
TABLE_DRAWS = F.TABLE_DRAWS


def table_kept(prefix, top_p=TABLE_TOP_P):
    y = F.table_logits(prefix).astype(np.float64)
    kept, dist = TO.kept_set(y[None], 0, top_p)
    return y, kept[0], float(dist[0])


def table_leaves(top_p=TABLE_TOP_P):
    """every sequence the 3-step search of the TRUNCATED table model can return: {tuple(tokens): log q}; and the smallest
    distance of a top-p target from a group boundary over all prefixes"""
    out, dists = {}, []

    def walk(prefix, lp):
        y, kept, dist = table_kept(prefix, top_p)
        dists.append(dist)
        ls = y - np.log(np.exp(y[kept]).sum())
        for w in range(F.TABLE_V):
            if not kept[w]:
                continue
            seq = prefix + (w,)
            if w == F.TABLE_END or len(seq) == F.TABLE_STEPS:
                out[seq] = lp + ls[w]
            else:
                walk(seq, lp + ls[w])
    walk((), 0.0)
    return out, min(dists)


def table_search(seed, slots, top_p=TABLE_TOP_P):
    def logits_of(t, states):
        return np.stack([F.table_logits(tuple(states[0].toks[j])) for j in range(slots)])
    states, _ = TS.search(logits_of, 1, slots, F.TABLE_STEPS, seed, OFFSET, F.TABLE_END, 1.0, 0, top_p)
    return states[0]
