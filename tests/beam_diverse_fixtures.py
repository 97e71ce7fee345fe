"""Fixtures shared by tests/test_beam_diverse_cpu.py, tests/test_hip_beam_diverse_pick.py and tests/test_hip_beam_diverse_search.py:
shapes, seeds, penalties and edge scenarios of the diverse beam-search pick (include/set_hip.h set_beam_pick_diverse_f32).  The
logits, the histories, the tolerance of the floats (TOL), the near-tie gap (GAP) and the margin of the fixtures (MARGIN) are
tests/beam_constrained_fixtures.py's: the carried values come from the same row kernel that tolerance was measured on."""
import functools

import numpy as np

import beam_constrained_fixtures as F
import beam_constrained_oracle as BO
import beam_diverse_oracle as DO

START, END, STEPS, L0, LMAX = F.START, F.END, F.STEPS, F.L0, F.LMAX

# MEASURED on an MI355X: max |device - float64 oracle| of scores, best_score and done_score over every step of every DIRECT fixture
# below (tests/test_hip_beam_diverse_pick.py prints them), recorded rounded up.  All below F.TOL = 6.4e-6, the bound the tests use
SCORES_MEASURED = 1.5e-6               # measured 1.40e-6
BEST_MEASURED = 6.1e-7                 # measured 6.09e-7
DONE_MEASURED = 1.7e-6                 # measured 1.61e-6
assert max(SCORES_MEASURED, BEST_MEASURED, DONE_MEASURED) < F.TOL

# shape -> (V, ld, k, G, NI): both row-read paths (float4 for ld % 4 == 0 and V <= 12288, scalar otherwise), the row tails,
# g = 1 and the largest g
SHAPES = {
    "v255":       (255, 256, 4, 2, 3),
    "v1027_g2":   (1027, 1027, 8, 4, 1),
    "v1027_g1":   (1027, 1027, 8, 8, 1),
    "v4099":      (4099, 4100, 6, 3, 3),
    "v12289_sc":  (12289, 12292, 8, 2, 2),
}
CONSTRAINTS = {"neutral": BO.NEUTRAL, "all": F.CONSTRAINTS["all"]}
MODELS = (1, 2)
PENALTY = 0.75                        # of the order of the gaps between the rows' leading words: it flips picks, it does not forbid
# (shape, constraint, models) -> seed: the smallest seed >= 1, found on the oracle alone, whose four steps keep adjacent keys among
# every group's g + 1 best and every two rank scores of an image 0.002 apart (>= F.MARGIN), in which the penalty changes a pick
# against penalty = 0 and in which a hypothesis completes (tests/test_beam_diverse_cpu.py asserts all of it)
SEEDS = {
    ('v1027_g1', 'all', 1): 2,
    ('v1027_g1', 'all', 2): 1,
    ('v1027_g1', 'neutral', 1): 1,
    ('v1027_g1', 'neutral', 2): 1,
    ('v1027_g2', 'all', 1): 1,
    ('v1027_g2', 'all', 2): 1,
    ('v1027_g2', 'neutral', 1): 1,
    ('v1027_g2', 'neutral', 2): 2,
    ('v12289_sc', 'all', 1): 3,
    ('v12289_sc', 'all', 2): 2,
    ('v12289_sc', 'neutral', 1): 1,
    ('v12289_sc', 'neutral', 2): 1,
    ('v255', 'all', 1): 2,
    ('v255', 'all', 2): 3,
    ('v255', 'neutral', 1): 1,
    ('v255', 'neutral', 2): 1,
    ('v4099', 'all', 1): 1,
    ('v4099', 'all', 2): 1,
    ('v4099', 'neutral', 1): 1,
    ('v4099', 'neutral', 2): 1,
}
DIRECT = sorted((s, c, m) for s in SHAPES for c in CONSTRAINTS for m in MODELS)
LAYOUT = {"v255": 255, "v4099": 4099}          # the same logits on the other row-read path: shape -> its leading dimension


def direct_inputs(shape, cname, models, seed=None):
    """-> (per step the list of `models` (NI * k, V) logits, seqs, scores): every slot alive, as in the middle of a search"""
    V, _, k, G, NI = SHAPES[shape]
    tag = "diverse/" + F.case_tag(shape, cname, models, SEEDS[(shape, cname, models)] if seed is None else seed)
    seqs, scores = F.histories(tag, NI, k)
    return [[F.step_logits(tag + "/m%d" % m, t, V, NI * k) for m in range(models)] for t in range(STEPS)], seqs, scores


def start_state(seqs, scores, k, G):
    NI = scores.shape[0]
    st = DO.new_state(NI, k, G, seqs.shape[2], START)
    st["seqs"], st["scores"] = seqs.copy(), scores.astype(np.float64)             # (g_left = g, k_left = k)
    return st


def run_oracle(logits, seqs, scores, c, k, V, first_len, G, penalty, rows_only=False):
    """the oracle over consecutive steps -> per step (a copy of the state after it, seqs_out, words, rows, info)"""
    st = start_state(seqs, scores, k, G)
    out = []
    for t, lg in enumerate(logits):
        so, words, rows, info = DO.pick(lg[0], lg[1] if len(lg) > 1 else None, st, first_len + t, c, k, V, END, G, penalty, rows_only)
        st["seqs"] = so
        out.append(({n: v.copy() for n, v in st.items()}, so.copy(), words, rows, info))
    return out


@functools.lru_cache(maxsize=None)
def direct_reference(shape, cname, models, seed=None, penalty=PENALTY):
    """computed once per process and shared; callers must not change it"""
    V, _, k, G, NI = SHAPES[shape]
    logits, seqs, scores = direct_inputs(shape, cname, models, seed)
    return run_oracle(logits, seqs, scores, CONSTRAINTS[cname], k, V, L0, G, penalty)


def rank_gap(st):
    return BO.rank_gap(st)


def direct_quality(shape, cname, models, seed=None):
    """-> (smallest gap between adjacent keys among a group's g + 1 best, smallest gap between two rank scores of an image,
    the penalty changes a pick against penalty = 0, hypotheses completed)"""
    ref = direct_reference(shape, cname, models, seed)
    plain = direct_reference(shape, cname, models, seed, 0.0)
    gap = min(DO.min_gap(step[4]) for step in ref)
    live = any(not (np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])) for a, b in zip(ref, plain))
    return gap, rank_gap(ref[-1][0]), live, int(ref[-1][0]["n_done"].sum())


def find_seed(shape, cname, models, margin=0.002, limit=400):
    for seed in range(1, limit):
        gap, rgap, live, nd = direct_quality(shape, cname, models, seed)
        if gap >= margin and rgap >= margin and live and nd > 0:
            return seed
    raise LookupError((shape, cname, models))


# ---- edge scenarios: V = 255, ld = 256, from the first step of a search (cur_len 1, the first slot of every group alive) ------
EDGE_V, EDGE_LD, EDGE_LMAX = F.EDGE_V, F.EDGE_LD, F.EDGE_LMAX


def _rows(n, spec):
    """n rows; spec: {row: {word: probability}} — log-probabilities of a distribution, every other word -inf"""
    lg = np.full((n, EDGE_V), -np.inf, np.float32)
    for r, words in spec.items():
        for w, p in words.items():
            lg[r, w] = np.float32(np.log(p))
    return lg


def edge_tie():
    """k = 2, G = 2, penalty 0.5, two images.  Group 0 takes word A (logit 8).  In group 1's row A has the logit 2.0 and B 1.5 among
    90 fillers of logit 0: log-sum-exp ~ 4.6, so 2.0 - lse and 1.5 - lse lie in one binade with lse itself a multiple of their ulp,
    both differences and (2.0 - lse) - 0.5 are exact in float32 and in float64, and the penalised key of A EQUALS the key of B
    bit for bit whatever the rounding of lse: the lower flat index wins.  Image 0: A = 20 < B = 30, the penalised word wins;
    image 1: A = 40 > B = 30, the unpenalised one"""
    lg = np.full((4, EDGE_V), -np.inf, np.float32)
    for i, a in enumerate((20, 40)):
        lg[2 * i, 100:190] = 0.0
        lg[2 * i, a] = 8.0
        lg[2 * i + 1, 100:190] = 0.0
        lg[2 * i + 1, a], lg[2 * i + 1, 30] = 2.0, 1.5
    return 2, 2, 2, 0.5, BO.NEUTRAL, [[lg]]


def edge_worst_case():
    """the lemma's worst case: k = 8, G = 8, penalty 1e4, every row the same eight words 10 .. 17 with falling probability and
    nothing else finite: group gi must take word 10 + gi, its row's (gi + 1)-th candidate, the last group its 8th"""
    p = [0.30, 0.22, 0.16, 0.11, 0.08, 0.06, 0.04, 0.03]
    return 1, 8, 8, 1e4, BO.NEUTRAL, [[_rows(8, {j: {10 + q: p[q] for q in range(8)} for j in range(8)})]]


def edge_twice():
    """k = 3, G = 3, penalty 0.4.  Groups 0 and 1 both take word 10 (group 1: 0.7 against 0.2, the penalty does not flip it).
    Group 2 offers 10 at 0.5 and 11 at 0.3: one penalty (log 0.5 - 0.4 > log 0.3) would keep 10, two (log 0.5 - 0.8 < log 0.3)
    give 11"""
    s = _rows(3, {0: {10: 0.9, 12: 0.1}, 1: {10: 0.7, 13: 0.2, 14: 0.1}, 2: {10: 0.5, 11: 0.3, 15: 0.2}})
    return 1, 3, 3, 0.4, BO.NEUTRAL, [[s]]


def edge_end_exempt():
    """k = 4, G = 2 (g = 2), penalty 5, two steps.  Step 1: group 0 takes 20 and <end> (one completion), group 1 — whose row also
    leads with <end>, unpenalised although group 0 picked it (penalised it would lose to 21 and 25) — takes <end> and 21: both
    groups end a hypothesis at one step.
    Step 2: both groups' survivors lead with <end> again: group 0 completes first (it finishes here), then group 1; best_* is the
    first maximum in group order"""
    s1 = _rows(4, {0: {20: 0.5, END: 0.3, 22: 0.2}, 1: {22: 1.0}, 2: {END: 0.6, 21: 0.3, 25: 0.1}, 3: {22: 1.0}})
    s2 = _rows(4, {0: {END: 0.8, 23: 0.2}, 1: {23: 1.0}, 2: {END: 0.7, 24: 0.3}, 3: {24: 1.0}})
    return 1, 4, 2, 5.0, BO.NEUTRAL, [[s1], [s2]]


def edge_early_none_finished():
    """k = 4, G = 2, penalty 0.3, word 5 banned, three images, three steps.  Image 0: group 0 completes both of its hypotheses by
    step 2 and is an ended group beside the live group 1 at step 3 (one group finishing steps before the others).  Image 1:
    group 1 offers only the banned word at step 2: no survivor, it ends with g_left = 0 while group 0 goes on.  Image 2: every
    group completes at steps 1 and 2: a finished image beside live ones at step 3"""
    steps = []
    for t in range(3):
        lg = np.full((12, EDGE_V), -np.inf, np.float32)
        live = F.step_logits("diverse_edge_live", t, EDGE_V, 12)
        live[:, END] = -np.inf
        # image 0
        lg[0:2] = (_rows(2, {0: {END: 0.5, 21: 0.3, 22: 0.2}, 1: {22: 1.0}}), _rows(2, {0: {END: 0.9, 23: 0.1}, 1: {23: 1.0}}), live[0:2])[t]
        lg[2:4] = live[2:4]
        # image 1
        lg[4:6] = live[4:6]
        lg[6:8] = _rows(2, {j: {5: 1.0} for j in range(2)}) if t == 1 else live[6:8]
        # image 2
        if t == 0:
            lg[8:12] = _rows(4, {0: {END: 0.5, 21: 0.3, 22: 0.2}, 1: {22: 1.0}, 2: {END: 0.45, 24: 0.35, 25: 0.2}, 3: {22: 1.0}})
        else:
            lg[8:12] = _rows(4, {0: {END: 0.9, 23: 0.1}, 1: {END: 1.0}, 2: {END: 0.8, 26: 0.2}, 3: {END: 1.0}})
        steps.append([lg])
    return 3, 4, 2, 0.3, BO.Constraints(banned=(5,)), steps


EDGES = {"tie": edge_tie, "worst_case": edge_worst_case, "twice": edge_twice, "end_exempt": edge_end_exempt,
         "early_none_finished": edge_early_none_finished}


def edge_inputs(name):
    NI, k, G, penalty, c, steps = EDGES[name]()
    seqs = np.full((NI, k, EDGE_LMAX), START, np.int64)
    scores = np.full((NI, k), -np.inf, np.float32)
    scores[:, ::k // G] = 0.0
    return NI, k, G, penalty, c, steps, seqs, scores


@functools.lru_cache(maxsize=None)
def edge_reference(name, penalty=None):
    NI, k, G, pen, c, steps, seqs, scores = edge_inputs(name)
    return run_oracle(steps, seqs, scores, c, k, EDGE_V, 1, G, pen if penalty is None else penalty)


# ---- the searches of tests/test_hip_beam_diverse_search.py: the models, shift and images of F's search fixture ----------------
SEARCH_SHAPES = ((4, 2), (6, 3))               # (k, G)
SEARCH_PENALTY = 0.5
SEARCH_BIG_PENALTY = 1e4
SEARCH_MAX_STEPS = F.SEARCH_MAX_STEPS


def search_constraints():
    cs = F.search_constraints()
    return {"neutral": BO.NEUTRAL, "all": cs["all"]}
