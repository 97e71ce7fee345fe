"""Fixtures shared by tests/test_sbs_ensemble_cpu.py, tests/test_hip_sbs_ensemble_pick.py and tests/test_hip_sbs_ensemble_search.py:
the two-model stochastic beam search pick (include/set_hip.h set_sbs_pick_ensemble_f32) and the threshold of
evaluate.sample_captions_distinct*(return_threshold=True).

The float64 restatement is tests/sbs_oracle.py UNCHANGED: the ensemble's per-word log-probabilities
L = log(0.5 (softmax(y_e) + softmax(y_d))) are formed here in float64 and handed to it as "logits" with inv_t = 1; they are
normalised, so its own log-softmax is the identity (tests/test_sbs_ensemble_cpu.py, test 1).  The oracle rounds what it is given
to float32 as it rounds one model's logits: that moves a word by at most 2^-24 (|L| + ln V), below the device's own error and
part of what MEASURED records."""
import numpy as np

import gumbel_oracle as GO
import sbs_fixtures as F
import sbs_oracle as SO

OFFSET, END, STEPS = F.OFFSET, F.END, F.STEPS

# ---- tolerance and gap (the recipe of sbs_fixtures.py) -----------------------------------------------------------------
# MEASURED: max |device - float64 oracle| of G and of phi over every step of every DIRECT fixture below (tests/
# test_hip_sbs_ensemble_pick.py prints both), on an MI355X: 4.69e-6 and 1.91e-6, recorded rounded up.  TOL = 4 x the larger one (logf / log1pf / expf
# differ between boxes and compilers); a measured value above 1e-4 would mean a wrong kernel, not a wider tolerance.
G_MEASURED = 4.7e-6
PHI_MEASURED = 2.0e-6
TOL = 4.0 * max(G_MEASURED, PHI_MEASURED)
GAP = 2.0 * TOL                       # two scores each off by TOL can swap
NEAR_TIE_FRACTION = 0.02
SEPARATION = 0.01                     # what every fixture keeps between adjacent candidates, the first loser included; >= 10 GAP


def inv_t(temperature):
    return F.inv_t(temperature)


def mean_logp(lg_e, lg_d, temperature=1.0):
    """L (rows, V) float64 = log(0.5 (softmax(y_e) + softmax(y_d))), y = fl32(x * inv_t): each model tempered BEFORE the average.
    -inf where both models give -inf."""
    out = []
    for lg in (lg_e, lg_d):
        y = GO.scaled(lg, inv_t(temperature)).astype(np.float64)
        m = y.max(1, keepdims=True)
        out.append(y - (m + np.log(np.exp(y - m).sum(1, keepdims=True))))
    a, b = out
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore"):
        L = hi + np.log1p(np.exp(np.where(np.isfinite(hi), lo - hi, -np.inf))) - np.log(2.0)
    return np.where(np.isfinite(hi), L, -np.inf)


# ---- direct fixtures: name -> (V, ld, k, NI, temperature, seed); three consecutive steps each.  The seeds were chosen on the
# oracle alone by first_seed() below: the smallest seed >= 1 whose three steps keep every adjacent pair of candidates, the first
# loser included, SEPARATION apart and carry a finished slot into a later step.
DIRECT = {
    "v255_k3_ni2":     (255, 256, 3, 2, 1.0, 1),
    "v1027_k8_ni1_sc": (1027, 1027, 8, 1, 0.5, 1),
    "v4099_k5_ni3":    (4099, 4100, 5, 3, 1.0, 1),
    "v12289_k3_ni1_sc": (12289, 12292, 3, 1, 0.5, 1),
}
REGISTER_PATH = {"v255_k3_ni2": True, "v1027_k8_ni1_sc": False, "v4099_k5_ni3": True, "v12289_k3_ni1_sc": False}
# the V = 1027 logits on both row-read paths: ld = 1027 (scalar) and ld = 1028 (register)
LAYOUT = ("v1027_k8_ni1_sc", 1027, 1028)
# logits2 == logits: the picks are set_sbs_pick_f32's (the one-model margins of the same logits are checked on the CPU)
DEGENERATE = ("v255_k3_ni2", "v4099_k5_ni3")


def model_logits(name, temperature, V, rows, steps=STEPS):
    """[(lg_e, lg_d)] per step: sbs_fixtures.step_logits under two names"""
    return [(F.step_logits(name + "_e", t, V, rows, temperature), F.step_logits(name + "_d", t, V, rows, temperature))
            for t in range(steps)]


def direct_logits(name):
    V, _, k, NI, T, _ = DIRECT[name]
    return model_logits(name, T, V, NI * k)


def oracle_search(Ls, NI, k, seed, end=END):
    """sbs_oracle.search on given per-step L (inv_t = 1: they are log-probabilities already)"""
    return SO.search(lambda t, st: Ls[t], NI, k, len(Ls), seed, OFFSET, end, 1.0)


def smallest_margin(infos):
    return min(SO.margin(i) for step in infos for i in step if not i.get("noop"))


def finished_slot_carries(infos):
    """a slot that search_with_fin saw finished after one step is the parent of a live slot at the next"""
    for before, step in zip(infos, infos[1:]):
        for old, info in zip(before, step):
            if not info.get("noop") and any(w >= 0 and old["_fin"][p] for p, w in zip(info["parents"], info["words"])):
                return True
    return False


def search_with_fin(Ls, NI, k, seed, end=END):
    """oracle_search that also notes, per step and image, which output slots are finished (for finished_slot_carries)"""
    states = [SO.Image(k) for _ in range(NI)]
    infos = []
    for t, L in enumerate(Ls):
        step = []
        for i in range(NI):
            states[i], info = SO.pick(states[i], L[i * k:(i + 1) * k], i, t, seed, OFFSET, end, 1.0)
            info["_fin"] = [bool(f) and states[i].G[s] > -np.inf for s, f in enumerate(states[i].fin)]
            step.append(info)
        infos.append(step)
    return states, infos


def good_seed(Ls, NI, k, seed, end=END):
    _, infos = search_with_fin(Ls, NI, k, seed, end)
    return smallest_margin(infos) >= SEPARATION and finished_slot_carries(infos)


def first_seed(name):
    V, _, k, NI, T, _ = DIRECT[name]
    Ls = [mean_logp(e, d, T) for e, d in direct_logits(name)]
    seed = 1
    while not good_seed(Ls, NI, k, seed):
        seed += 1
    return seed


# ---- edge rows: V = 255, k = 3, one image ----------------------------------------------------------------------------------
EDGE_V, EDGE_K = F.EDGE_V, F.EDGE_K
EDGE_SEED = {"one_sided": 1, "few_words": 1}


def edge_one_sided():
    """EditNet's odd words and DCNet's even words are -inf, every fifth word (and <end>) in both: every candidate is possible in
    ONE model only (l = its log-probability there - ln 2), and a word impossible in both is never picked"""
    out = []
    for e, d in model_logits("edge_one_sided", 1.0, EDGE_V, EDGE_K):
        e[:, 1::2] = -np.inf
        d[:, 0::2] = -np.inf
        for lg in (e, d):
            lg[:, 0::5] = -np.inf
            lg[:, END] = -np.inf
        out.append((e, d))
    return out


def edge_few_words():
    """sbs_fixtures.edge_one_word for EditNet; DCNet has the same few words with other logits, and at step 1 no <end> (possible
    in one model only).  Step 0: one candidate (two dead slots); step 1: two; step 2: <end> alone; step 3: a closed image"""
    e = F.edge_one_word()
    d = [np.full((EDGE_K, EDGE_V), -np.inf, np.float32) for _ in e]
    d[0][:, 7] = -1.0
    d[1][:, 9] = 0.75
    d[2][:, END] = 0.5
    d[3][:, 11] = 1.0
    return list(zip(e, d))


# ---- the searches of tests/test_hip_sbs_ensemble_search.py: `editnet_full_b4` + `dcnet_full_b4` (the pair of
# tests/test_hip_ensemble_beam.py), sbs_fixtures.SEARCH_END_BOOST on both fc.bias, max_steps 6, EditNet's inputs for both.
# (n, NI) -> the torch.manual_seed of the call.  Chosen on the CPU by first_search_seed(): the smallest seed >= 201 / 301 for
# which the NUMPY models' own search (numpy_search below, no GPU) keeps every margin >= SEPARATION and finishes a sequence.
SEARCH_MAX_STEPS = F.SEARCH_MAX_STEPS
SEARCH_TEMPERATURE = {(3, 2): 1.0, (5, 1): 0.5}
SEARCH_SEED = {(3, 2): 201, (5, 1): 301}


def seed_of(manual_seed):
    """what rng.next_seed() returns after torch.manual_seed(manual_seed)"""
    import torch
    from show_edit_tell_amd import rng
    torch.manual_seed(manual_seed)
    return rng.next_seed()


_NP = {}


def _numpy_models(temperature):
    import dcnet_gumbel_fixtures as DF
    import gumbel_fixtures as GF
    from oracle import cases, dcnet_np as DN, editnet_np as EN
    if "d" not in _NP:
        _NP["d"] = (cases.build_editnet(GF.CASE), cases.build_dcnet(DF.CASE), GF.inputs(5))
    de, dd, inp = _NP["d"]
    end = int(de["wm"]["<end>"])

    def boosted(sd):
        sd = dict(sd)
        sd["fc.bias"] = sd["fc.bias"].copy()
        sd["fc.bias"][end] += np.float32(F.SEARCH_END_BOOST[temperature])
        return sd

    return EN.cast_params(boosted(de["sd"])), DN.cast_params(boosted(dd["sd"])), de["wm"], inp


def numpy_search(n, NI, manual_seed):
    """The numpy models' own stochastic beam search: both oracle models step on the same words, sbs_oracle.pick on L, both
    states re-indexed by the pick's rows.  Returns (states, infos)."""
    from oracle import beam_np
    T = SEARCH_TEMPERATURE[(n, NI)]
    Pe, Pd, wm, (prev, plen, X) = _numpy_models(T)
    start, end = int(wm["<start>"]), int(wm["<end>"])
    e = beam_np.EditNetBeam(Pe, X[:NI], prev[:NI], plen[:NI], n)
    d = beam_np.DcnetBeam(Pd, prev[:NI], plen[:NI], n)
    seed = seed_of(manual_seed)
    words = np.full((NI * n,), start, np.int64)
    states = [SO.Image(n) for _ in range(NI)]
    infos = []
    for t in range(SEARCH_MAX_STEPS):
        L = mean_logp(e.step(words), d.step(words), T)
        step, rows, nxt = [], [], []
        for i in range(NI):
            states[i], info = SO.pick(states[i], L[i * n:(i + 1) * n], i, t, seed, OFFSET, end, 1.0)
            step.append(info)
            rows += [i * n + r for r in info["rows"]]
            nxt += info["next_words"]
        infos.append(step)
        if all(st.n_open == 0 for st in states):
            break
        idx = np.array(rows)
        e.reindex(idx)
        d.reindex(idx)
        words = np.array(nxt, np.int64)
    return states, infos


def good_search_seed(n, NI, manual_seed):
    states, infos = numpy_search(n, NI, manual_seed)
    return smallest_margin(infos) >= SEPARATION and any(st.fin[s] for st in states for s in range(n) if st.G[s] > -np.inf)


def first_search_seed(n, NI, start):
    s = start
    while not good_search_seed(n, NI, s):
        s += 1
    return s


# ---- threshold on the table model (sbs_fixtures.table_logits): TABLE_K + 1 slots -------------------------------------------
def table_search(seed, slots):
    def logits_of(t, states):
        return np.stack([F.table_logits(tuple(states[0].toks[j])) for j in range(slots)])
    states, _ = SO.search(logits_of, 1, slots, F.TABLE_STEPS, seed, OFFSET, F.TABLE_END)
    return states[0]
