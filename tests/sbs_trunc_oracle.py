"""Float64 restatement of the TRUNCATED stochastic beam search pick (include/set_hip.h set_sbs_pick_opts_f32 /
set_sbs_pick_ensemble_opts_f32): tests/trunc_sample_oracle.kept_set composed with tests/sbs_oracle.py, both imported unchanged.
Test infrastructure: only tests/ import this module.

One model: the kept set is taken on y = fl32(x * inv_t) of every live unfinished row, words outside it become -inf and the
oracle's pick does the rest (its log-sum-exp then runs over the kept set).  Ensemble: L = log(0.5 (softmax(y_e) + softmax(y_d)))
as tests/sbs_ensemble_fixtures.mean_logp forms it, the kept set on L, the mask, and the oracle renormalises (inv_t = 1)."""
import numpy as np

import gumbel_oracle as GO
import sbs_ensemble_fixtures as E
import sbs_oracle as SO
import trunc_sample_oracle as TO

NEG = -np.inf


def _cut(st, z, top_k, top_p):
    """z (k, V) float64 -> (kept (k, V) bool, dist (k,), gap (k,)) of the rows the pick reads (live, unfinished, image open); every
    other row keeps everything.  gap: the smallest kept value minus the largest finite value cut (inf when nothing finite is
    cut): what a device that forms z in float32 must resolve to take the same set."""
    k, V = z.shape
    kept, dist, gap = np.ones((k, V), bool), np.full(k, np.inf), np.full(k, np.inf)
    for j in range(k):
        if st.n_open == 0 or st.G[j] == NEG or st.fin[j] or not np.isfinite(z[j]).any():
            continue
        kj, dj = TO.kept_set(z[j:j + 1], top_k, top_p)
        kept[j], dist[j] = kj[0], dj[0]
        cut = ~kj[0] & np.isfinite(z[j])
        if cut.any():
            gap[j] = z[j][kj[0]].min() - z[j][cut].max()
    return kept, dist, gap


def masked(st, logits, inv_t, top_k, top_p):
    """one model: (logits with -inf outside the kept set of y, kept, dist, gap)"""
    lg = np.array(logits, np.float32)
    kept, dist, gap = _cut(st, GO.scaled(lg, inv_t).astype(np.float64), top_k, top_p)
    lg[~kept] = NEG
    return lg, kept, dist, gap


def pick(st, logits, img, t, seed, offset, end_idx, inv_t=1.0, top_k=0, top_p=1.0):
    """sbs_oracle.pick on the truncated rows; info also carries kept (k, V), dist (k,) and gap (k,)"""
    lg, kept, dist, gap = masked(st, logits, inv_t, top_k, top_p)
    new, info = SO.pick(st, lg, img, t, seed, offset, end_idx, inv_t)
    info.update(kept=kept, dist=dist, gap=gap)
    return new, info


def pick_ensemble(st, lg_e, lg_d, img, t, seed, offset, end_idx, temperature=1.0, top_k=0, top_p=1.0):
    """the two-model pick: the kept set on L, the oracle renormalises the masked L"""
    L = E.mean_logp(lg_e, lg_d, temperature)
    kept, dist, gap = _cut(st, L, top_k, top_p)
    L = np.where(kept, L, NEG)
    new, info = SO.pick(st, L, img, t, seed, offset, end_idx, 1.0)
    info.update(kept=kept, dist=dist, gap=gap)
    return new, info


def search(logits_of, NI, k, steps, seed, offset, end_idx, inv_t=1.0, top_k=0, top_p=1.0, temperature=None):
    """sbs_oracle.search under truncation.  logits_of(t, states) -> (NI k, V) logits of step t, or a pair of them (the ensemble:
    then `temperature` tempers each model and inv_t is not used).  Returns (states, infos[t][i])."""
    states = [SO.Image(k) for _ in range(NI)]
    infos = []
    for t in range(steps):
        lg = logits_of(t, states)
        step = []
        for i in range(NI):
            rows = slice(i * k, (i + 1) * k)
            if isinstance(lg, tuple):
                states[i], info = pick_ensemble(states[i], np.asarray(lg[0])[rows], np.asarray(lg[1])[rows], i, t, seed, offset,
                                                end_idx, 1.0 if temperature is None else temperature, top_k, top_p)
            else:
                states[i], info = pick(states[i], np.asarray(lg)[rows], i, t, seed, offset, end_idx, inv_t, top_k, top_p)
            step.append(info)
        infos.append(step)
    return states, infos


def smallest_margin(infos):
    return min([SO.margin(i) for step in infos for i in step if not i.get("noop")] or [np.inf])


def smallest_dist(infos):
    return min(float(i["dist"].min()) for step in infos for i in step)


def smallest_gap(infos):
    return min(float(i["gap"].min()) for step in infos for i in step)
