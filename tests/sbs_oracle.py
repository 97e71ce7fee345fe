"""Float64 restatement of the stochastic beam search pick (include/set_hip.h "Stochastic beam search pick", csrc/sbs.hip) and
of a whole search over given per-step logits.  The noise is tests/gumbel_oracle.py's.  Test infrastructure: only tests/ import
this module.

The restatement is the definition, not the kernel's shape: the conditioned score is formed for ALL V words of a parent and the
k largest are taken over every candidate of the image."""
import numpy as np

import gumbel_oracle as GO

NEG = -np.inf


def log1mexp(d):
    """log(1 - exp(d)) for d <= 0 (d == 0: -inf)"""
    d = np.asarray(d, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(d > -np.log(2.0), np.log(-np.expm1(d)), np.log1p(-np.exp(np.minimum(d, 0.0))))


def conditioned(G, g):
    """g~ of every word of ONE parent with perturbed score G: the children's scores g conditioned on their maximum being G.
    The first arg-max gets G exactly; -inf stays -inf."""
    g = np.asarray(g, np.float64)
    out = np.full(g.shape, NEG)
    ok = np.isfinite(g)
    if not ok.any():
        return out
    am = int(np.argmax(g))
    Z = g[am]
    with np.errstate(invalid="ignore", over="ignore"):
        u = (G - g[ok]) + log1mexp(g[ok] - Z)
        out[ok] = G - np.maximum(u, 0.0) - np.log1p(np.exp(-np.abs(u)))
    out[am] = G
    return out


class Image:
    """the k slots of one image"""

    def __init__(self, k):
        self.k = k
        self.phi = np.zeros(k)
        self.G = np.full(k, NEG)
        self.G[0] = 0.0
        self.fin = np.zeros(k, bool)
        self.toks = [[] for _ in range(k)]
        self.n_open = 1

    def copy(self):
        o = Image.__new__(Image)
        o.k, o.phi, o.G, o.fin, o.n_open = self.k, self.phi.copy(), self.G.copy(), self.fin.copy(), self.n_open
        o.toks = [list(t) for t in self.toks]
        return o


def pick(st, logits, img, t, seed, offset, end_idx, inv_t=1.0):
    """One step of image `img` (rows img k .. img k + k - 1 of the launch) on logits (k, V).  Returns (new Image, info) with
    info = dict(parents, words (the picked word of every output slot, -1 for a dead one), next_words, rows (relative to the
    image), scores (every finite candidate's g~ in pick order, for the margins), step_logp (per output slot))."""
    k = st.k
    V = logits.shape[1]
    if st.n_open == 0:
        return st.copy(), dict(parents=list(range(k)), words=[-1] * k, next_words=[0] * k, rows=list(range(k)), scores=[],
                               step_logp=[0.0] * k, noop=True)
    cands = []                                           # (g~, flat, parent, word, phi')
    for j in range(k):
        if st.G[j] == NEG:
            continue
        if st.fin[j]:
            cands.append((st.G[j], j * V + end_idx, j, end_idx, st.phi[j]))
            continue
        y = GO.scaled(logits[j], inv_t).astype(np.float64)
        m = y.max()
        lse = m + np.log(np.exp(y - m).sum())
        ph = st.phi[j] + (y - lse)
        g = ph + GO.noise(seed, offset, [img * k + j], t, V)[0]
        g[~np.isfinite(y)] = NEG
        gt = conditioned(st.G[j], g)
        for v in np.argsort(-gt, kind="stable")[:k + 1]:          # (k + 1: the margin below the k-th rank needs one more)
            if gt[v] > NEG:
                cands.append((gt[v], j * V + int(v), j, int(v), ph[v]))
    cands.sort(key=lambda c: (-c[0], c[1]))
    new = Image(k)
    new.G[:] = NEG
    new.phi[:] = NEG
    parents, words, nxt, rows, logp = [], [], [], [], []
    for s in range(k):
        if s >= len(cands):
            parents.append(s); words.append(-1); nxt.append(0); rows.append(s); logp.append(0.0)
            continue
        gt, _, p, w, ph = cands[s]
        new.G[s], new.phi[s] = gt, ph
        new.fin[s] = bool(st.fin[p]) or w == end_idx
        new.toks[s] = list(st.toks[p]) + ([] if st.fin[p] else [w])
        parents.append(p); words.append(w)
        nxt.append(0 if new.fin[s] else w)
        rows.append(s if st.fin[p] else p)
        logp.append(0.0 if st.fin[p] else ph - st.phi[p])
    new.n_open = int(sum(1 for s in range(min(k, len(cands))) if not new.fin[s]))
    return new, dict(parents=parents, words=words, next_words=nxt, rows=rows, scores=[c[0] for c in cands[:k + 1]],
                     step_logp=logp, noop=False)


def margin(info):
    """the smallest distance of two adjacent candidates among the k picks and the first loser (inf when there is one or none)"""
    s = np.asarray(info["scores"], np.float64)
    return float(np.min(s[:-1] - s[1:])) if len(s) > 1 else float("inf")


def search(logits_of, NI, k, steps, seed, offset, end_idx, inv_t=1.0):
    """The whole search of NI images.  logits_of(t, states) -> (NI k, V) logits of step t for the current slots (a recorded
    route hands back its step; a table model looks at states[i].toks[j]).  Returns (states, infos[t][i])."""
    states = [Image(k) for _ in range(NI)]
    infos = []
    for t in range(steps):
        lg = np.asarray(logits_of(t, states))
        step = []
        for i in range(NI):
            states[i], info = pick(states[i], lg[i * k:(i + 1) * k], i, t, seed, offset, end_idx, inv_t)
            step.append(info)
        infos.append(step)
    return states, infos


def results(states, end_idx, max_steps):
    """what evaluate.sample_captions_distinct returns: per image [(tokens, logp, G, finished)] of the live slots in draw order,
    tokens in the sampled rollouts' convention (<end> as 0, zero-filled to max_steps)"""
    out = []
    for st in states:
        rows = []
        for s in range(st.k):
            if st.G[s] == NEG:
                continue
            tk = [0 if w == end_idx else int(w) for w in st.toks[s]]
            rows.append((tk + [0] * (max_steps - len(tk)), float(st.phi[s]), float(st.G[s]), bool(st.fin[s])))
        out.append(rows)
    return out
