"""Test helper (not a test): the numpy oracle's side of the edit-trace parity tests.  Builds a case (oracle.cases recipe, B /
iseed optionally overridden), lets the oracle decode it greedily, turns that into forced tokens with the product's own
`tokens_from_greedy`, replays them through `oracle.editnet_np.step(..., trace=[])` and lays the per-step records out in the
trace's shapes.  Everything here is computed once per case and shared by the tests that need it; nobody may write to it."""
import functools

import numpy as np

from oracle import cases, editnet_np as EN

GAP_MIN = 1e-4            # select must equal the oracle's arg-max from this top-1 / top-2 gap of alpha_c on (> 2 x STATE_TOL)


@functools.lru_cache(maxsize=None)
def build(base, B=None, iseed=None):
    """oracle.cases.build_editnet(base), or the same recipe with B / iseed overridden"""
    if B is None and iseed is None:
        return cases.build_editnet(base)
    c = dict(cases.EDITNET_CASES.get(base) or cases.ADAPTIVE_ALL[base])
    c.update({k: v for k, v in (("B", B), ("iseed", iseed)) if v is not None})
    key = "%s@B%s_i%s" % (base, B, iseed)
    table = cases.ADAPTIVE_ALL if base in cases.ADAPTIVE_ALL else cases.DP_CASES     # where build_editnet looks names up
    table[key] = c
    try:
        return cases.build_editnet(key)
    finally:
        del table[key]


def _gate(P, e, h2_prev, c2_prev):
    """CopyLSTMCellC's gate (editnet.py:265-283) recomputed from one oracle trace entry; also the adaptive memory it implies"""
    x2 = np.concatenate([e["h1"], e["attend_cap"], e["attend_img"]], 1)
    gates = EN._linear(x2, P, "copy_lstm.x2h") + EN._linear(h2_prev, P, "copy_lstm.h2h")
    i, f, g, o = np.split(gates, 4, axis=1)
    c_new = EN._sigmoid(f) * c2_prev + EN._sigmoid(i) * np.tanh(g)
    gate = EN._sigmoid(EN._linear(c_new, P, "copy_lstm.gate_cnew") + EN._linear(e["sel"], P, "copy_lstm.gate_cmem"))
    return gate, gate * e["sel"] + (1 - gate) * c_new


@functools.lru_cache(maxsize=None)
def forced(base, B=None, iseed=None, max_len=18, rows=None):
    """The oracle's record of the forced decode of its own greedy output.  rows: keep only these rows of the case (a tuple).
    Returns a dict: d (the case), tokens (list of lists), n_steps (B), S, tok (B, S + 1) zero-padded, and per step, padded to
    the trace's shapes and zeroed beyond n_steps: alpha_c (B, S, T), alpha_v (B, S, R), gate_full (B, S, D), copy_gate (B, S),
    logp (B, S), select (B, S; -1 beyond n_steps), second (B, S) the runner-up position, gap (B, S) top-1 - top-2 of alpha_c."""
    from show_edit_tell_amd import evaluate
    d = dict(build(base, B, iseed))
    if rows is not None:
        idx = list(rows)
        for k in ("prev", "plen", "X", "image_mean"):
            if k in d:
                d[k] = d[k][idx]
    adaptive = "image_mean" in d
    P = EN.cast_params(d["sd"])
    wm = d["wm"]
    X, prev, plen, mean = d["X"], d["prev"], d["plen"], d.get("image_mean")
    seq, _ = EN.greedy_decode(P, wm["<start>"], wm["<end>"], prev, plen, X, max_len=max_len, image_mean=mean, adaptive=adaptive)
    tokens = evaluate.tokens_from_greedy(seq, wm)
    n_steps = np.array([len(r) - 1 for r in tokens])
    S, nb = int(n_steps.max()), len(tokens)
    tok = np.zeros((nb, S + 1), np.int64)
    for b, r in enumerate(tokens):
        tok[b, :len(r)] = r
    T, R, D = prev.shape[1], X.shape[1], d["case"]["D"]
    st = EN.SeqState(P, X, prev, plen, mean, adaptive)
    out = dict(d=d, tokens=tokens, n_steps=n_steps, S=S, tok=tok,
               alpha_c=np.zeros((nb, S, T), np.float32), alpha_v=np.zeros((nb, S, R), np.float32),
               gate_full=np.zeros((nb, S, D), np.float32), copy_gate=np.zeros((nb, S), np.float32),
               logp=np.zeros((nb, S), np.float32), select=np.full((nb, S), -1, np.int64),
               second=np.full((nb, S), -1, np.int64), gap=np.full((nb, S), np.inf))
    mem_err = 0.0
    for t in range(S):
        h2_prev, c2_prev = st.h2.copy(), st.c2.copy()
        tr = []
        logits = EN.step(st, tok[:, t], None, tr)
        e = tr[0]
        live = t < n_steps
        gate, mem = _gate(P, e, h2_prev, c2_prev)
        mem_err = max(mem_err, float(np.abs(mem - e["c2"]).max()))
        ac = np.zeros((nb, T), np.float32)
        ac[:, :e["alpha_c"].shape[1]] = e["alpha_c"]
        av = np.zeros((nb, R), np.float32)
        av[:, :e["alpha"].shape[1]] = e["alpha"]
        order = np.argsort(-ac.astype(np.float64), axis=1, kind="stable")        # first index on ties
        top = np.take_along_axis(ac.astype(np.float64), order[:, :2], 1) if T > 1 else None
        lp = EN._log_softmax(logits, 1)[np.arange(nb), tok[:, t + 1]]
        out["alpha_c"][live, t] = ac[live]
        out["alpha_v"][live, t] = av[live]
        out["gate_full"][live, t] = gate[live]
        out["copy_gate"][live, t] = gate.astype(np.float64).mean(1)[live]
        out["logp"][live, t] = lp[live]
        out["select"][live, t] = order[live, 0]
        if top is not None:
            out["second"][live, t] = order[live, 1]
            out["gap"][live, t] = (top[:, 0] - top[:, 1])[live]
    out["mem_err"] = mem_err
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def exempt_share(o):
    """share of the recorded (row, step) pairs whose alpha_c top-1 / top-2 gap is below GAP_MIN — from the oracle alone"""
    live = o["select"] >= 0
    return float((o["gap"][live] < GAP_MIN).mean()), int(live.sum()), float(o["gap"][live].min())
