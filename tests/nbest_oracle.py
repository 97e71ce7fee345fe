"""Test infrastructure: oracle/beam_np.beam_loop restated so that it returns EVERY completed hypothesis — the reference's
`complete_seqs` / `complete_seqs_scores` (editnet.py:666-699, dcnet.py:450-500, eval_full.py:150-200) before it takes the max —
and whether the search ran into the step limit.  The loop body is beam_loop's line by line; only what it returns differs.
tests/test_nbest_beam_cpu.py pins it to beam_loop and to the reference's goldens; tests/test_hip_nbest_beam.py compares the HIP
searches' n-best lists with it."""
import numpy as np

from oracle import beam_np, cases, dcnet_np as DN, editnet_np as EN

# the table both n-best tests run on: fixture, fc.bias[<end>] of BOTH models as shipped / lowered by 1.0 / lowered by 1.5,
# beam sizes, all six images, three models
FIXTURE = "beam_small_e5"
SHIFTS = (0.0, -1.0, -1.5)
BEAMS = (3, 4, 5)
MODELS = ("editnet", "dcnet", "ensemble")
# (shift, k, image) cells taken out because two neighbouring n-best scores of one of the three models lie within
# beam_parity.MARGIN_MIN of each other (none at the shipped bias, at most two in all).  None had to be removed.
REMOVED = ()


def nbest_loop(states, combine, start, end, V, k, max_steps=50):
    """-> (done, limit): done = [(tokens, score, pick)] in completion order (by pick, within a pick by pick rank), limit = the
    search stopped at the step limit with hypotheses alive (beam_loop then answers seqs[0][:18], NaN; also returned)."""
    words = np.full((k,), start, np.int64)
    seqs = words[:, None]
    top = np.zeros((k, 1), np.float32)
    done = []
    step = 1
    while True:
        scores = top + combine([s.step(words) for s in states])
        flat = scores[0] if step == 1 else scores.reshape(-1)
        order = np.argsort(-flat, kind="stable")[:k]
        top_s = flat[order]
        parent, nxt = order // V, order % V
        seqs = np.concatenate([seqs[parent], nxt[:, None]], 1)
        inc = [i for i, w in enumerate(nxt) if w != end]
        comp = [i for i in range(len(nxt)) if i not in inc]
        for i in comp:
            done.append((seqs[i].tolist(), float(top_s[i]), step))
        k -= len(comp)
        if k == 0:
            return done, False, None
        seqs = seqs[inc]
        for s in states:
            s.reindex(parent[inc])
        top = top_s[inc][:, None].astype(np.float32)
        words = nxt[inc]
        if step > max_steps:
            return done, True, seqs[0][:18].tolist()
        step += 1


def ranked(done, m=None):
    """the n-best list: score descending, equal scores in completion order (a stable sort), at most m entries"""
    out = sorted(done, key=lambda e: -e[1])
    return out if m is None else out[:m]


def min_gap(done):
    sc = [e[1] for e in ranked(done)]
    return min((a - b for a, b in zip(sc, sc[1:])), default=np.inf)


COMBINE = {
    "single": lambda ls: EN._log_softmax(ls[0], 1),
    "ensemble": lambda ls: np.log((EN._softmax(ls[0], 1) + EN._softmax(ls[1], 1)) / 2),
}


def search(model, Pe, Pd, X1, prev1, plen1, start, end, k):
    """the three existing combiners on beam_np.EditNetBeam / DcnetBeam (beam_np.beam_editnet / beam_dcnet / beam_ensemble)"""
    V = (Pe if model != "dcnet" else Pd)["fc.weight"].shape[0]
    if model == "editnet":
        return nbest_loop([beam_np.EditNetBeam(Pe, X1, prev1, plen1, k)], COMBINE["single"], start, end, V, k)
    if model == "dcnet":
        return nbest_loop([beam_np.DcnetBeam(Pd, prev1, plen1, k)], COMBINE["single"], start, end, V, k)
    return nbest_loop([beam_np.EditNetBeam(Pe, X1, prev1, plen1, k), beam_np.DcnetBeam(Pd, prev1, plen1, k)], COMBINE["ensemble"],
                      start, end, V, k)


def shifted(d, shift):
    """both models' weights with fc.bias[<end>] moved by `shift` (float32 arithmetic)"""
    end = d["wm"]["<end>"]
    out = []
    for key in ("sd_e", "sd_d"):
        sd = {n: v.copy() for n, v in d[key].items()}
        sd["fc.bias"][end] = sd["fc.bias"][end] + np.float32(shift)
        out.append(sd)
    return out


_table = {}


def table():
    """{(shift, k, image, model): (done, limit, limit_answer)} of the whole table, computed once per process"""
    if _table:
        return _table
    d = cases.build_beam(FIXTURE)
    wm, B = d["wm"], d["case"]["B"]
    for shift in SHIFTS:
        sd_e, sd_d = shifted(d, shift)
        Pe, Pd = EN.cast_params(sd_e), DN.cast_params(sd_d)
        for k in BEAMS:
            for b in range(B):
                if (shift, k, b) in REMOVED:
                    continue
                for model in MODELS:
                    _table[(shift, k, b, model)] = search(model, Pe, Pd, d["X"][b:b + 1], d["prev"][b:b + 1], d["plen"][b:b + 1],
                                                          wm["<start>"], wm["<end>"], k)
    return _table
