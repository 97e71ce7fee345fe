"""GPU: the n-best lists of the eight beam searches (evaluate.beam_search_*(n_best=m)) and of the four C entry points under them
(set_beam_pick_nbest_f32, set_{editnet,dcnet,ensemble}_beam_persistent_nbest) against tests/nbest_oracle.py — beam_np.beam_loop
restated so that it returns every completed hypothesis; tests/test_nbest_beam_cpu.py pins it and the table used here.

The table's fixture (beam_small_e5, D = 64) lies outside the persistent launches (D = 1024, A = 512 only: set_hip.h), so its
per-image searches take the per-step route at every k; that the persistent launch is TAKEN and did not fall back is asserted where
it exists, at beam_full_b4 / beam_adaptive_full_b4 dimensions (tests (a2), (b2), (d)), against the batched per-step search that
test (a) pins to the oracle — the way tests/test_hip_ensemble_beam.py compares its searches that run."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_parity
import nbest_oracle as NO
import pick_oracle
from hip_adapter import load_numpy_state, to_dev
from oracle import cases

pytestmark = pytest.mark.gpu


def _models(d, sds):
    from show_edit_tell_amd import dcnet, editnet
    c, dc, wm = d["case"], d["dcase"], d["wm"]
    xe = load_numpy_state(editnet.DecoderC(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), sds[0])
    dae = load_numpy_state(dcnet.DAE(wm, None, dc["D"], dc["A"], dc["C"], dc["E"]), sds[1])
    return xe, dae


def _searches(model, xe, dae):
    """(per-image search, batched search) of one model as functions of (X, prev, plen, wm, k, **kw)"""
    from show_edit_tell_amd import evaluate as ev
    if model == "editnet":
        return (lambda X, p, l, wm, k, **kw: ev.beam_search_editnet(xe, X, p, l, wm, k, **kw),
                lambda X, p, l, wm, k, **kw: ev.beam_search_editnet_batched(xe, X, p, l, wm, k, **kw))
    if model == "dcnet":
        return (lambda X, p, l, wm, k, **kw: ev.beam_search_dcnet(dae, p, l, wm, k, **kw),
                lambda X, p, l, wm, k, **kw: ev.beam_search_dcnet_batched(dae, p, l, wm, k, **kw))
    return (lambda X, p, l, wm, k, **kw: ev.beam_search_ensemble(xe, dae, X, p, l, wm, k, **kw),
            lambda X, p, l, wm, k, **kw: ev.beam_search_ensemble_batched(xe, dae, X, p, l, wm, k, **kw))


def _same_primary(a, b):
    return a[0] == b[0] and (a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1])))


def _check_vs_oracle(nbest, done, where):
    """token lists equal the oracle's IN ORDER, scores within SCORE_TOL (the CPU test asserts that no two neighbours are closer
    than MARGIN_MIN = 2 SCORE_TOL, so the order is decided)"""
    want = NO.ranked(done)
    print(where, "n-best", [(len(s), round(v, 4)) for s, v in nbest], "oracle", [(len(s), round(v, 4), p) for s, v, p in want])
    assert [s for s, _ in nbest] == [s for s, _, _ in want], (where, nbest, want)
    assert all(abs(v - w[1]) < beam_parity.SCORE_TOL for (_, v), w in zip(nbest, want)), (where, nbest, want)


# ---- (a) the table: every search with n_best = k against the oracle
@pytest.mark.parametrize("model", NO.MODELS)
@pytest.mark.parametrize("shift", NO.SHIFTS)
def test_n_best_lists_vs_the_oracle_over_the_table(shift, model):
    """Per-image entry with k = 3, 4, 5 (the per-step route at these dimensions, see the module docstring) and the batched entry on
    all six images at once: token lists in the oracle's order, scores within SCORE_TOL; the primary result is the one of the call
    without n_best; n_best = 2 is the first two entries of n_best = k."""
    d = cases.build_beam(NO.FIXTURE)
    wm, B = d["wm"], d["case"]["B"]
    t = NO.table()
    xe, dae = _models(d, NO.shifted(d, shift))
    X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])
    one_f, many_f = _searches(model, xe, dae)
    for _ in range(2):                                                   # (the token tables are built on the second call: the
        many_f(X, prev, plen, wm, 3)                                     # calls compared below all run with them)
    n = 0
    for k in NO.BEAMS:
        keep = [b for b in range(B) if (shift, k, b) not in NO.REMOVED]
        seqs, scores, lists = many_f(X, prev, plen, wm, k, return_scores=True, n_best=k)
        seqs0, scores0 = many_f(X, prev, plen, wm, k, return_scores=True)
        seqs2, lists2 = many_f(X, prev, plen, wm, k, n_best=2)
        assert seqs == seqs0 == seqs2 and all(_same_primary((0, a), (0, b_)) for a, b_ in zip(scores, scores0))
        for b in keep:
            done, limit, _ = t[(shift, k, b, model)]
            _check_vs_oracle(lists[b], done, ("batched", shift, k, b, model))
            assert lists2[b] == lists[b][:2]
            assert np.isnan(scores[b]) == limit
            if not limit:
                assert (seqs[b], scores[b]) == lists[b][0]
            one = (X[b:b + 1], prev[b:b + 1], plen[b:b + 1])
            res = one_f(*one, wm, k, n_best=k)
            assert len(res) == 3
            _check_vs_oracle(res[2], done, ("per image", shift, k, b, model))
            assert _same_primary(res, one_f(*one, wm, k))
            assert one_f(*one, wm, k, n_best=2)[2] == res[2][:2]
            if not limit:
                assert (res[0], res[1]) == res[2][0]
            n += 2
    assert n == 2 * (len(NO.BEAMS) * B - sum(1 for s, _, _ in NO.REMOVED if s == shift))


# ---- (a2) the persistent launches (full dimensions) against the batched per-step search
def _boosted_full(d, boost):
    end = d["wm"]["<end>"]
    out = []
    for key in ("sd_e", "sd_d"):
        sd = {n: v.copy() for n, v in d[key].items()}
        sd["fc.bias"][end] = sd["fc.bias"][end] - np.float32(4.0) + np.float32(boost)
        out.append(sd)
    return out


def _well_formed(nbest, k, wm):
    assert len(nbest) <= k
    assert all(s[0] == wm["<start>"] and s[-1] == wm["<end>"] and wm["<end>"] not in s[:-1] for s, _ in nbest), nbest
    assert all(a[1] >= b[1] for a, b in zip(nbest, nbest[1:])), nbest


@pytest.mark.parametrize("model", NO.MODELS)
def test_persistent_n_best_vs_the_batched_search(model):
    """beam_full_b4 with <end> boosts 2.7 / 2.8 in both models (the searches of tests/test_hip_ensemble_beam.py that run for 6 - 14
    tokens and shrink k inside the launch), k = 3 and 4, four images.  The persistent launch is taken (asserted: the private entry
    answers, it is None on a fall-back).  Finished searches whose batched n-best scores are further apart than MARGIN_MIN: the
    same token lists in the same order, scores within SCORE_TOL (counted).  The numpy oracle (tests/nbest_oracle.search at these
    dimensions, 45 s on a CPU, not run here) finishes 4 / 5 / 12 of the 16 searches of EditNet / DCNet / the ensemble, every
    neighbouring gap >= 0.33, with completions as late as picks 35, 49 and 50 (DCNet, 2.7, k = 4, image 2); the floors asked for
    (3 / 3 / 9) leave room only for a device search that tips between "finishes" and "step limit" at a near-tie pick.  Searches at the
    step limit (a chaotic 50-pick trajectory, the project compares their first tokens only): NaN on both routes, a well-formed
    list.  Always: the primary result is the call's without n_best, and entry 0 when the search finished."""
    from show_edit_tell_amd import evaluate as ev
    d = cases.build_beam("beam_full_b4")
    wm, B = d["wm"], d["case"]["B"]
    X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])
    strict = 0
    for boost in (2.7, 2.8):
        xe, dae = _models(d, _boosted_full(d, boost))
        one_f, many_f = _searches(model, xe, dae)
        private = {"editnet": lambda X_, p, l, k, **kw: ev._beam_search_editnet_persistent(xe, X_, p, l, wm, k, **kw),
                   "dcnet": lambda X_, p, l, k, **kw: ev._beam_search_dcnet_persistent(dae, p, l, wm, k, **kw),
                   "ensemble": lambda X_, p, l, k, **kw: ev._beam_search_ensemble_persistent(xe, dae, X_, p, l, wm, k, **kw)}[model]
        for k in (3, 4):
            bseqs, bscores, blists = many_f(X, prev, plen, wm, k, return_scores=True, n_best=k)
            for b in range(B):
                one = (X[b:b + 1], prev[b:b + 1], plen[b:b + 1])
                one_f(*one, wm, k)                                       # (the token tables are built on the second call)
                res = private(*one, k, n_best=k)
                assert res is not None, "the persistent launch must be taken at k <= 4 with the token tables active"
                plain = private(*one, k)
                assert plain is not None and _same_primary(res, plain), (res, plain)
                assert private(*one, k, n_best=2)[2] == res[2][:2]
                _well_formed(res[2], k, wm)
                gaps = [x[1] - y[1] for x, y in zip(blists[b], blists[b][1:])]
                print(model, boost, k, b, "persistent", [(len(s), round(v, 4)) for s, v in res[2]], "batched",
                      [(len(s), round(v, 4)) for s, v in blists[b]])
                if np.isnan(bscores[b]):
                    assert np.isnan(res[1])
                    continue
                assert not np.isnan(res[1]) and (res[0], res[1]) == res[2][0] and len(res[2]) == k
                if all(g > beam_parity.MARGIN_MIN for g in gaps):
                    assert [s for s, _ in res[2]] == [s for s, _ in blists[b]], (model, boost, k, b, res[2], blists[b])
                    assert all(abs(x[1] - y[1]) < beam_parity.SCORE_TOL for x, y in zip(res[2], blists[b]))
                    strict += 1
    print(model, "strict comparisons", strict)
    assert strict >= {"editnet": 3, "dcnet": 3, "ensemble": 9}[model], strict


# ---- (b) adaptive features: the number of completed hypotheses the reference's own loop recorded
def _adaptive_decoder(d, boost):
    from show_edit_tell_amd import editnet_adaptive
    c, wm = d["case"], d["wm"]
    sd = {k: v.copy() for k, v in d["sd"].items()}
    sd["fc.bias"][wm["<end>"]] += np.float32(boost)
    return load_numpy_state(editnet_adaptive.DecoderC(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), sd)


def test_adaptive_n_best_counts_vs_the_reference_golden():
    """beam_adaptive_small, k = 3 and 5 at both boosts, beam_search_adaptive and its batched form: len(n-best) == the golden's
    ncomplete, the searches at the step limit included; finished searches: entry 0 is the reference's answer."""
    from show_edit_tell_amd import evaluate as ev
    d = cases.build_editnet("editnet_adaptive_small")
    g = beam_parity.load("beam_adaptive_small")
    wm, B = d["wm"], d["case"]["B"]
    X, mean, prev, plen = to_dev(d["X"]), to_dev(d["image_mean"]), to_dev(d["prev"]), to_dev(d["plen"])
    n = 0
    for boost in g["boosts"]:
        dec = _adaptive_decoder(d, boost)
        for k in (3, 5):
            pre = "k%d.adaptive_e%d." % (k, int(round(float(boost) * 10)))
            seqs, scores, lists = ev.beam_search_adaptive_batched(dec, X, mean, prev, plen, wm, k, return_scores=True, n_best=k)
            for b in range(B):
                tok, sc, nb = ev.beam_search_adaptive(dec, X[b:b + 1], mean[b:b + 1], prev[b:b + 1], plen[b:b + 1], wm, k, n_best=k)
                want = int(g[pre + "ncomplete"][b])
                print(pre, b, "ncomplete", want, "batched", len(lists[b]), "per image", len(nb))
                assert len(lists[b]) == want and len(nb) == want, (pre, b, want, len(lists[b]), len(nb))
                if not bool(g[pre + "infinite"][b]):
                    assert abs(nb[0][1] - float(g[pre + "score"][b])) < beam_parity.SCORE_TOL
                    beam_parity.check_one(g, k, pre.split(".")[1], b, nb[0][0], nb[0][1])
                n += 1
    assert n == 2 * 2 * B


def test_adaptive_persistent_n_best_counts_at_full_dimensions():
    """beam_adaptive_full_b4 (R = 100, masked regions), k = 3 and 4 at both boosts: the persistent launch is taken (asserted) and
    the list has the golden's ncomplete entries for every FINISHED search (at the step limit the count depends on a chaotic
    trajectory at these dimensions: a well-formed list of at most k entries)."""
    from show_edit_tell_amd import evaluate as ev
    d = cases.build_editnet("editnet_adaptive_full_b4")
    g = beam_parity.load("beam_adaptive_full_b4")
    wm, B = d["wm"], d["case"]["B"]
    X, mean, prev, plen = to_dev(d["X"]), to_dev(d["image_mean"]), to_dev(d["prev"]), to_dev(d["plen"])
    finished = 0
    for boost in g["boosts"]:
        dec = _adaptive_decoder(d, boost)
        for k in (3, 4):
            pre = "k%d.adaptive_e%d." % (k, int(round(float(boost) * 10)))
            for b in range(B):
                one = (X[b:b + 1], prev[b:b + 1], plen[b:b + 1])
                ev.beam_search_adaptive(dec, one[0], mean[b:b + 1], one[1], one[2], wm, k)      # (token table: second call)
                res = ev._beam_search_editnet_persistent(dec, *one, wm, k, image_mean=mean[b:b + 1], n_best=k)
                assert res is not None, "the persistent launch must be taken"
                _well_formed(res[2], k, wm)
                if not bool(g[pre + "infinite"][b]):
                    assert len(res[2]) == int(g[pre + "ncomplete"][b]) and (res[0], res[1]) == res[2][0]
                    beam_parity.check_one(g, k, pre.split(".")[1], b, res[0], res[1])
                    finished += 1
    assert finished >= 8, finished


# ---- (c) set_beam_pick_nbest_f32 on made-up logits against a numpy restatement
K8, V16, END, START, LMAX = 8, 16, 15, 14, 8


def _np_pick(logits, scores, k_left, seqs, best_score, best_seq, best_len, done_score, done_seq, done_len, n_done, cur_len, flags):
    """csrc/beam.hip beam_pick_k in float32 numpy, in place (tests/pick_oracle.beam_pick at this test's sizes).  Every row's
    largest logit stands >= 32 above the others, so that its log-sum-exp IS that logit in float32 (1 + 15 e^-32 rounds to 1) and
    every candidate value is exact."""
    return pick_oracle.beam_pick(logits, scores, k_left, seqs, best_score, best_seq, best_len, done_score, done_seq, done_len,
                                 n_done, cur_len, flags, K8, V16, END)


def _made_up_logits(rng, NI, p_end):
    """(NI * 8, 16): per row one word at 0 (<end> with probability p_end[image]), every other word at -(32 + 0.5 n), n in 0 .. 5 —
    few distinct values, so equal candidates are common"""
    lg = -(32.0 + 0.5 * rng.integers(0, 6, size=(NI * K8, V16))).astype(np.float32)
    for r in range(NI * K8):
        top = END if rng.random() < p_end[r // K8] else int(rng.integers(0, 14))
        lg[r, top] = 0.0
    return lg


def test_beam_pick_nbest_on_made_up_logits():
    """NI = 3, k = 8 (BEAM_KMAX), V = 16, three consecutive picks.  The scenario (asserted on the restatement): two completions
    with equal score in one pick, recorded in pick-rank order; a pick of rank >= k_left whose word is <end>, not recorded; an
    image whose k_left reaches 0 before the last pick, for which the following call is a no-op.  Every output of every pick,
    the four done_* arrays included, equals the restatement exactly."""
    from show_edit_tell_amd import _lib
    from show_edit_tell_amd._lib import check, ptr, stream_of
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    NI, k, V = 3, K8, V16
    rng = np.random.default_rng(2)
    neg = np.float32(-np.inf)
    h = dict(scores=np.full((NI, k), neg, np.float32), k_left=np.full(NI, k, np.int32), seqs=np.full((NI, k, LMAX), START, np.int64),
             best_score=np.full(NI, neg, np.float32), best_seq=np.zeros((NI, LMAX), np.int64), best_len=np.zeros(NI, np.int32),
             done_score=np.full((NI, k), neg, np.float32), done_seq=np.zeros((NI, k, LMAX), np.int64),
             done_len=np.zeros((NI, k), np.int32), n_done=np.zeros(NI, np.int32))
    h["scores"][:, 0] = 0.0
    g = {n: torch.from_numpy(v.copy()).to(dev) for n, v in h.items()}
    g["seqs2"] = g["seqs"].clone()
    words, rows = torch.zeros(NI * k, dtype=torch.long, device=dev), torch.zeros(NI * k, dtype=torch.int32, device=dev)
    flags = dict(noop=0, uncounted_end=0, tie=0, zero=0)
    p_end = (0.35, 0.45, 0.95)
    for cur_len in (1, 2, 3):
        lg = _made_up_logits(rng, NI, p_end)
        lg_d = torch.from_numpy(lg).to(dev)
        check(lib.set_beam_pick_nbest_f32(ptr(lg_d), None, V, NI, k, V, END, cur_len, LMAX, ptr(g["scores"]), ptr(g["k_left"]),
                                          ptr(g["seqs"]), ptr(g["seqs2"]), ptr(g["best_score"]), ptr(g["best_seq"]), ptr(g["best_len"]),
                                          ptr(words), ptr(rows), ptr(g["done_score"]), ptr(g["done_seq"]), ptr(g["done_len"]),
                                          ptr(g["n_done"]), stream_of(dev)), "set_beam_pick_nbest_f32")
        torch.cuda.synchronize()
        live_before = h["k_left"].copy()
        out, w_np, r_np = _np_pick(lg, h["scores"], h["k_left"], h["seqs"], h["best_score"], h["best_seq"], h["best_len"],
                                   h["done_score"], h["done_seq"], h["done_len"], h["n_done"], cur_len, flags)
        got_out = g["seqs2"].cpu().numpy()
        for i in range(NI):
            if live_before[i] > 0:                                      # (a finished image's sequences are not copied)
                assert np.array_equal(got_out[i, :, :cur_len + 1], out[i, :, :cur_len + 1]), (cur_len, i)
                h["seqs"][i] = out[i]
        g["seqs"], g["seqs2"] = g["seqs2"], g["seqs"]
        g["seqs2"].copy_(g["seqs"])                                     # (both buffers hold the current sequences, as on the host)
        h["seqs"] = g["seqs"].cpu().numpy().copy()
        assert np.array_equal(words.cpu().numpy(), w_np) and np.array_equal(rows.cpu().numpy(), r_np), cur_len
        for name in ("scores", "k_left", "best_score", "best_seq", "best_len", "done_score", "done_seq", "done_len", "n_done"):
            assert np.array_equal(g[name].cpu().numpy(), h[name]), (cur_len, name, g[name].cpu().numpy(), h[name])
        print("pick", cur_len, "k_left", h["k_left"], "n_done", h["n_done"], flags)
    assert flags["tie"] >= 1 and flags["uncounted_end"] >= 1 and flags["zero"] >= 1 and flags["noop"] >= 1, flags
    assert (h["n_done"] + h["k_left"] == k).all()


# ---- (d) the entries without n-best produce the same bytes as the entries with it
def test_beam_pick_outputs_are_byte_identical_with_and_without_n_best():
    """set_beam_pick_f32 against set_beam_pick_nbest_f32, three consecutive picks on logits of beam_small_e5's size (6 images,
    k = 5, V = 203, random values, <end> favoured): every output array of every pick holds the same bytes."""
    from show_edit_tell_amd import _lib
    from show_edit_tell_amd._lib import check, ptr, stream_of
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    NI, k, V, Lmax, end = 6, 5, 203, 8, 202
    rng = np.random.default_rng(5)

    def state():
        s = dict(scores=torch.full((NI, k), float("-inf"), device=dev), k_left=torch.full((NI,), k, dtype=torch.int32, device=dev),
                 seqs_in=torch.full((NI, k, Lmax), 201, dtype=torch.long, device=dev),
                 seqs_out=torch.full((NI, k, Lmax), 201, dtype=torch.long, device=dev),
                 best_score=torch.full((NI,), float("-inf"), device=dev), best_seq=torch.zeros(NI, Lmax, dtype=torch.long, device=dev),
                 best_len=torch.zeros(NI, dtype=torch.int32, device=dev), words=torch.zeros(NI * k, dtype=torch.long, device=dev),
                 rows=torch.zeros(NI * k, dtype=torch.int32, device=dev))
        s["scores"][:, 0] = 0.0
        return s

    a, b = state(), state()
    extra = (torch.full((NI, k), float("-inf"), device=dev), torch.zeros(NI, k, Lmax, dtype=torch.long, device=dev),
             torch.zeros(NI, k, dtype=torch.int32, device=dev), torch.zeros(NI, dtype=torch.int32, device=dev))
    order = ("scores", "k_left", "seqs_in", "seqs_out", "best_score", "best_seq", "best_len", "words", "rows")
    for cur_len in (1, 2, 3):
        lg = rng.standard_normal((NI * k, V)).astype(np.float32) * 3
        lg[:, end] += 4.0
        lg_d = torch.from_numpy(lg).to(dev)
        head = (ptr(lg_d), None, V, NI, k, V, end, cur_len, Lmax)
        check(lib.set_beam_pick_f32(*head, *(ptr(a[n]) for n in order), stream_of(dev)), "set_beam_pick_f32")
        check(lib.set_beam_pick_nbest_f32(*head, *(ptr(b[n]) for n in order), *(ptr(x) for x in extra), stream_of(dev)),
              "set_beam_pick_nbest_f32")
        torch.cuda.synchronize()
        for n in order:
            assert torch.equal(a[n].view(torch.uint8), b[n].view(torch.uint8)), (cur_len, n)
        for s in (a, b):
            s["seqs_in"], s["seqs_out"] = s["seqs_out"], s["seqs_in"]
    assert int(extra[3].sum()) >= 3 and int(extra[3].sum()) == NI * k - int(b["k_left"].sum())


def _persistent_pair(model, xe, dae, X, prev, plen, wm, k, picks):
    """(rc, buffer bytes) of set_*_beam_persistent and of its _nbest twin on 0x5A-filled output buffers"""
    from show_edit_tell_amd import _lib, evaluate as ev
    from show_edit_tell_amd._lib import ptr, stream_of
    lib = _lib.load()
    dev = X.device
    Xk, pk, lk = X.expand(k, -1, -1).contiguous(), prev.expand(k, -1).contiguous(), plen.reshape(-1).expand(k).contiguous()
    start, end = int(wm["<start>"]), int(wm["<end>"])
    de, dd = xe._dims(k, pk.shape[1], Xk.shape[1], picks), dae._dims(k, pk.shape[1], picks)
    we, wd = xe._weights(de), dae._weights(dd)
    ws_e, ws_d = xe._workspace(de), dae._workspace(dd)
    res = []
    for nb in (False, True):
        out = ev._PersistentBeamOut(picks, dev, nb)
        out.buf.fill_(0x5A)
        tail = (start, end, picks, out.hist_parent, out.hist_word, out.best_score, out.best_word, out.result)
        if model == "editnet":
            args = (C.byref(we), C.byref(de), ptr(Xk), None, ptr(pk), ptr(lk)) + tail + (ptr(ws_e), ws_e.numel(), stream_of(dev))
            f = lib.set_editnet_beam_persistent_nbest if nb else lib.set_editnet_beam_persistent
        elif model == "dcnet":
            args = (C.byref(wd), C.byref(dd), ptr(pk), ptr(lk)) + tail + (ptr(ws_d), ws_d.numel(), stream_of(dev))
            f = lib.set_dcnet_beam_persistent_nbest if nb else lib.set_dcnet_beam_persistent
        else:
            nx = lib.set_ensemble_beam_xbuf_bytes(C.byref(de), C.byref(dd))
            xbuf = torch.empty(max(nx, 16), dtype=torch.uint8, device=dev)
            args = (C.byref(we), C.byref(de), C.byref(wd), C.byref(dd), ptr(Xk), ptr(pk), ptr(lk)) + tail + (
                ptr(ws_e), ws_e.numel(), ptr(ws_d), ws_d.numel(), ptr(xbuf), xbuf.numel(), stream_of(dev))
            f = lib.set_ensemble_beam_persistent_nbest if nb else lib.set_ensemble_beam_persistent
        rc = f(*args, out.hist_score) if nb else f(*args)
        torch.cuda.synchronize()
        res.append((rc, out.buf.cpu().numpy().copy(), out))
    return res


@pytest.mark.parametrize("model", NO.MODELS)
def test_persistent_outputs_are_byte_identical_with_and_without_n_best(model):
    """set_*_beam_persistent against set_*_beam_persistent_nbest.  beam_small_e5 (outside the launch): both answer
    SET_ERR_UNSUPPORTED and leave every output byte untouched.  beam_full_b4 with <end> boost 2.8, image 2, k = 4 (a search of 9
    tokens that shrinks k): both launch, and hist_parent, hist_word, best_score, best_word and result hold the same bytes; the
    rows of hist_score past the picks made stay untouched and the made ones hold a value or -inf."""
    from show_edit_tell_amd import evaluate as ev
    d = cases.build_beam(NO.FIXTURE)
    wm = d["wm"]
    xe, dae = _models(d, (d["sd_e"], d["sd_d"]))
    X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])
    for _ in range(2):                                                   # (token tables)
        _searches(model, xe, dae)[0](X[:1], prev[:1], plen[:1], wm, 3)
    (rc0, b0, _), (rc1, b1, _) = _persistent_pair(model, xe, dae, X[:1], prev[:1], plen[:1], wm, 3, 51)
    assert rc0 == 2 and rc1 == 2 and (b0 == 0x5A).all() and (b1 == 0x5A).all()

    d = cases.build_beam("beam_full_b4")
    wm = d["wm"]
    xe, dae = _models(d, _boosted_full(d, 2.8))
    X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])
    one = (X[2:3], prev[2:3], plen[2:3])
    for _ in range(2):
        _searches(model, xe, dae)[0](*one, wm, 4)
    (rc0, b0, o0), (rc1, b1, o1) = _persistent_pair(model, xe, dae, *one, wm, 4, 51)
    assert rc0 == 0 and rc1 == 0
    assert o0.o_hs == o1.o_hs == len(b0) and np.array_equal(b0, b1[:o1.o_hs])
    made = int(b1[o1.o_res:o1.o_res + 16].view("int32")[3])
    hs = b1[o1.o_hs:].view("float32").reshape(51, 4)
    assert 1 <= made <= 51 and (b1[o1.o_hs + made * 16:] == 0x5A).all()
    assert not np.isnan(hs[:made]).any() and (hs[:made] <= 0).all() and (hs[:made] > -np.inf).any()


# ---- (e)
def test_n_best_outside_1_to_beam_size_raises():
    from show_edit_tell_amd import evaluate as ev
    d = cases.build_beam(NO.FIXTURE)
    wm = d["wm"]
    xe, dae = _models(d, (d["sd_e"], d["sd_d"]))
    X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])
    da = cases.build_editnet("editnet_adaptive_small")
    dec = _adaptive_decoder(da, 2.5)
    Xa, mean, pa, la = to_dev(da["X"]), to_dev(da["image_mean"]), to_dev(da["prev"]), to_dev(da["plen"])
    for bad in (0, 4):
        for model in NO.MODELS:
            for f in _searches(model, xe, dae):
                with pytest.raises(ValueError):
                    f(X[:1], prev[:1], plen[:1], wm, 3, n_best=bad)
        for f in (ev.beam_search_adaptive, ev.beam_search_adaptive_batched):
            with pytest.raises(ValueError):
                f(dec, Xa[:1], mean[:1], pa[:1], la[:1], da["wm"], 3, n_best=bad)
    tok, sc, nb = ev.beam_search_editnet(xe, X[:1], prev[:1], plen[:1], wm, 3, n_best=3)       # the bounds themselves are fine
    assert len(nb) <= 3 and len(ev.beam_search_editnet(xe, X[:1], prev[:1], plen[:1], wm, 3, n_best=1)[2]) <= 1
    tok, sc, nb, tr = ev.beam_search_editnet(xe, X[:1], prev[:1], plen[:1], wm, 3, return_trace=True, n_best=3)
    assert tr.tokens.shape[0] == 1 and tr.tokens[0, :len(tok)].tolist() == tok                 # the trace stays the primary's
    if len(nb) > 1:                                                                             # (the docstring's recipe)
        tr2 = ev.edit_trace(xe, X[:1], prev[:1], plen[:1], wm, [nb[1][0]])
        assert tr2.tokens[0, :len(nb[1][0])].tolist() == nb[1][0]
