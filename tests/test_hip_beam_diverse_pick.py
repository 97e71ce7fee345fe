"""GPU: set_beam_pick_diverse_f32 (csrc/beam_constrained.hip bd_merge_k) through the direct ABI against the float64 restatement of
tests/beam_diverse_oracle.py, four consecutive steps per fixture so that state carries over: every shape x one and two models x
neutral constraints and the constrained fixtures' "all", the same logits on both row-read paths, groups = 1 against
set_beam_pick_constrained_f32, penalty = 0, and the edge scenarios.  Integer outputs equal the oracle's, floats are within TOL
of tests/beam_constrained_fixtures.py (tests/beam_diverse_fixtures.py holds what was measured here)."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_constrained_fixtures as F
import beam_constrained_oracle as BO
import beam_diverse_fixtures as D
import beam_diverse_oracle as DO

pytestmark = pytest.mark.gpu

INTS = ("k_left", "g_left", "best_seq", "best_len", "done_seq", "done_len", "done_group", "n_done")
FLOATS = ("scores", "best_score", "done_score")


def _padded(lg, ld, dev):
    """(rows, V) logits in a (rows, ld) device buffer whose padding is NaN: it must never be read as a word"""
    buf = torch.full((lg.shape[0], ld), float("nan"), device=dev)
    buf[:, :lg.shape[1]] = torch.from_numpy(lg).to(dev)
    return buf


def run_device(steps, seqs, scores, c, k, V, ld, first_len, G, penalty, entry="diverse"):
    """the steps through the C entry -> per step ({name: numpy} of the state after it, seqs_out, words, rows), as
    beam_diverse_fixtures.run_oracle returns them.  entry = "constrained": set_beam_pick_constrained_f32 (G = 1)"""
    from show_edit_tell_amd import _lib
    from show_edit_tell_amd._lib import check, ptr, stream_of
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    NI, Lmax = scores.shape[0], seqs.shape[2]
    h = DO.new_state(NI, k, G, Lmax, F.START, np.float32)
    h["seqs"], h["scores"] = seqs.copy(), scores.astype(np.float32)
    g = {n: torch.from_numpy(v).to(dev) for n, v in h.items()}
    g["seqs2"] = g["seqs"].clone()
    words = torch.full((NI * k,), -7, dtype=torch.long, device=dev)
    rows = torch.full((NI * k,), -7, dtype=torch.int32, device=dev)
    banned = torch.tensor(c.banned, dtype=torch.long, device=dev) if c.banned else None
    copts = _lib.BeamConstraintsC(c.no_repeat_ngram, c.min_len, c.length_alpha, len(c.banned), banned.data_ptr() if c.banned else None)
    ws = torch.empty(lib.set_beam_pick_diverse_workspace_bytes(NI, k), dtype=torch.uint8, device=dev)
    out = []
    for t, lg in enumerate(steps):
        bufs = [_padded(x, ld, dev) for x in lg]
        args = (ptr(bufs[0]), ptr(bufs[1]) if len(bufs) > 1 else None, ld, NI, k, V, F.END, first_len + t, Lmax, ptr(g["scores"]),
                ptr(g["k_left"]), ptr(g["seqs"]), ptr(g["seqs2"]), ptr(g["best_score"]), ptr(g["best_seq"]), ptr(g["best_len"]),
                ptr(words), ptr(rows), ptr(g["done_score"]), ptr(g["done_seq"]), ptr(g["done_len"]), ptr(g["n_done"]))
        if entry == "constrained":
            assert G == 1
            check(lib.set_beam_pick_constrained_f32(*args, C.byref(copts), ptr(ws), ws.numel(), stream_of(dev)),
                  "set_beam_pick_constrained_f32")
            g["g_left"].copy_(g["k_left"].view(NI, 1))
        else:
            check(lib.set_beam_pick_diverse_f32(*args, ptr(g["done_group"]), ptr(g["g_left"]), G, penalty, C.byref(copts), ptr(ws),
                                                ws.numel(), stream_of(dev)), "set_beam_pick_diverse_f32")
        torch.cuda.synchronize()
        g["seqs"], g["seqs2"] = g["seqs2"], g["seqs"]
        state = {n: g[n].cpu().numpy().copy() for n in INTS + FLOATS}
        out.append((state, g["seqs"].cpu().numpy().copy(), words.cpu().numpy().copy(), rows.cpu().numpy().copy()))
        g["seqs2"].copy_(g["seqs"])                                     # (both buffers hold the current sequences, as on the host)
    return out


def compare(got, ref, first_len, k, G, where):
    """integer outputs equal, floats within TOL; -> the largest float errors {name: value}"""
    err = dict.fromkeys(FLOATS, 0.0)
    g = k // G
    for t, ((gs, gseq, gw, gr), (rs, rseq, rw, rr, info)) in enumerate(zip(got, ref)):
        L = first_len + t
        for n in INTS:
            assert np.array_equal(gs[n], rs[n]), (where, t, n, gs[n], rs[n])
        assert np.array_equal(gw, rw) and np.array_equal(gr, rr), (where, t, gw, rw, gr, rr)
        for i, gi, e in DO.groups_of(info):                            # the sequences of every group that picked at this step
            if not e["exhausted"]:
                assert np.array_equal(gseq[i, gi * g:gi * g + g, :L + 1], rseq[i, gi * g:gi * g + g, :L + 1]), (where, t, i, gi)
        for n in FLOATS:
            a, b = gs[n].astype(np.float64), rs[n]
            assert np.array_equal(np.isinf(a), np.isinf(b)) and not np.isnan(a).any(), (where, t, n, a, b)
            fin = np.isfinite(b)
            if fin.any():
                err[n] = max(err[n], float(np.abs(a[fin] - b[fin]).max()))
    print(where, "max |device - oracle|", {n: "%.3g" % v for n, v in err.items()})
    for n in FLOATS:
        assert err[n] <= F.TOL, (where, n, err[n], F.TOL)
    return err


def _same_bytes(a, b, where):
    for t, (x, y) in enumerate(zip(a, b)):
        for n in INTS + FLOATS:
            assert x[0][n].tobytes() == y[0][n].tobytes(), (where, t, n)
        assert all(x[j].tobytes() == y[j].tobytes() for j in (1, 2, 3)), (where, t)


@pytest.mark.parametrize("shape,cname,models", D.DIRECT)
def test_direct_fixtures_against_the_oracle(shape, cname, models):
    V, ld, k, G, NI = D.SHAPES[shape]
    logits, seqs, scores = D.direct_inputs(shape, cname, models)
    got = run_device(logits, seqs, scores, D.CONSTRAINTS[cname], k, V, ld, D.L0, G, D.PENALTY)
    compare(got, D.direct_reference(shape, cname, models), D.L0, k, G, (shape, cname, models))


@pytest.mark.parametrize("shape", sorted(D.LAYOUT))
@pytest.mark.parametrize("models", D.MODELS)
def test_both_row_read_paths_give_identical_bytes(shape, models):
    """the "all" fixture of the shape with its own (float4) leading dimension and with ld = V (odd: scalar reads)"""
    V, ld, k, G, NI = D.SHAPES[shape]
    assert ld % 4 == 0 and V <= 12288 and D.LAYOUT[shape] % 4 != 0
    logits, seqs, scores = D.direct_inputs(shape, "all", models)
    a = run_device(logits, seqs, scores, D.CONSTRAINTS["all"], k, V, ld, D.L0, G, D.PENALTY)
    b = run_device(logits, seqs, scores, D.CONSTRAINTS["all"], k, V, D.LAYOUT[shape], D.L0, G, D.PENALTY)
    _same_bytes(a, b, (shape, models))


@pytest.mark.parametrize("shape", sorted(D.SHAPES))
@pytest.mark.parametrize("models", D.MODELS)
def test_one_group_gives_the_bytes_of_the_constrained_pick(shape, models):
    """groups = 1 on the "all" fixture's inputs (the penalty is then idle): every output of set_beam_pick_constrained_f32 byte for
    byte, done_group = 0"""
    V, ld, k, G, NI = D.SHAPES[shape]
    logits, seqs, scores = D.direct_inputs(shape, "all", models)
    a = run_device(logits, seqs, scores, D.CONSTRAINTS["all"], k, V, ld, D.L0, 1, D.PENALTY)
    b = run_device(logits, seqs, scores, D.CONSTRAINTS["all"], k, V, ld, D.L0, 1, D.PENALTY, entry="constrained")
    _same_bytes(a, b, (shape, models))
    assert not a[-1][0]["done_group"].any() and int(a[-1][0]["n_done"].sum()) > 0


@pytest.mark.parametrize("shape", sorted(D.SHAPES))
def test_without_a_penalty_every_group_repeats_group_0(shape):
    """penalty = 0 and every group given group 0's rows, histories and scores: the words and scores of group 0, step after step"""
    V, ld, k, G, NI = D.SHAPES[shape]
    g = k // G
    logits, seqs, scores = D.direct_inputs(shape, "all", 1)
    src = (np.arange(NI * k) // k) * k + np.arange(NI * k) % g            # row -> the row of group 0 with the same place in its group
    logits = [[lg[src] for lg in step] for step in logits]
    seqs, scores = seqs.reshape(NI * k, -1)[src].reshape(seqs.shape), scores.reshape(-1)[src].reshape(scores.shape)
    got = run_device(logits, seqs, scores, D.CONSTRAINTS["all"], k, V, ld, D.L0, G, 0.0)
    for t, (st, gseq, gw, gr) in enumerate(got):
        sc, w = st["scores"].reshape(NI, G, g), gw.reshape(NI, G, g)
        parent = gr.reshape(NI, G, g) - (np.arange(NI)[:, None, None] * k + np.arange(G)[None, :, None] * g)
        for gi in range(1, G):
            assert sc[:, gi].tobytes() == sc[:, 0].tobytes() and np.array_equal(w[:, gi], w[:, 0]), (shape, t, gi)
            assert np.array_equal(parent[:, gi], parent[:, 0]) and np.array_equal(st["g_left"][:, gi], st["g_left"][:, 0]), (shape, t, gi)
    assert int(got[-1][0]["n_done"].sum()) > 0


@pytest.mark.parametrize("name", sorted(D.EDGES))
def test_edge_scenarios(name):
    """an exact tie between a penalised and an unpenalised key (the lower flat index wins, both ways), the lemma's worst case
    (k = 8, G = 8, the last group takes its row's 8th candidate), a word penalised twice, <end> on top in a later group while
    earlier groups end too, one group finishing steps before the others, a group with no survivor, a finished image beside live
    ones: everything the oracle says, whose own outcome tests/test_beam_diverse_cpu.py pins"""
    NI, k, G, penalty, c, steps, seqs, scores = D.edge_inputs(name)
    got = run_device(steps, seqs, scores, c, k, D.EDGE_V, D.EDGE_LD, 1, G, penalty)
    compare(got, D.edge_reference(name), 1, k, G, name)
    if name == "early_none_finished":                                  # a finished image is left untouched, bytes and all
        for n in INTS + FLOATS:
            assert got[2][0][n][2].tobytes() == got[1][0][n][2].tobytes(), n
        assert got[2][1][2].tobytes() == got[1][1][2].tobytes()
