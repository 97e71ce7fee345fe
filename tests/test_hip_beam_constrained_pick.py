"""GPU: set_beam_pick_constrained_f32 (csrc/beam_constrained.hip) through the direct ABI against the float64 restatement of
tests/beam_constrained_oracle.py, consecutive steps per fixture so that state carries over: every shape x one and two models x
each constraint alone and all together, the same logits on both row-read paths, the edge scenarios, and neutral constraints
against set_beam_pick_nbest_f32.  Integer outputs equal the oracle's, floats are within TOL (tests/beam_constrained_fixtures.py,
which also holds what was measured)."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_constrained_fixtures as F
import beam_constrained_oracle as BO

pytestmark = pytest.mark.gpu

INTS = ("k_left", "best_seq", "best_len", "done_seq", "done_len", "n_done")
FLOATS = ("scores", "best_score", "done_score")


def _padded(lg, ld, dev):
    """(rows, V) logits in a (rows, ld) device buffer whose padding is NaN: it must never be read as a word"""
    buf = torch.full((lg.shape[0], ld), float("nan"), device=dev)
    buf[:, :lg.shape[1]] = torch.from_numpy(lg).to(dev)
    return buf


def run_device(steps, seqs, scores, c, k, V, ld, first_len, entry="constrained"):
    """the steps through the C entry -> per step ({name: numpy} of the state after it, seqs_out, words, rows), as
    beam_constrained_fixtures.run_oracle returns them.  entry = "nbest": set_beam_pick_nbest_f32 on the same arguments"""
    from show_edit_tell_amd import _lib
    from show_edit_tell_amd._lib import check, ptr, stream_of
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    NI, Lmax = scores.shape[0], seqs.shape[2]
    h = BO.new_state(NI, k, Lmax, F.START, np.float32)
    h["seqs"], h["scores"] = seqs.copy(), scores.astype(np.float32)
    g = {n: torch.from_numpy(v).to(dev) for n, v in h.items()}
    g["seqs2"] = g["seqs"].clone()
    words = torch.full((NI * k,), -7, dtype=torch.long, device=dev)
    rows = torch.full((NI * k,), -7, dtype=torch.int32, device=dev)
    banned = torch.tensor(c.banned, dtype=torch.long, device=dev) if c.banned else None
    copts = _lib.BeamConstraintsC(c.no_repeat_ngram, c.min_len, c.length_alpha, len(c.banned), banned.data_ptr() if c.banned else None)
    ws = torch.empty(lib.set_beam_pick_constrained_workspace_bytes(NI, k), dtype=torch.uint8, device=dev)
    out = []
    for t, lg in enumerate(steps):
        bufs = [_padded(x, ld, dev) for x in lg]
        args = (ptr(bufs[0]), ptr(bufs[1]) if len(bufs) > 1 else None, ld, NI, k, V, F.END, first_len + t, Lmax, ptr(g["scores"]),
                ptr(g["k_left"]), ptr(g["seqs"]), ptr(g["seqs2"]), ptr(g["best_score"]), ptr(g["best_seq"]), ptr(g["best_len"]),
                ptr(words), ptr(rows), ptr(g["done_score"]), ptr(g["done_seq"]), ptr(g["done_len"]), ptr(g["n_done"]))
        if entry == "nbest":
            check(lib.set_beam_pick_nbest_f32(*args, stream_of(dev)), "set_beam_pick_nbest_f32")
        else:
            check(lib.set_beam_pick_constrained_f32(*args, C.byref(copts), ptr(ws), ws.numel(), stream_of(dev)),
                  "set_beam_pick_constrained_f32")
        torch.cuda.synchronize()
        g["seqs"], g["seqs2"] = g["seqs2"], g["seqs"]
        state = {n: g[n].cpu().numpy().copy() for n in INTS + FLOATS}
        out.append((state, g["seqs"].cpu().numpy().copy(), words.cpu().numpy().copy(), rows.cpu().numpy().copy()))
        g["seqs2"].copy_(g["seqs"])                                     # (both buffers hold the current sequences, as on the host)
    return out


def _wrote_seqs(info_i):
    """the images whose sequences the step writes: live before it and not out of candidates"""
    return info_i is not None and not info_i["exhausted"]


def compare(got, ref, first_len, where, tol=None):
    """integer outputs equal, floats within TOL; -> the largest float errors {name: value}"""
    tol = F.TOL if tol is None else tol
    err = dict.fromkeys(FLOATS, 0.0)
    for t, ((gs, gseq, gw, gr), (rs, rseq, rw, rr, info)) in enumerate(zip(got, ref)):
        L = first_len + t
        for n in INTS:
            assert np.array_equal(gs[n], rs[n]), (where, t, n, gs[n], rs[n])
        assert np.array_equal(gw, rw) and np.array_equal(gr, rr), (where, t, gw, rw, gr, rr)
        for i, inf in enumerate(info):
            if _wrote_seqs(inf):
                assert np.array_equal(gseq[i, :, :L + 1], rseq[i, :, :L + 1]), (where, t, i)
        for n in FLOATS:
            a, b = gs[n].astype(np.float64), rs[n]
            assert np.array_equal(np.isinf(a), np.isinf(b)) and not np.isnan(a).any(), (where, t, n, a, b)
            fin = np.isfinite(b)
            if fin.any():
                err[n] = max(err[n], float(np.abs(a[fin] - b[fin]).max()))
    print(where, "max |device - oracle|", {n: "%.3g" % v for n, v in err.items()})
    for n in FLOATS:
        assert err[n] <= tol, (where, n, err[n], tol)
    return err


@pytest.mark.parametrize("shape,cname,models", F.DIRECT)
def test_direct_fixtures_against_the_oracle(shape, cname, models):
    V, ld, k, NI = F.SHAPES[shape]
    logits, seqs, scores = F.direct_inputs(shape, cname, models)
    got = run_device(logits, seqs, scores, F.CONSTRAINTS[cname], k, V, ld, F.L0)
    compare(got, F.direct_reference(shape, cname, models), F.L0, (shape, cname, models))


@pytest.mark.parametrize("shape", sorted(F.LAYOUT))
@pytest.mark.parametrize("models", F.MODELS)
def test_both_row_read_paths_give_identical_bytes(shape, models):
    """the "all" fixture of the shape with its own (float4) leading dimension and with ld = V (odd: scalar reads)"""
    V, ld, k, NI = F.SHAPES[shape]
    assert ld % 4 == 0 and V <= 12288 and F.LAYOUT[shape] % 4 != 0
    logits, seqs, scores = F.direct_inputs(shape, "all", models)
    a = run_device(logits, seqs, scores, F.CONSTRAINTS["all"], k, V, ld, F.L0)
    b = run_device(logits, seqs, scores, F.CONSTRAINTS["all"], k, V, F.LAYOUT[shape], F.L0)
    for t, (x, y) in enumerate(zip(a, b)):
        for n in INTS + FLOATS:
            assert x[0][n].tobytes() == y[0][n].tobytes(), (shape, models, t, n)
        assert all(x[j].tobytes() == y[j].tobytes() for j in (1, 2, 3)), (shape, models, t)


@pytest.mark.parametrize("name", sorted(F.EDGES))
def test_edge_scenarios(name):
    """exact ties (lowest flat index, a banned winner), <end> on top while min_len forbids it, fewer than k survivors, no survivor
    (k_left = 0, best_* untouched), k_left < k, a finished image beside a live one, and alpha = 0.7 reversing two completions of
    different picks: everything the oracle says, whose own outcome tests/test_beam_constrained_cpu.py pins"""
    NI, c, steps = F.EDGES[name]()
    seqs = np.full((NI, F.EDGE_K, F.EDGE_LMAX), F.START, np.int64)
    scores = np.full((NI, F.EDGE_K), -np.inf, np.float32)
    scores[:, 0] = 0.0
    got = run_device(steps, seqs, scores, c, F.EDGE_K, F.EDGE_V, F.EDGE_LD, 1)
    compare(got, F.edge_reference(name), 1, name)
    if name == "few_none_finished":                                    # a finished image is left untouched, bytes and all
        for n in INTS + FLOATS:
            assert got[2][0][n][0].tobytes() == got[1][0][n][0].tobytes(), n
            assert got[2][0][n][1].tobytes() == got[1][0][n][1].tobytes(), n


@pytest.mark.parametrize("shape", sorted(F.SHAPES))
@pytest.mark.parametrize("models", F.MODELS)
def test_neutral_constraints_against_the_nbest_entry(shape, models):
    """the "alpha" fixture's inputs with neutral constraints and through set_beam_pick_nbest_f32: every integer output identical,
    floats within TOL of each other"""
    V, ld, k, NI = F.SHAPES[shape]
    logits, seqs, scores = F.direct_inputs(shape, "alpha", models)
    a = run_device(logits, seqs, scores, BO.NEUTRAL, k, V, ld, F.L0)
    b = run_device(logits, seqs, scores, BO.NEUTRAL, k, V, ld, F.L0, entry="nbest")
    for t, (x, y) in enumerate(zip(a, b)):
        live = (a[t - 1][0]["k_left"] if t else np.full(NI, k)) > 0         # (a finished image's sequences are not copied)
        for n in INTS:
            assert np.array_equal(x[0][n], y[0][n]), (shape, models, t, n)
        assert np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]), (shape, models, t)
        assert np.array_equal(x[1][live, :, :F.L0 + t + 1], y[1][live, :, :F.L0 + t + 1]), (shape, models, t)
        for n in FLOATS:
            assert np.array_equal(np.isinf(x[0][n]), np.isinf(y[0][n]))
            fin = np.isfinite(x[0][n])
            assert (np.abs(x[0][n][fin].astype(np.float64) - y[0][n][fin]) <= F.TOL).all(), (shape, models, t, n)
