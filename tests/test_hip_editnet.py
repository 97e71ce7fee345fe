"""GPU parity: the HIP EditNet path (through the C ABI) against the reference's golden vectors and
against the numpy oracle on the same seeded inputs.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

import parity
from hip_adapter import editnet_modules, to_dev
from oracle import cases, editnet_np as EN

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name", ["editnet_small", "editnet_small_end", "editnet_full_b4", "editnet_full_v9490",
                                  "editnet_full_b128"])
def test_greedy_vs_golden(name):
    d, xe, rl = editnet_modules(name)
    g = parity.load(name)
    with torch.no_grad():
        seq, logp = rl(d["wm"], to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]), True, False)
    torch.cuda.synchronize()
    namb = parity.check_greedy(_np(seq), _np(logp), g)
    print(name, "ambiguous rows:", namb)


@pytest.mark.parametrize("name", ["editnet_small", "editnet_full_b4", "editnet_full_b128"])
def test_xe_vs_golden(name):
    d, xe, rl = editnet_modules(name)
    c, g = d["case"], parity.load(name)
    with torch.no_grad():
        pred, caps_s, dl, sort_ind = xe(to_dev(d["X"]), to_dev(d["caps"]), to_dev(d["clen"]), to_dev(d["prev"]),
                                        to_dev(d["plen"]), False, 0.0)
    torch.cuda.synchronize()
    parity.check_xe(_np(pred), dl, _np(sort_ind), g, c["V"], small=c["D"] < 1024)


@pytest.mark.parametrize("name", ["editnet_small", "editnet_full_b4"])
def test_step_intermediates_vs_oracle(name):
    """Drive begin + step through the C ABI one timestep at a time and compare every intermediate
    with the numpy oracle (same tokens fed to both).  This is the chained check at B = 6 / 4; every stage on its own, against
    float64, at the row counts and dimensions where the step changes route (with and without the token table, bt < B,
    sliced and masked attention) is tests/test_hip_step_stages.py."""
    import ctypes as C
    from show_edit_tell_amd import _lib
    d, xe, rl = editnet_modules(name)
    c = d["case"]
    lib = _lib.load()
    B, T, R, D, A, F, V = c["B"], c["T"], c["R"], c["D"], c["A"], c["F"], c["V"]
    dims = xe._dims(B, T, R, 19)
    ws = xe._workspace(dims)
    w = xe._weights()
    X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"].reshape(-1))
    st = _lib.stream_of(X.device)
    _lib.check(lib.set_editnet_begin(C.byref(w), C.byref(dims), _lib.ptr(X), None, _lib.ptr(prev), _lib.ptr(plen),
                                     _lib.ptr(ws), ws.numel(), st), "begin")
    P = EN.cast_params(d["sd"])
    S = EN.SeqState(P, d["X"], d["prev"], d["plen"])
    Tm = S.H.shape[1]
    get = lambda n, shp: _np(xe.ws_tensor(dims, n, shp))
    parity.assert_close(get("H", (B, T, D))[:, :Tm], S.H, parity.STATE_TOL, "H")
    parity.assert_close(get("M", (B, T, D))[:, :Tm], S.M, parity.STATE_TOL, "M")
    parity.assert_close(get("final_hidden", (B, D)), S.final_hidden, parity.STATE_TOL, "final_hidden")
    assert np.array_equal(get("mask", (B, T))[:, :Tm], S.mask)
    assert not get("mask", (B, T))[:, Tm:].any()
    parity.assert_close(get("image_mean", (B, F)), S.image_mean, parity.STATE_TOL, "image_mean")
    parity.assert_close(get("att1", (B, R, A)), S.att1, 5e-5, "att1")
    parity.assert_close(get("att1_c", (B, T, A))[:, :Tm], S.att1_c, 5e-5, "att1_c")
    toks = cases.synth.integers(c["iseed"], "step.toks", (4, B), 0, V)
    logits = torch.empty(B, V, dtype=torch.float32, device=X.device)
    for t in range(4):
        tok = to_dev(toks[t])
        _lib.check(lib.set_editnet_step(C.byref(w), C.byref(dims), _lib.ptr(X), _lib.ptr(tok), 1, B,
                                        _lib.ptr(logits), V, _lib.ptr(ws), ws.numel(), st), "step")
        tr = []
        EN.step(S, toks[t], None, tr)
        o = tr[0]
        for k, shp in (("h1", (B, D)), ("c1", (B, D)), ("ctx_cap", None), ("alpha_c", (B, T)), ("alpha", (B, R)),
                       ("attend_img", (B, F)), ("sel", (B, D)), ("attend_cap", (B, D)), ("h2", (B, D)),
                       ("c2", (B, D))):
            if shp is None:
                continue
            got = get(k, shp)
            want = o[k]
            if k == "alpha_c":
                got = got[:, :Tm]
            parity.assert_close(got, want, 1e-4, "step %d %s" % (t, k))
        parity.assert_close(_np(logits), o["logits"], parity.LOGIT_TOL, "step %d logits" % t)


@pytest.mark.parametrize("name", ["editnet_small", "editnet_full_b4", "editnet_full_b128"])
def test_token_table_folding(name, monkeypatch):
    """The inference-time token table (folded token-only contractions) kicks in on the second call with
    unchanged weights, keeps parity with the goldens, and is dropped when a source weight changes."""
    d, xe, rl = editnet_modules(name)
    c, g = d["case"], parity.load(name)
    args = (d["wm"], to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]), True, False)
    with torch.no_grad():
        for i in range(3):
            seq, logp = rl(*args)
            assert (rl._tok_state["table"] is not None) == (i >= 1)
            parity.check_greedy(_np(seq), _np(logp), g)
        pred, caps_s, dl, sort_ind = xe(to_dev(d["X"]), to_dev(d["caps"]), to_dev(d["clen"]), to_dev(d["prev"]),
                                        to_dev(d["plen"]), False, 0.0)
        pred, caps_s, dl, sort_ind = xe(to_dev(d["X"]), to_dev(d["caps"]), to_dev(d["clen"]), to_dev(d["prev"]),
                                        to_dev(d["plen"]), False, 0.0)
        assert xe._tok_state["table"] is not None
        parity.check_xe(_np(pred), dl, _np(sort_ind), g, c["V"], small=c["D"] < 1024)
        rl.embed.embedding.weight.mul_(1.0)            # in-place update bumps the version -> table invalid
        rl(*args)
        assert rl._tok_state["table"] is None


def test_bench_path_multi_stream_token_table_vs_golden():
    """The benchmarked configuration itself against the reference's golden: B = 128, the folded token table active (built on
    the second no-grad call), 16 decodes spread over 7 HIP streams (each with its own workspace) as bench.py's timed region
    issues them — EVERY result goes through parity.check_greedy (ids bit-exact away from near-ties, log-probs within 1e-4,
    near-tie rows accounted for) against editnet_full_b128.npz."""
    d, xe, rl = editnet_modules("editnet_full_b128")
    g = parity.load("editnet_full_b128")
    args = (d["wm"], to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]), True, False)
    with torch.no_grad():
        rl(*args)
        rl(*args)                                        # the table is built here
        assert rl._tok_state["table"] is not None
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(7)]
        cur = torch.cuda.current_stream()
        for s in streams:
            s.wait_stream(cur)
        outs = []
        for i in range(16):
            with torch.cuda.stream(streams[i % 7]):
                outs.append(rl(*args))
        for s in streams:
            cur.wait_stream(s)
        torch.cuda.synchronize()
        assert rl._tok_state["table"] is not None
    namb = [parity.check_greedy(_np(seq), _np(logp), g) for seq, logp in outs]
    for seq, logp in outs[1:]:                           # and the 16 decodes are bit-identical to each other
        assert torch.equal(seq, outs[0][0]) and torch.equal(logp, outs[0][1])
    print("ambiguous rows per decode:", namb)
