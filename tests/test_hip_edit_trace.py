"""GPU: the edit trace (include/set_hip.h set_editnet_edit_trace, evaluate.edit_trace) — per-word caption attention, selected
slot, copy gate, visual attention and forced-word log-probability of a teacher-forced decode — against the numpy oracle's
per-step record of the same forced tokens (tests/edit_trace_oracle.py: `oracle.editnet_np.step(..., trace=[])`; the gate is
recomputed there from the trace entries with the oracle's `_linear` / `_sigmoid`).

Tolerances are the project's own (tests/parity.py): STATE_TOL = 2e-5 for alpha_c, alpha_v, copy_gate and gate_full (O(1),
upstream of the logits), LOGIT_TOL = 1e-4 for logp.  `select` must equal the oracle's arg-max wherever the oracle's top-1 /
top-2 gap of alpha_c is >= 1e-4 (more than twice STATE_TOL: two weights each within tolerance cannot swap above it) and be one
of the oracle's two best positions below it; the share of such exempt (row, step) pairs is computed from the oracle alone
and asserted BEFORE the device result is looked at."""
import ctypes as C

import numpy as np
import pytest
import torch

import edit_trace_oracle as O
import parity
from hip_adapter import load_numpy_state, to_dev
from show_edit_tell_amd import _lib, evaluate

pytestmark = pytest.mark.gpu

# set_editnet_workspace_bytes of the PARENT commit (a library built from it, before the trace existed) for the dims of
# editnet_small, editnet_full_b4 and editnet_adaptive_small with maxT = 19: the trace must not have moved them
PARENT_WS_BYTES = {"editnet_small": 729856, "editnet_full_b4": 12663040, "editnet_adaptive_small": 772608}


def _np(t):
    return t.detach().cpu().numpy()


_modules = {}


def _decoder(d, kind="xe"):
    """the HIP-backed decoder of a case (editnet.DecoderC, editnet_rl.DecoderC for greedy, the adaptive one when the case is)"""
    from show_edit_tell_amd import editnet, editnet_adaptive, editnet_rl
    c = d["case"]
    key = (c["wseed"], c["V"], c["D"], "adaptive" if "image_mean" in d else kind)
    if key not in _modules:
        cls = editnet_adaptive.DecoderC if "image_mean" in d else (editnet_rl.DecoderC if kind == "rl" else editnet.DecoderC)
        _modules[key] = load_numpy_state(cls(d["wm"], c["D"], c["D"], c["D"], c["A"], c["F"]), d["sd"])
    return _modules[key]


def _inputs(d):
    mean = to_dev(d["image_mean"]) if "image_mean" in d else None
    return to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"]), mean


def _trace(o, monkeypatch=None, table=None):
    d = o["d"]
    if table is not None:
        monkeypatch.setenv("SET_TOKEN_TABLE", "1" if table else "0")
    X, prev, plen, mean = _inputs(d)
    tr = evaluate.edit_trace(_decoder(d), X, prev, plen, d["wm"], o["tokens"], image_mean=mean)
    torch.cuda.synchronize()
    return tr


def _check(tr, o, max_exempt=0.0):
    """all six outputs + padding against the oracle record `o`; the exempt share is asserted by the caller beforehand"""
    n_steps, S = o["n_steps"], o["S"]
    assert _np(tr.n_steps).tolist() == n_steps.tolist() and tuple(tr.logp.shape) == (len(n_steps), S)
    assert np.array_equal(_np(tr.tokens), o["tok"])
    errs = {}
    for name, tol in (("alpha_c", parity.STATE_TOL), ("alpha_v", parity.STATE_TOL), ("copy_gate", parity.STATE_TOL),
                      ("gate_full", parity.STATE_TOL), ("logp", parity.LOGIT_TOL)):
        got = _np(getattr(tr, name))
        errs[name] = parity.maxerr(got, o[name])
        print("%s max abs err %.3e (tol %.1e)" % (name, errs[name], tol))
    for name, tol in (("alpha_c", parity.STATE_TOL), ("alpha_v", parity.STATE_TOL), ("copy_gate", parity.STATE_TOL),
                      ("gate_full", parity.STATE_TOL), ("logp", parity.LOGIT_TOL)):
        parity.assert_close(_np(getattr(tr, name)), o[name], tol, name)
    sel = _np(tr.select).astype(np.int64)
    live = o["select"] >= 0
    firm = live & (o["gap"] >= O.GAP_MIN)
    assert np.array_equal(sel[firm], o["select"][firm]), "select differs from the oracle's arg-max above the gap"
    soft = live & ~firm
    assert ((sel[soft] == o["select"][soft]) | (sel[soft] == o["second"][soft])).all(), "select outside the oracle's two best"
    # padding: zeros and select = -1 beyond n_steps (exact: the launch writes them)
    pad = ~live
    assert (sel[pad] == -1).all()
    for name in ("alpha_c", "alpha_v", "gate_full", "copy_gate", "logp"):
        assert not _np(getattr(tr, name))[pad].any(), name + " beyond n_steps must be zero"
    # the kernel's own arg-max is the first largest of the alpha_c it recorded
    assert np.array_equal(sel[live], _np(tr.alpha_c)[live].argmax(-1))
    return errs


def _oracle_ok(o, max_share=0.0):
    share, pairs, gap = O.exempt_share(o)
    print("oracle: %d recorded (row, step) pairs, smallest alpha_c gap %.2e, exempt share %.4f" % (pairs, gap, share))
    assert share <= max_share, "exempt share %.4f of %d pairs (smallest gap %.2e)" % (share, pairs, gap)
    assert o["mem_err"] <= 1e-5, "gate recomputed from the trace entries does not give the trace's c2: %.2e" % o["mem_err"]


def test_editnet_small_all_outputs(monkeypatch):
    """editnet_small (6 rows, T = 9, D = 64, V = 203, R = 7; gemv class, unfused copy gate): all six outputs, the zero / -1
    padding beyond n_steps, alpha_c columns beyond the longest previous caption 0.  Oracle alone: 0 exempt of 108 pairs
    (every row of the oracle's greedy decode runs all 18 steps; smallest gap 5.2e-4).  Early-ending rows: the B = 17 / 65
    cases and a shortened copy of these tokens below."""
    o = O.forced("editnet_small")
    _oracle_ok(o)
    tr = _trace(o, monkeypatch, True)           # (token table pinned: the two traces compared below run the same kernels)
    _check(tr, o)
    longest = int(o["d"]["plen"].max())
    assert longest == o["d"]["prev"].shape[1] or not _np(tr.alpha_c)[:, :, longest:].any()
    # the same tokens cut to ragged lengths (prefixes of the oracle's sequences: the records of the kept steps do not change)
    keep = [18, 1, 7, 0, 12, 3]
    toks = [r[:k + 1] for r, k in zip(o["tokens"], keep)]
    d = o["d"]
    X, prev, plen, _ = _inputs(d)
    cut = evaluate.edit_trace(_decoder(d), X, prev, plen, d["wm"], toks)
    assert _np(cut.n_steps).tolist() == keep
    for b, k in enumerate(keep):
        for name in ("alpha_c", "alpha_v", "gate_full", "copy_gate", "logp", "select"):
            got, full = _np(getattr(cut, name)), _np(getattr(tr, name))
            assert np.array_equal(got[b, :k], full[b, :k]), (name, b)
            assert (got[b, k:] == (-1 if name == "select" else 0)).all(), (name, b)


def test_short_previous_caption_columns_are_zero():
    """rows 0 and 4 of editnet_small (previous captions of 1 and 4 words; T = 9): alpha_c columns >= 4, the longest previous
    caption of THIS batch, are exactly 0"""
    o = O.forced("editnet_small", rows=(0, 4))
    _oracle_ok(o)
    tr = _trace(o)
    _check(tr, o)
    assert int(o["d"]["plen"].max()) == 4
    assert not _np(tr.alpha_c)[:, :, 4:].any()


@pytest.mark.parametrize("B,iseed", [(17, 51), (65, 52)])
def test_row_counts_where_the_step_changes_kernel_class(B, iseed):
    """editnet_small's recipe at 17 rows (first row count on the fused copy gate, which keeps no gate) and 65 rows (> 64-row
    tile hints): the trace reads buffers those classes fill differently.  The oracle's greedy rows end at different steps
    (n_steps 3, 10, 18 at B = 17; 5, 10, 17, 18 at B = 65): early-ending rows next to live ones.  Oracle alone: 0 exempt of
    283 pairs (smallest gap 1.4e-3) / 0 of 1148 (5.4e-4)."""
    o = O.forced("editnet_small", B, iseed)
    _oracle_ok(o)
    assert len(set(o["n_steps"].tolist())) >= 3
    _check(_trace(o), o)


def test_single_row_with_a_one_word_previous_caption():
    """B = 1: row 0 of editnet_small alone; its previous caption has one word, so alpha_c = [1, 0, ...] and select = 0"""
    o = O.forced("editnet_small", rows=(0,))
    assert int(o["d"]["plen"][0, 0]) == 1
    _oracle_ok(o)
    tr = _trace(o)
    _check(tr, o)
    n = int(o["n_steps"][0])
    ac = _np(tr.alpha_c)[0, :n]
    assert (ac[:, 0] == 1.0).all() and not ac[:, 1:].any() and not _np(tr.select)[0, :n].any()


@pytest.mark.parametrize("table", [False, True])
def test_full_dimensions_with_and_without_token_table(table, monkeypatch):
    """editnet_full_b4 (D = 1024, V = 10000, R = 36, T = 18), the step with and without the derived token table.  Oracle
    alone: 0 exempt of 72 pairs, smallest gap 1.7e-4."""
    o = O.forced("editnet_full_b4")
    _oracle_ok(o)
    _check(_trace(o, monkeypatch, table), o)


def test_full_dimensions_17_rows_fused_copy_gate():
    """editnet_full_b4's recipe at B = 17 with iseed = 53 (the first seed tried), S = 4 forced steps: the fused copy-gate route
    at the real D.  Exempt share from the oracle alone: 0 of 68 pairs (smallest gap 2.0e-3); asserted <= 2 %."""
    o = O.forced("editnet_full_b4", 17, 53, 4)
    _oracle_ok(o, 0.02)
    assert o["S"] == 4
    _check(_trace(o), o)


def test_adaptive_features_masked_regions():
    """editnet_adaptive_small (R = 12, ragged valid regions, per-image mean): alpha_v is 0 on masked regions and matches
    visual_attention_adaptive's weights (cut by the oracle to the batch's largest valid count) elsewhere.  Oracle alone: 0
    exempt of 108 pairs, smallest gap 3.5e-3."""
    o = O.forced("editnet_adaptive_small")
    _oracle_ok(o)
    tr = _trace(o)
    _check(tr, o)
    nvalid = o["d"]["nvalid"]
    assert nvalid.min() < nvalid.max() <= o["d"]["X"].shape[1]
    av = _np(tr.alpha_v)
    for b, n in enumerate(nvalid):
        assert not av[b, :, int(n):].any(), "masked regions of row %d" % b
        assert abs(float(av[b, 0, :int(n)].sum()) - 1.0) < 1e-5


@pytest.mark.parametrize("name", ["editnet_small", "editnet_full_b4"])
def test_consistent_with_the_greedy_decode(name):
    """decoder(...) greedy -> tokens_from_greedy -> edit_trace: logp[b, t] equals the greedy seq_logp[b, t] within 2e-5 (the
    tolerance of parity.check_two_paths_rows) for t < n_steps[b], and n_steps equals the greedy row lengths"""
    d = O.build(name)
    rl = _decoder(d, "rl")
    X, prev, plen, _ = _inputs(d)
    with torch.no_grad():
        for _ in range(2):
            seq, seq_logp = rl(d["wm"], prev, plen, X, True, False)
    seq_h, lp_h = _np(seq), _np(seq_logp)
    tr = evaluate.edit_trace(rl, X, prev, plen, d["wm"], evaluate.tokens_from_greedy(seq, d["wm"]))
    torch.cuda.synchronize()
    lengths = [int(np.nonzero(r == 0)[0][0]) + 1 if (r == 0).any() else len(r) for r in seq_h]
    assert _np(tr.n_steps).tolist() == lengths
    got = _np(tr.logp)
    for b, n in enumerate(lengths):
        e = float(np.abs(got[b, :n] - lp_h[b, :n]).max())
        print("row %d: %d steps, max |logp - seq_logp| = %.3e" % (b, n, e))
        assert e <= 2e-5, (b, e)


def test_return_trace_on_the_beam_searches(monkeypatch):
    """return_trace=True on beam_search_editnet (k = 3) and beam_search_editnet_batched with the beam_small_e3 inputs: tokens
    and scores identical to the call without the keyword, the attached trace equal to edit_trace on those tokens bit for bit"""
    from oracle import cases
    from show_edit_tell_amd import editnet
    monkeypatch.setenv("SET_TOKEN_TABLE", "1")              # same step kernels in every call of this test
    d = cases.build_beam("beam_small_e3")
    c, wm = d["case"], d["wm"]
    xe = load_numpy_state(editnet.DecoderC(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), d["sd_e"])
    X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])

    def same(a, b):
        for name in ("alpha_c", "select", "copy_gate", "gate_full", "alpha_v", "logp", "n_steps", "tokens"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name

    seqs, scores = evaluate.beam_search_editnet_batched(xe, X, prev, plen, wm, 3, return_scores=True)
    seqs2, scores2, tr = evaluate.beam_search_editnet_batched(xe, X, prev, plen, wm, 3, return_scores=True, return_trace=True)
    assert seqs2 == seqs and np.array_equal(np.array(scores2), np.array(scores), equal_nan=True)
    same(tr, evaluate.edit_trace(xe, X, prev, plen, wm, seqs))
    assert _np(tr.n_steps).tolist() == [len(s) - 1 for s in seqs]
    seqs3, tr3 = evaluate.beam_search_editnet_batched(xe, X, prev, plen, wm, 3, return_trace=True)
    assert seqs3 == seqs
    same(tr3, tr)
    for b in (0, 1, 4):
        one = (X[b:b + 1], prev[b:b + 1], plen[b:b + 1])
        seq, sc = evaluate.beam_search_editnet(xe, *one, wm, 3)
        seq2, sc2, tr1 = evaluate.beam_search_editnet(xe, *one, wm, 3, return_trace=True)
        assert seq2 == seq and (sc2 == sc or (np.isnan(sc) and np.isnan(sc2)))
        same(tr1, evaluate.edit_trace(xe, *one, wm, [seq]))
        assert len(tr1.rows(wm)[0]) == len(seq) - 1
    torch.cuda.synchronize()


def test_trace_does_not_disturb_the_decoder():
    """a greedy decode before and after an edit_trace call on the same decoder returns bit-identical seq / seq_logp, and
    set_editnet_workspace_bytes still returns what the parent commit returned"""
    o = O.forced("editnet_small")
    d = o["d"]
    rl = _decoder(d, "rl")
    X, prev, plen, _ = _inputs(d)
    with torch.no_grad():
        for _ in range(2):
            rl(d["wm"], prev, plen, X, True, False)
        before = [t.clone() for t in rl(d["wm"], prev, plen, X, True, False)]
        evaluate.edit_trace(rl, X, prev, plen, d["wm"], o["tokens"])
        after = rl(d["wm"], prev, plen, X, True, False)
    torch.cuda.synchronize()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    lib = _lib.load()
    for name, want in PARENT_WS_BYTES.items():
        c = O.build(name)["case"]
        dims = _lib.EditNetDims(B=c["B"], T=c["T"], R=c["R"], F=c["F"], D=c["D"], A=c["A"], V=c["V"], maxT=19,
                                adaptive=int(name == "editnet_adaptive_small"))
        assert lib.set_editnet_workspace_bytes(C.byref(dims)) == want, name


def test_raw_abi_errors_leave_outputs_untouched_and_optional_outputs(monkeypatch):
    """NULL out, S = 0, S + 1 > maxT + 1 and a too-small trace_ws return their error codes and leave a sentinel-filled output
    buffer untouched; gate_full = NULL and alpha_v = NULL are accepted and the other outputs are unchanged"""
    from show_edit_tell_amd._lib import ptr, stream_of
    monkeypatch.setenv("SET_TOKEN_TABLE", "0")             # every call below on the same step kernels
    o = O.forced("editnet_small")
    d = o["d"]
    dec = _decoder(d)
    X, prev, plen, _ = _inputs(d)
    dev = X.device
    lib = _lib.load()
    B, S, T, R, D = len(o["tokens"]), o["S"], d["case"]["T"], d["case"]["R"], d["case"]["D"]
    dims = dec._dims(B, T, R, S)
    w = dec._weights(dims)
    ws = dec._workspace(dims)
    tok, n_steps = to_dev(o["tok"].copy()), to_dev(o["n_steps"].astype(np.int32))
    n_tws = lib.set_editnet_edit_trace_workspace_bytes(C.byref(dims), S)
    assert n_tws > 0
    assert lib.set_editnet_edit_trace_workspace_bytes(C.byref(dims), 0) == 0
    assert lib.set_editnet_edit_trace_workspace_bytes(C.byref(dims), S + 1) == 0
    tws = torch.empty(n_tws, dtype=torch.uint8, device=dev)
    sizes = dict(alpha_c=B * S * T, select=B * S, copy_gate=B * S, gate_full=B * S * D, alpha_v=B * S * R, logp=B * S)
    SENT = 0x5A
    bufs = {k: torch.full((n * 4,), SENT, dtype=torch.uint8, device=dev) for k, n in sizes.items()}

    def call(out, S_=S, tws_bytes=n_tws, drop=()):
        st = None if out is None else _lib.EditTrace(**{k: (None if k in drop else v.data_ptr()) for k, v in out.items()})
        return lib.set_editnet_edit_trace(C.byref(w), C.byref(dims), ptr(X), None, ptr(prev), ptr(plen), ptr(tok), tok.shape[1],
                                          ptr(n_steps), S_, None if st is None else C.byref(st), ptr(ws), ws.numel(), ptr(tws),
                                          tws_bytes, stream_of(dev))

    assert call(None) == 1                                   # SET_ERR_ARG
    assert call(bufs, S_=0) == 1
    assert call(bufs, S_=S + 1) == 1                         # S + 1 > maxT + 1
    assert call(bufs, drop=("logp",)) == 1                   # a required output missing
    assert call(bufs, tws_bytes=256) == 4                    # SET_ERR_WORKSPACE
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == SENT).all()), k + " was touched by a refused call"
    assert call(bufs) == 0
    full = {k: v.clone() for k, v in bufs.items()}
    part = {k: torch.full_like(v, SENT) for k, v in bufs.items()}
    assert call(part, drop=("gate_full", "alpha_v")) == 0
    torch.cuda.synchronize()
    for k in sizes:
        if k in ("gate_full", "alpha_v"):
            assert bool((part[k] == SENT).all()), k
        else:
            assert torch.equal(part[k], full[k]), k
    ref = _trace(o)
    assert torch.equal(full["logp"].view(torch.float32).view(B, S), ref.logp)
    assert torch.equal(full["select"].view(torch.int32).view(B, S), ref.select)
