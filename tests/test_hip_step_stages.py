"""GPU: every stage of ONE decode timestep against its float64 restatement, at the shapes where the step changes route.

set_editnet_begin / set_dcnet_begin run once, then set_*_step a few timesteps through the C ABI.  Around each step the
recurrent state and every intermediate are read back through set_*_ws_tensor, and each stage's device output is compared with
tests/step_stage_oracle.py evaluated on the DEVICE's own inputs to that stage: attention_lstm on the state read before the
step, the two attentions on the device's h1, `select` on the device's alpha_c, copy_lstm on the device's h1 / attend_cap /
attend_img / sel, fc on the device's h2.  Rounding is therefore not carried from stage to stage, the hard arg-max cannot
amplify it, and no row is filtered: every row of every case is compared.  The shapes are tests/step_stage_grid.py (the routes
they reach are asserted on the CPU, tests/test_step_stage_oracle_cpu.py); every EditNet case runs without and with the
inference token table, both judged by the same float64 stages.

Tolerances: parity.STATE_TOL for states, contexts and attention weights, parity.LOGIT_TOL for the logits, relative to
max|ref| of the tensor AND absolute as parity.assert_close applies them (the smaller of the two bounds decides).  Exact
checks: alpha_c is 0 behind a row's length, alpha is 0 on masked regions, `sel` is the selected Mem row to 1 ulp, and rows
>= bt of every tensor (and of the caller's logits) keep their bits.

STEP_STAGES_ERRORS_OUT=<path> additionally writes, per model, grid id and stage, the largest error as a fraction of its
bound, next to the same figure for the float32 numpy oracle's stage on the same inputs (profiles/step_stages_errors.json).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import parity
import step_stage_grid as G
import step_stage_oracle as SO
from hip_adapter import load_numpy_state, to_dev
from oracle import cases, dcnet_np as DN, editnet_np as EN
from show_edit_tell_amd import _lib, synth
from stage_judge import judge, write_report

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
RATIOS = {}            # (model, grid id) -> stage -> [largest hip ratio, largest float32-oracle ratio]


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("STEP_STAGES_ERRORS_OUT")
    if not path or not RATIOS:
        return
    write_report(path, "[hip, float32 numpy oracle]: largest |stage output - float64 stage| / (tol * min(max|ref|, 1)) over all "
                 "timesteps, runs and token-table settings of a grid id; tol = parity.STATE_TOL, parity.LOGIT_TOL for fc.logits",
                 RATIOS)


_judge = functools.partial(judge, RATIOS)          # (key, stage, got, ref, tol, what, f32=None): tests/stage_judge.py


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _tokens(seed, steps, B, bts, V):
    """(steps, B) ids from synth.integers with 0 and V - 1 forced into every step's active rows (one row: alternating)"""
    toks = synth.integers(seed, "step.toks", (steps, B), 0, V)
    for t, n in enumerate(bts):
        if n == 1:
            toks[t, 0] = 0 if t % 2 == 0 else V - 1
        else:
            toks[t, t % n], toks[t, (t + 1) % n] = 0, V - 1
    return toks


def _step_rows(B, bt):
    """rows per timestep: G.STEPS steps of bt rows; a shrunk batch (bt < B) first takes one step at full width, as the
    teacher-forced loop does, so that the rows behind bt hold live state when the narrow steps must leave them alone"""
    return ([B] if bt < B else []) + [bt] * G.STEPS


def _prev(seed, B, T, V):
    prev, plen = cases._prev(dict(iseed=seed, B=B, T=T, V=V))          # lengths 1, T and T // 2 forced
    plen = plen.reshape(-1)
    assert plen.min() == 1 and plen.max() == T and (B <= 4 or T // 2 in plen)
    return prev, plen


_MODELS = {}


def _editnet_model(D, A, F, V, adaptive):
    key = ("editnet", D, A, F, V, adaptive)
    if key not in _MODELS:
        from show_edit_tell_amd import editnet, editnet_adaptive
        wm = synth.word_map(V)
        sd = synth.editnet_state(31, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
        cls = editnet_adaptive.DecoderC if adaptive else editnet.DecoderC
        _MODELS.clear()                                   # one model on the device at a time
        _MODELS[key] = (load_numpy_state(cls(wm, D, D, D, A, F), sd), EN.cast_params(sd, np.float64), EN.cast_params(sd))
    return _MODELS[key]


def _dcnet_model(D, A, Cc, E, V):
    key = ("dcnet", D, A, Cc, E, V)
    if key not in _MODELS:
        from show_edit_tell_amd import dcnet
        sd = synth.dcnet_state(37, V, D, A, Cc, E, 3.0, 8.0, 3.0)
        _MODELS.clear()
        _MODELS[key] = (load_numpy_state(dcnet.DAE(synth.word_map(V), None, D, A, Cc, E), sd),
                        DN.cast_params(sd, np.float64), DN.cast_params(sd))
    return _MODELS[key]


def _weights(model, dims, table):
    if not table:
        w = model._weights()
        assert not w.tok_table
        return w
    for _ in range(2):                                    # the table is built once the same weights were seen twice
        w = model._weights(dims)
    assert w.tok_table, "no token table attached"
    return w


def _reader(model, dims, ws, shapes):
    def get(name, rows=None):
        a = model.ws_tensor(dims, name, shapes[name], ws=ws).detach().cpu().numpy().copy()
        return a if rows is None else a[:rows]
    return get


def _check_tail_rows(before, after, n, what):
    for k in before:
        assert np.array_equal(_bits(before[k][n:]), _bits(after[k][n:])), "%s: %s changed in rows >= %d" % (what, k, n)


@pytest.mark.parametrize("case", G.editnet_cases(), ids=G.case_id)
def test_editnet_step_stages(case):
    gid, B, bt, table = case
    dm = G.editnet_dims(gid)
    D, A, F, V, T, R, adaptive = (dm[k] for k in ("D", "A", "F", "V", "T", "R", "adaptive"))
    model, P, P32 = _editnet_model(D, A, F, V, adaptive)
    seed = 100 + sorted(G.EDITNET_GRID).index(gid)
    key = ("editnet", gid)
    prev, plen = _prev(seed, B, T, V)
    mean = None
    if adaptive:
        _, _, nv = synth.adaptive_features(seed, B, R, F, min(3, R))
        nv[0], nv[1] = 1, R                               # a row with one valid region and a row with all of them
        X = synth.features(seed, B, R, F) * (np.arange(R)[None, :] < nv[:, None])[:, :, None].astype(np.float32)
        mean = (X.sum(1) / nv[:, None].astype(np.float32)).astype(np.float32)
    else:
        X = synth.features(seed, B, R, F)
    lib = _lib.load()
    dims = model._dims(B, T, R, 19)
    ws = model._new_workspace(dims)
    w = _weights(model, dims, table)
    Xd, prevd, plend = to_dev(X), to_dev(prev), to_dev(plen)
    meand = None if mean is None else to_dev(mean)
    st = _lib.stream_of(Xd.device)
    _lib.check(lib.set_editnet_begin(C.byref(w), C.byref(dims), _lib.ptr(Xd), _lib.ptr(meand), _lib.ptr(prevd),
                                     _lib.ptr(plend), _lib.ptr(ws), ws.numel(), st), "begin")
    shapes = dict(H=(B, T, D), M=(B, T, D), mask=(B, T), final_hidden=(B, D), image_mean=(B, F), att1=(B, R, A),
                  att1_c=(B, T, A), rmask=(B, R), h1=(B, D), c1=(B, D), h2=(B, D), c2=(B, D), alpha_c=(B, T), alpha=(B, R),
                  attend_img=(B, F), attend_cap=(B, D), sel=(B, D))
    get = _reader(model, dims, ws, shapes)
    H, Mem, mask, fh, imean, att1, att1_c = (get(k) for k in ("H", "M", "mask", "final_hidden", "image_mean", "att1", "att1_c"))
    behind = np.arange(T)[None, :] >= plen[:, None]
    assert np.array_equal(mask != 0, ~behind), "prologue mask"
    rmask = None
    if adaptive:
        rmask = get("rmask")
        assert np.array_equal(rmask, SO.region_mask(P, X)), "region mask differs from the rule above region_masks_k"
        assert rmask[0].sum() == 1 and rmask[1].sum() == R
    state = ("h1", "c1", "h2", "c2", "alpha_c", "alpha", "attend_img", "attend_cap", "sel")
    bts = _step_rows(B, bt)
    toks = _tokens(seed, len(bts), B, bts, V)
    logits = torch.empty(B, V, dtype=torch.float32, device=Xd.device)
    for t, n in enumerate(bts):
        what = "%s step %d (%d rows) " % (G.case_id(case), t, n)
        before = {k: get(k) for k in state}
        logits.fill_(SENTINEL)
        tok = to_dev(toks[t, :n])
        _lib.check(lib.set_editnet_step(C.byref(w), C.byref(dims), _lib.ptr(Xd), _lib.ptr(tok), 1, n, _lib.ptr(logits), V,
                                        _lib.ptr(ws), ws.numel(), st), "step")
        torch.cuda.synchronize()
        after = {k: get(k) for k in state}
        lg = logits.cpu().numpy()
        a = {k: v[:n] for k, v in after.items()}
        b = {k: v[:n] for k, v in before.items()}
        tk = toks[t, :n]
        # ---- attention LSTM
        h1, c1 = SO.attention_lstm(P, tk, fh[:n], b["h2"], imean[:n], b["h1"], b["c1"])
        o32 = EN.lstm_cell(P32, "attention_lstm", np.concatenate([EN.embed(P32, tk), fh[:n], b["h2"], imean[:n]], 1), b["h1"],
                           b["c1"])
        _judge(key, "attention_lstm.h1", a["h1"], h1, parity.STATE_TOL, what + "h1", o32[0])
        _judge(key, "attention_lstm.c1", a["c1"], c1, parity.STATE_TOL, what + "c1", o32[1])
        # ---- caption attention + context gate
        alpha_c, attend_cap = SO.caption_attention(P, H[:n], att1_c[:n], a["h1"], tk, mask[:n])
        g32, ac32 = EN.caption_attention(P32, H[:n], a["h1"], EN.embed(P32, tk), mask[:n], att1_c[:n])
        _judge(key, "caption_attention.alpha_c", a["alpha_c"], alpha_c, parity.STATE_TOL, what + "alpha_c", ac32)
        _judge(key, "caption_attention.attend_cap", a["attend_cap"], attend_cap, parity.STATE_TOL, what + "attend_cap", g32)
        assert not a["alpha_c"][behind[:n]].any(), what + "alpha_c behind a row's length"
        np.testing.assert_allclose(a["alpha_c"].astype(np.float64).sum(1), 1.0, atol=1e-5)
        # ---- visual attention
        alpha, attend_img = SO.visual_attention(P, X[:n], att1[:n], a["h1"], None if rmask is None else rmask[:n])
        if adaptive:
            i32, al32 = EN.visual_attention_adaptive(P32, X[:n], a["h1"], return_alpha=True)
            al32 = np.pad(al32, ((0, 0), (0, R - al32.shape[1])))
        else:
            i32, al32 = EN.visual_attention(P32, X[:n], a["h1"], att1[:n], return_alpha=True)
        _judge(key, "visual_attention.alpha", a["alpha"], alpha, parity.STATE_TOL, what + "alpha", al32)
        _judge(key, "visual_attention.attend_img", a["attend_img"], attend_img, parity.STATE_TOL, what + "attend_img", i32)
        if adaptive:
            assert not a["alpha"][rmask[:n] == 0].any(), what + "alpha on masked regions"
        # ---- select, on the device's own alpha_c
        sel = SO.select(Mem[:n], a["alpha_c"])
        _judge(key, "select.sel", a["sel"], sel, parity.STATE_TOL, what + "sel", EN.select(Mem[:n], a["alpha_c"]))
        row = Mem[np.arange(n), SO.select_index(a["alpha_c"])]
        assert (np.abs(a["sel"].astype(np.float64) - row) <= np.spacing(np.abs(row))).all(), what + "sel is not the Mem row"
        # ---- copy LSTM
        h2, c2 = SO.copy_lstm(P, a["h1"], a["attend_cap"], a["attend_img"], b["h2"], b["c2"], a["sel"])
        o32 = EN.copy_lstm(P32, np.concatenate([a["h1"], a["attend_cap"], a["attend_img"]], 1), b["h2"], b["c2"], a["sel"])
        _judge(key, "copy_lstm.h2", a["h2"], h2, parity.STATE_TOL, what + "h2", o32[0])
        _judge(key, "copy_lstm.c2", a["c2"], c2, parity.STATE_TOL, what + "c2", o32[1])
        # ---- fc
        _judge(key, "fc.logits", lg[:n], SO.fc(P, a["h2"]), parity.LOGIT_TOL, what + "logits", EN._linear(a["h2"], P32, "fc"))
        # ---- rows the step was not asked for
        _check_tail_rows(before, after, n, what)
        assert (lg[n:] == SENTINEL).all(), what + "logits rows >= bt were written"


@pytest.mark.parametrize("case", G.dcnet_cases(), ids=G.case_id)
def test_dcnet_step_stages(case):
    gid, B, bt = case
    dm = G.dcnet_dims(gid)
    D, A, Cc, E, V, T = (dm[k] for k in ("D", "A", "C", "E", "V", "T"))
    model, P, P32 = _dcnet_model(D, A, Cc, E, V)
    seed = 200 + sorted(G.DCNET_GRID).index(gid)
    key = ("dcnet", gid)
    prev, plen = _prev(seed, B, T, V)
    lib = _lib.load()
    dims = model._dims(B, T, 19)
    ws = model._new_workspace(dims)
    w = _weights(model, dims, False)
    prevd, plend = to_dev(prev), to_dev(plen)
    st = _lib.stream_of(prevd.device)
    _lib.check(lib.set_dcnet_begin(C.byref(w), C.byref(dims), _lib.ptr(prevd), _lib.ptr(plend), _lib.ptr(ws), ws.numel(), st),
               "begin")
    shapes = dict(enc=(B, T, 2 * Cc), mask=(B, T), final_hidden=(B, 2 * Cc), att1_c=(B, T, A), h1=(B, D), c1=(B, D), h2=(B, D),
                  c2=(B, D), alpha_c=(B, T), attend_cap=(B, 2 * Cc))
    get = _reader(model, dims, ws, shapes)
    enc, mask, fh, att1_c = (get(k) for k in ("enc", "mask", "final_hidden", "att1_c"))
    behind = np.arange(T)[None, :] >= plen[:, None]
    assert np.array_equal(mask != 0, ~behind), "prologue mask"
    state = ("h1", "c1", "h2", "c2", "alpha_c", "attend_cap")
    bts = _step_rows(B, bt)
    toks = _tokens(seed, len(bts), B, bts, V)
    logits = torch.empty(B, V, dtype=torch.float32, device=prevd.device)
    for t, n in enumerate(bts):
        what = "dcnet %s step %d (%d rows) " % (G.case_id(case), t, n)
        before = {k: get(k) for k in state}
        logits.fill_(SENTINEL)
        tok = to_dev(toks[t, :n])
        _lib.check(lib.set_dcnet_step(C.byref(w), C.byref(dims), _lib.ptr(tok), 1, n, _lib.ptr(logits), V, _lib.ptr(ws),
                                      ws.numel(), st), "step")
        torch.cuda.synchronize()
        after = {k: get(k) for k in state}
        lg = logits.cpu().numpy()
        a = {k: v[:n] for k, v in after.items()}
        b = {k: v[:n] for k, v in before.items()}
        tk = toks[t, :n]
        h1, c1 = SO.dc_attention_lstm(P, tk, fh[:n], b["h2"], b["h1"], b["c1"])
        o32 = DN.lstm_cell(P32, "attention_lstm", np.concatenate([DN.embed(P32, tk), fh[:n], b["h2"]], 1), b["h1"], b["c1"])
        _judge(key, "attention_lstm.h1", a["h1"], h1, parity.STATE_TOL, what + "h1", o32[0])
        _judge(key, "attention_lstm.c1", a["c1"], c1, parity.STATE_TOL, what + "c1", o32[1])
        alpha_c, attend_cap = SO.dc_caption_attention(P, enc[:n], att1_c[:n], a["h1"], mask[:n])
        c32, ac32 = DN.caption_attention(P32, enc[:n], a["h1"], mask[:n], att1_c[:n], True)
        _judge(key, "caption_attention.alpha_c", a["alpha_c"], alpha_c, parity.STATE_TOL, what + "alpha_c", ac32)
        _judge(key, "caption_attention.attend_cap", a["attend_cap"], attend_cap, parity.STATE_TOL, what + "attend_cap", c32)
        assert not a["alpha_c"][behind[:n]].any(), what + "alpha_c behind a row's length"
        h2, c2 = SO.dc_language_lstm(P, a["h1"], a["attend_cap"], b["h2"], b["c2"])
        o32 = DN.lstm_cell(P32, "language_lstm", np.concatenate([a["h1"], a["attend_cap"]], 1), b["h2"], b["c2"])
        _judge(key, "language_lstm.h2", a["h2"], h2, parity.STATE_TOL, what + "h2", o32[0])
        _judge(key, "language_lstm.c2", a["c2"], c2, parity.STATE_TOL, what + "c2", o32[1])
        _judge(key, "fc.logits", lg[:n], SO.fc(P, a["h2"]), parity.LOGIT_TOL, what + "logits", DN._linear(a["h2"], P32, "fc"))
        _check_tail_rows(before, after, n, what)
        assert (lg[n:] == SENTINEL).all(), what + "logits rows >= bt were written"
