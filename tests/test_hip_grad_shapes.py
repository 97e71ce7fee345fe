"""GPU: every parameter gradient of EditNet, adaptive EditNet and DCNet (plus the DCNet MSE stage) through both
grad-enabled routes at AWKWARD shapes, against a float64 torch-autograd statement of the same model on the CPU
(oracle/xe_grad_torch.py, pinned to the reference's own autograd by tests/test_xe_grad_oracle_cpu.py).

The other gradient tests either run at the few shapes a reference golden was captured for, or compare one HIP schedule
with another (both sides run the same backward kernels).  The grid (tests/grad_grid.py) reaches the shape-dependent
branches those leave out: B on both sides of the 16- / 64- / 128-row switches, B = 1, R = 1 / 2 / 5 / 100, valid-region
counts around the two-slice switch at 48, T = 1, previous captions of length 1, tied and minimal caption lengths,
D = 128 / 512 / 2048, V & 3 != 0 with >= 64 rows per timestep.

Criteria are the project's own (tests/test_hip_train.py::_check_grads, on the FULL arrays): scores within
parity.LOGIT_TOL, loss within 1e-4, gradient norms within 1e-4 * |ref| + floor, elements within 1e-4 * max|ref| + floor,
floor = 1e-6 * the model's largest gradient norm.  No row, parameter or element is excused: the CPU test guarantees that
no grid row has a hard-select near-tie or a ReLU kink within fp32 summation noise."""
import contextlib

import numpy as np
import pytest
import torch

import grad_grid as G
import parity
from hip_adapter import load_numpy_state, to_dev

pytestmark = pytest.mark.gpu

ROUTES = pytest.mark.parametrize("seq", [True, False], ids=["sequence-node", "per-operator"])
DEFER = pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "deferred"])


def _np(t):
    return t.detach().cpu().numpy()


def _module(kind, d):
    from show_edit_tell_amd import dcnet, dcnet_with_mse, editnet, editnet_adaptive
    m = d["dims"]
    if kind in ("editnet", "adaptive"):
        cls = editnet.DecoderC if kind == "editnet" else editnet_adaptive.DecoderC
        return load_numpy_state(cls(d["wm"], m["D"], m["D"], m["D"], m["A"], m["F"]), d["sd"])
    dae = load_numpy_state(dcnet.DAE(d["wm"], None, m["D"], m["A"], m["C"], m["E"]), d["sd"])
    if kind == "dcnet":
        return dae
    ar = dcnet_with_mse.DAEWithAR(dae=dae)
    ar.affine_hidden.load_state_dict({k.split(".", 1)[1]: torch.from_numpy(v.copy()) for k, v in d["affine"].items()})
    return ar.to("cuda:0").eval()


def _forward(kind, mod, d):
    caps, clen, prev, plen = (to_dev(d[k]) for k in ("caps", "clen", "prev", "plen"))
    if kind == "editnet":
        return mod(to_dev(d["X"]), caps, clen, prev, plen, False, 0.0)
    if kind == "adaptive":
        return mod(to_dev(d["X"]), to_dev(d["image_mean"]), caps, clen, prev, plen, False, 0.0)
    return mod(caps, clen, prev, plen)


def _run(kind, name, seq, deferred, train, monkeypatch):
    from show_edit_tell_amd import autograd_ops as A, editnet, rng
    from show_edit_tell_amd.autograd_ops import deferred_param_grads
    from show_edit_tell_amd.train import xe_loss_sum
    monkeypatch.setattr(editnet, "_XE_SEQUENCE", seq)
    d = G.build(kind, name)
    ref = G.oracle(kind, name, train)
    mod = _module(kind, d)
    what = "%s %s %s %s %s" % (kind, name, "train" if train else "eval", "node" if seq else "per-op",
                               "deferred" if deferred else "immediate")
    if kind == "dcnet_mse":
        # the product's own stage-2 function: forward, CE / n_tok + SSE / (B * D), deferred backward with its on_ready
        # hook, no optimizer step (one rank: the normalisers are the local ones)
        from show_edit_tell_amd.train import dcnet_mse_backward
        caps, clen, prev, plen = (to_dev(d[k]) for k in ("caps", "clen", "prev", "plen"))
        loss, n_tok, _ = dcnet_mse_backward(mod, caps, clen, prev, plen, reduce=False)
        assert n_tok == sum(ref["dl"])
        assert abs(loss - ref["loss"]) < 1e-4, (what, loss, ref["loss"])
        G.check_grads(((k, None if p.grad is None else _np(p.grad)) for k, p in mod.named_parameters()), ref["grads"], what)
        mod.zero_grad(set_to_none=True)     # then the outputs of the same forward, below
    if train:
        mod.train()
        with rng.dropout_seed(G.TRAIN["dcnet" if kind == "dcnet_mse" else kind][name]):
            out = _forward(kind, mod, d)
    else:
        out = _forward(kind, mod, d)
    pred, caps_s, dl, sort_ind = out[:4]
    assert pred.requires_grad
    assert list(dl) == list(ref["dl"])
    # scores per original sample; exactly zero behind each caption's length
    inv, inv_o = parity.unsort(_np(sort_ind)), parity.unsort(ref["sort_ind"])
    mine = _np(pred)[inv]
    err = parity.assert_close(mine, ref["pred"][inv_o], parity.LOGIT_TOL, what + " scores")
    dl_orig = np.asarray(dl)[inv]
    for b in range(mine.shape[0]):
        assert not mine[b, dl_orig[b]:].any(), (what, "scores behind the caption's length", b)
    loss_sum, n_tok, _, _ = xe_loss_sum(pred, caps_s, dl)
    loss = loss_sum / n_tok
    if kind == "adaptive":                   # CE + MSE (editnet_adaptive.py:594-596)
        gd_fh, last_h = out[4], out[5]
        loss = loss + torch.nn.functional.mse_loss(last_h, gd_fh)
    elif kind == "dcnet_mse":                # train.dcnet_mse_backward's loss (dcnet_with_mse.py:388-392)
        gd_fh, last_h = out[4], out[5]
        loss = loss + A.mse_sum(last_h, gd_fh) / last_h.numel()
    if kind in ("adaptive", "dcnet_mse"):
        parity.assert_close(_np(gd_fh), ref["gd_final"], parity.STATE_TOL, what + " gd_final_hidden")
        parity.assert_close(_np(last_h), ref["last_hidden"], parity.STATE_TOL, what + " decoder_last_hidden")
    print(what, "max score err %.2e" % err, "loss", float(loss.detach()), "ref", ref["loss"])
    assert abs(float(loss.detach()) - ref["loss"]) < 1e-4, (what, float(loss.detach()), ref["loss"])
    with (deferred_param_grads() if deferred else contextlib.nullcontext()):
        loss.backward()
    G.check_grads(((k, None if p.grad is None else _np(p.grad)) for k, p in mod.named_parameters()), ref["grads"], what)


@ROUTES
@DEFER
@pytest.mark.parametrize("name", list(G.EDITNET))
def test_editnet_gradients_vs_float64_autograd(name, deferred, seq, monkeypatch):
    _run("editnet", name, seq, deferred, False, monkeypatch)


@ROUTES
@DEFER
@pytest.mark.parametrize("name", list(G.ADAPTIVE))
def test_adaptive_gradients_vs_float64_autograd(name, deferred, seq, monkeypatch):
    """CE + MSE(decoder_last_hidden, gd_final_hidden); valid-region counts 1, 47, 48, 49 and R"""
    _run("adaptive", name, seq, deferred, False, monkeypatch)


@ROUTES
@DEFER
@pytest.mark.parametrize("name", list(G.DCNET))
def test_dcnet_gradients_vs_float64_autograd(name, deferred, seq, monkeypatch):
    _run("dcnet", name, seq, deferred, False, monkeypatch)


@ROUTES
@pytest.mark.parametrize("name", list(G.DCNET_MSE))
def test_dcnet_mse_stage_gradients_vs_float64_autograd(name, seq, monkeypatch):
    """the stage-2 loss through DAEWithAR: train.dcnet_mse_backward itself (forward, loss, deferred backward, no optimizer
    step), then the six outputs of the same forward and the loss assembled from them"""
    _run("dcnet_mse", name, seq, True, False, monkeypatch)


@ROUTES
@pytest.mark.parametrize("kind,name", [(k, n) for k, tab in G.TRAIN.items() for n in tab])
def test_train_mode_gradients_vs_float64_autograd(kind, name, seq, monkeypatch):
    """model.train() under rng.dropout_seed(seed > 2**32) against the float64 statement fed the numpy keep masks
    (oracle.xe_grad_torch.philox_masks).

    Adaptive row a_dead settles what happens when the dropout zeroes a valid region row entirely (at one of its four steps
    both non-zero entries of a non-trailing region of the longest row are dropped; tests/test_xe_grad_oracle_cpu.py asserts
    that, and that no other row has such a step).  The reference then truncates alpha and the features to the COUNT of
    unmasked regions (editnet_adaptive.py:455-456), which removes that row's last valid region from the context; a rule that
    only masks the zeroed region keeps it, and differs from the reference's scores and gradients.  editnet.py mirrors the
    reference: the per-operator route zeroes the feature rows behind the count, the sequence node detects such a batch and
    hands it to the per-operator route (asserted here through xe_sequence.TRUNCATION_FALLBACKS)."""
    from show_edit_tell_amd import xe_sequence
    before = xe_sequence.TRUNCATION_FALLBACKS
    _run(kind, name, seq, False, True, monkeypatch)
    assert xe_sequence.TRUNCATION_FALLBACKS - before == (1 if (name == "a_dead" and seq) else 0)
