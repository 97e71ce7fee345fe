"""GPU: the DCNet MSE stage (reference `dcnet_with_mse.py`, show_edit_tell_amd.dcnet_with_mse / train.dcnet_mse_train_step)
against tests/golden/dcnet_mse_*.npz, the reference's own classes (tools/make_dcnet_mse_golden.py): the no-grad forward on
the persistent launch and on the per-step loop, both grad routes in eval and train mode with every gradient, the train step,
the data-parallel exchange, the hand-off to stage 3 and the MSE kernels themselves."""
import os

import numpy as np
import pytest
import torch

import parity
from hip_adapter import load_numpy_state, to_dev
from oracle import cases
from test_hip_train_mode import _check_grads, _check_pred
from tools.make_dcnet_mse_golden import affine_state, golden_name

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().numpy()


def mse_module(name, dev=DEV):
    """dcnet_with_mse.DAEWithAR over a stage-1 dcnet.DAE with the case's weights and the golden's affine_hidden"""
    from show_edit_tell_amd import dcnet, dcnet_with_mse
    d = cases.build_dcnet(name)
    c = d["case"]
    stage1 = load_numpy_state(dcnet.DAE(d["wm"], None, c["D"], c["A"], c["C"], c["E"]), d["sd"], dev)
    ar = dcnet_with_mse.DAEWithAR(dae=stage1)
    ar.affine_hidden.load_state_dict({k.split(".", 1)[1]: torch.from_numpy(v.copy()) for k, v in affine_state(c).items()})
    return d, ar.to(dev).eval()


def _inputs(d, dev=DEV):
    return tuple(to_dev(d[k], dev) for k in ("caps", "clen", "prev", "plen"))


def _check_outputs(out, g, pre, c):
    pred, caps_s, dl, sort_ind, gd_fh, last_h = out
    assert np.array_equal(_np(sort_ind), g[pre + "sort_ind"])
    _check_pred(pred, g, pre, c["V"], c["D"] < 1024, dl)
    parity.assert_close(_np(gd_fh), g[pre + "gd_final"], parity.STATE_TOL, pre + "gd_final_hidden")
    parity.assert_close(_np(last_h), g[pre + "last_hidden"], parity.STATE_TOL, pre + "decoder_last_hidden")


def _loss(out):
    from show_edit_tell_amd import autograd_ops as A
    from show_edit_tell_amd.train import xe_loss_sum
    pred, caps_s, dl, _, gd_fh, last_h = out
    ce_sum, n_tok, _, _ = xe_loss_sum(pred, caps_s, dl)
    return ce_sum / n_tok + A.mse_sum(last_h, gd_fh) / last_h.numel()


@pytest.mark.parametrize("name,persistent", [("dcnet_small", "0"), ("dcnet_full_b4", "1"), ("dcnet_full_b4", "0")],
                         ids=["small-per-step", "full_b4-persistent", "full_b4-per-step"])
def test_nograd_forward_vs_golden(name, persistent, monkeypatch):
    """set_dcnet_xe_forward_hidden: dcnet_full_b4 (B = 4) takes the persistent launch unless SET_DEC_PERSISTENT=0 (read per
    call) forces the per-step loop (F/A-merged once the token table is built); dcnet_small's dims only run per step.  Ragged
    caption lengths: rows end at different steps."""
    monkeypatch.setenv("SET_DEC_PERSISTENT", persistent)
    d, ar = mse_module(name)
    g = parity.load(golden_name(name, False))
    with torch.no_grad():
        for _ in range(2):
            out = ar(*_inputs(d))
            assert not out[0].requires_grad
            _check_outputs(out, g, "eval.", d["case"])
        # the plain XE forward (last_hidden NULL) is unchanged by the new entry point
        pred_xe = ar.dae.__class__.__mro__[1].forward(ar.dae, *_inputs(d))[0]
    assert torch.equal(pred_xe, out[0])


@pytest.mark.parametrize("seq", [True, False], ids=["sequence-node", "per-operator"])
@pytest.mark.parametrize("name", ["dcnet_small", "dcnet_full_b4"])
def test_grad_path_eval_mode_vs_golden(name, seq, monkeypatch):
    from show_edit_tell_amd import editnet
    monkeypatch.setattr(editnet, "_XE_SEQUENCE", seq)
    d, ar = mse_module(name)
    g = parity.load(golden_name(name, False))
    out = ar(*_inputs(d))
    assert out[0].requires_grad and out[5].requires_grad
    _check_outputs(out, g, "eval.", d["case"])
    loss = _loss(out)
    assert abs(float(loss.detach()) - float(g["eval.loss"])) < 1e-4
    loss.backward()
    _check_grads(ar, g, "eval.", "%s MSE eval %s" % (name, "node" if seq else "per-op"))


@pytest.mark.parametrize("seq", [True, False], ids=["sequence-node", "per-operator"])
@pytest.mark.parametrize("name", ["dcnet_small", "dcnet_full_b4"])
def test_train_mode_vs_golden(name, seq, monkeypatch):
    from show_edit_tell_amd import editnet, rng
    monkeypatch.setattr(editnet, "_XE_SEQUENCE", seq)
    d, ar = mse_module(name)
    g = parity.load(golden_name(name, True))
    ar.train()
    with rng.dropout_seed(int(g["train.seed"])):
        out = ar(*_inputs(d))
    _check_outputs(out, g, "train.", d["case"])
    loss = _loss(out)
    assert abs(float(loss.detach()) - float(g["train.loss"])) < 1e-4
    loss.backward()
    _check_grads(ar, g, "train.", "%s MSE train %s" % (name, "node" if seq else "per-op"))


def test_train_step_loss_update_and_refusal():
    from show_edit_tell_amd import _lib, rng
    from show_edit_tell_amd.train import dcnet_mse_train_step
    d, ar = mse_module("dcnet_small")
    g = parity.load(golden_name("dcnet_small", True))
    opt = torch.optim.Adam(ar.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in ar.state_dict().items()}
    with rng.dropout_seed(int(g["train.seed"])):
        loss, n_tok = dcnet_mse_train_step(ar, opt, *_inputs(d))
    assert abs(loss - float(g["train.loss"])) < 1e-4
    assert n_tok == int((d["clen"] - 1).sum())
    after = {k: v.detach().clone() for k, v in ar.state_dict().items()}
    assert all(not torch.equal(before[k], after[k]) for k in ("dae.fc.weight", "affine_hidden.weight",
                                                              "dae.caption_encoder.lstm_encoder.weight_hh_l0"))
    # a non-finite loss is refused before the optimizer runs.  (Made non-finite through the MSE term: a caption id outside
    # [0, V) would also reach the embedding gradient's index_add_, which range-checks on the device.)
    with torch.no_grad():
        ar.affine_hidden.bias[0] = float("nan")
    after = {k: v.detach().clone() for k, v in ar.state_dict().items()}
    with pytest.raises(_lib.SetError):
        dcnet_mse_train_step(ar, opt, *_inputs(d))
    for k, v in ar.state_dict().items():                     # no optimizer step was taken
        assert torch.equal(v.view(torch.int32), after[k].view(torch.int32)), k


def _dp_worker(rank, world, port, ret):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_hip_dcnet_mse import _inputs, mse_module
    from show_edit_tell_amd import train
    train.BUCKET_BYTES = 64 << 10                    # several buckets in flight
    d, ar = mse_module("dcnet_small")
    full = _inputs(d)
    grads = lambda: {k: p.grad.detach().cpu().double().numpy().copy() for k, p in ar.named_parameters() if p.grad is not None}
    loss_ref, n_ref, _ = train.dcnet_mse_backward(ar, *full, reduce=False)
    ref = grads()
    B = full[0].shape[0]
    cuts = [0, max(1, B // 3), B]                     # ragged shards: a mean of means would be wrong
    shard = tuple(t[cuts[rank]:cuts[rank + 1]].contiguous() for t in full)
    loss, n_tok, _ = train.dcnet_mse_backward(ar, *shard)
    got = grads()
    floor = 1e-6 * max(float(np.sqrt((r ** 2).sum())) for r in ref.values())
    worst = max(float(max(np.abs(got[k] - ref[k]).max() - floor, 0.0) / max(np.abs(ref[k]).max(), 1e-6)) for k in ref)
    ret[rank] = dict(worst=worst, keys=sorted(got) == sorted(ref), loss=loss, loss_ref=loss_ref, n_tok=n_tok, n_ref=n_ref)
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_two_ranks_equal_the_concatenated_batch():
    """world size 2 over gloo on one device (tests/test_hip_dp.py's pattern): SUM-reduced gradients of the two shards ==
    the single-process gradients of the whole batch (CE normalised by the global token count, the MSE by B_global * D)"""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_dp_worker, args=(2, 29500 + (os.getpid() % 150), ret), nprocs=2, join=True)
    r0, r1 = ret[0], ret[1]
    assert r0["keys"] and r1["keys"]
    assert max(r0["worst"], r1["worst"]) < 2e-4, dict(ret)
    assert r0["n_tok"] + r1["n_tok"] == r0["n_ref"]
    assert abs(r0["loss"] - r1["loss"]) < 1e-12
    assert abs(r0["loss"] - r0["loss_ref"]) < 1e-5 * max(1.0, abs(r0["loss_ref"]))


def test_hand_off_to_stage3_scst():
    """stage-2 state -> dcnet_rl.DAEWithAR (strict) -> one dcnet_scst_train_step runs; affine_hidden gets no gradient"""
    from show_edit_tell_amd import ciderd, dcnet_rl
    from show_edit_tell_amd.train import dcnet_mse_train_step, dcnet_scst_train_step
    d, ar = mse_module("dcnet_small")
    c, wm = d["case"], d["wm"]
    opt = torch.optim.Adam(ar.parameters(), lr=1e-3)
    dcnet_mse_train_step(ar, opt, *_inputs(d))
    rl = dcnet_rl.DAEWithAR(dae=dcnet_rl.DAE(wm, None, c["D"], c["A"], c["C"], c["E"])).to(DEV)
    rl.load_state_dict(ar.state_dict(), strict=True)
    B, V = c["B"], len(wm)
    rng = np.random.default_rng(3)
    allcaps = np.zeros((B, 5, 12), dtype=np.int64)
    for b in range(B):
        for j in range(5):
            n = int(rng.integers(3, 9))
            allcaps[b, j, 0] = wm["<start>"]
            allcaps[b, j, 1:1 + n] = rng.integers(1, V - 4, n)
            allcaps[b, j, 1 + n] = wm["<end>"]
    gt = ciderd.ground_truth_lists(allcaps, wm)
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(x) for x in caps] for caps in gt])
    scorer = ciderd.CiderD(df, max(docs, 2))
    opt3 = torch.optim.Adam(rl.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in rl.state_dict().items()}
    torch.manual_seed(4)
    reward, loss = dcnet_scst_train_step(rl, opt3, wm, to_dev(d["prev"]), to_dev(d["plen"]), gt, scorer)
    assert np.isfinite(reward) and np.isfinite(loss)
    assert rl.affine_hidden.weight.grad is None
    after = rl.state_dict()
    assert torch.equal(before["affine_hidden.weight"], after["affine_hidden.weight"])
    assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith("dae."))


@pytest.mark.parametrize("n", [1, 63, 4 * 1024 + 3, 128 * 1024 + 5])
def test_mse_kernels_vs_float64(n):
    import ctypes as C
    from show_edit_tell_amd import _lib, autograd_ops as A
    gen = torch.Generator().manual_seed(n)
    a64 = torch.randn(n, generator=gen, dtype=torch.float64)
    b64 = torch.randn(n, generator=gen, dtype=torch.float64)
    a = a64.float().to(DEV).requires_grad_(True)
    b = b64.float().to(DEV).requires_grad_(True)
    s1 = A.mse_sum(a, b)
    s2 = A.mse_sum(a, b)
    assert torch.equal(s1, s2)                               # fixed reduction order: the same bits on every call
    ref = float(((a64.float().double() - b64.float().double()) ** 2).sum())
    assert abs(float(s1) - ref) <= 1e-5 * ref + 1e-7
    s1.backward(torch.tensor(0.7, device=DEV))
    diff = a64.float().double() - b64.float().double()
    np.testing.assert_allclose(_np(a.grad), (1.4 * diff).numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(_np(b.grad), (-1.4 * diff).numpy(), rtol=1e-6, atol=1e-6)
    # the ABI directly: scale without a device factor, one output only
    lib = _lib.load()
    da = torch.empty(n, device=DEV)
    assert lib.set_mse_bwd_f32(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n, 0.5, None, C.c_void_p(da.data_ptr()),
                               None, None) == 0
    np.testing.assert_allclose(_np(da), (0.5 * diff).numpy(), rtol=1e-6, atol=1e-6)
    assert lib.set_mse_sum_f32(None, None, n, None, None) == 1                          # SET_ERR_ARG before any launch
