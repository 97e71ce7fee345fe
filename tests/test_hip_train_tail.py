"""GPU: the training tail — token cross-entropy and MSE (csrc/loss.hip), clip-grad-norm + Adam (csrc/optim.hip) — against
the float64 oracle of tests/train_tail_oracle.py, at the shapes, strides and row families where such kernels go wrong, plus
the memory contract and the refusals of the C ABI.

Tolerances.  Every compared quantity is measured twice against the oracle on the same inputs: the library's kernel, and
torch's fp32 route (F.cross_entropy / logsumexp on the device; clip_grad_norm_ + torch.optim.Adam; ((a-b)**2).sum()).  Units:
2^-24 max(1, max |finite x_row|, |ref|) for a loss or lse row, 2^-24 |dloss| for the score gradient, 2^-24 max(1, max |ref|)
per tensor for everything else.  `python tests/test_hip_train_tail.py OUT.json` writes both figures per case family
(profiles/train_tail_errors.json); a test then asserts

    kernel error <= 2 x (torch-fp32 error of the family, from the file) + 2 units

— 2 x for another, equally valid summation order, 2 units for the final roundings of the stored result.  The bound comes
from the reference route's figure, never from the kernel's own.  Zeros, untouched buffers and repeated calls are compared bit
for bit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):            # also when run as a script (the measured figures, below)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import train_tail_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

ERRORS_FILE = os.path.join(ROOT, "profiles", "train_tail_errors.json")
SET_OK, SET_ERR_ARG, SET_ERR_UNSUPPORTED, SET_ERR_WORKSPACE = 0, 1, 2, 4
DLOSS = 0.37
NAN_BITS, TAIL_BITS, TAIL = 0x7FC0BEEF, 0x5EA7D00D, 64
_bounds = {}


def _dev():
    return torch.device("cuda:0")


def _lib():
    from show_edit_tell_amd import _lib as L
    return L.load()


def _stream():
    from show_edit_tell_amd._lib import stream_of
    return stream_of(_dev())


def _hold(family, errs):
    """errs: {quantity: (kernel error, torch-fp32 error)} in units; the bound is read from the committed figures"""
    if not _bounds:
        with open(ERRORS_FILE) as f:
            _bounds.update(json.load(f)["families"])
    bad = []
    for q, (k, t) in sorted(errs.items()):
        bound = 2.0 * _bounds[family][q]["torch_fp32"] + 2.0
        print("%s %s: kernel %.3f  torch fp32 %.3f (file %.3f)  bound %.3f units" % (family, q, k, t, _bounds[family][q]["torch_fp32"], bound))
        if not k <= bound:
            bad.append((q, k, bound))
        # the committed figure must describe these inputs: torch's fp32 route, measured again here, may differ from it by
        # another reduction order of another torch build (a quarter of the figure, half a unit at least), not by more
        fresh = _bounds[family][q]["torch_fp32"]
        if not t <= fresh + max(0.5, 0.25 * fresh):
            bad.append((q, "torch fp32 route measured %.3f, the file says %.3f" % (t, fresh)))
    assert not bad, (family, bad)


def _filled(n):
    """n floats of a NaN pattern followed by TAIL sentinel floats; returns (float view of the n, int32 view of all)"""
    bits = torch.full((n + TAIL,), NAN_BITS, dtype=torch.int32, device=_dev())
    bits[n:] = TAIL_BITS
    return bits.view(torch.float32)[:n], bits


def _tail_kept(bits, n):
    return bool((bits[n:] == TAIL_BITS).all())


def _untouched(bits, n):
    return bool((bits[:n] == NAN_BITS).all()) and _tail_kept(bits, n)


# ------------------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------------------
def _place(x, layout):
    """the (B, T, V) float32 array on the device as a view with the layout's strides; returns (view, leaf it is a view of)"""
    B, T, V = x.shape
    if layout == "batch_major":
        leaf = torch.from_numpy(x).to(_dev())
        return leaf, leaf
    if layout == "time_major":
        leaf = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(_dev())
        return leaf.transpose(0, 1), leaf
    W = O.slice_width(V)
    leaf = torch.full((B, T, W), float("nan"), device=_dev())          # a read past column V would poison the row
    leaf[:, :, :V] = torch.from_numpy(x).to(_dev())
    return leaf[:, :, :V], leaf


def _xe_abi(scores, caps, live, dloss=DLOSS, T_arg=None, ld_grad=None, skip_fwd=False):
    """set_xe_loss_f32 then set_xe_loss_bwd_f32 into pre-filled buffers with sentinel tails"""
    lib = _lib()
    B, T, V = scores.shape
    T = T_arg or T
    V4 = (V + 3) & ~3
    tg = caps[:, 1:]
    assert tg.stride(0) == caps.shape[1] and tg.storage_offset() == 1          # a strided view, as the training loop passes it
    o = dict(B=B, T=T, V=V, V4=V4)
    o["rowloss"], o["rowloss_bits"] = _filled(T * B)
    o["lse"], o["lse_bits"] = _filled(2 * T * B)
    o["sum"], o["sum_bits"] = _filled(1)
    o["grad"], o["grad_bits"] = _filled(T * B * V4)
    live_c = (C.c_int * len(live))(*live)
    d = torch.tensor([dloss], dtype=torch.float32, device=_dev())
    args = (scores.data_ptr(), scores.stride(0), scores.stride(1), tg.data_ptr(), tg.stride(0), tg.stride(1), live_c, B, T, V)
    o["rc_fwd"] = None if skip_fwd else lib.set_xe_loss_f32(*args, o["rowloss"].data_ptr(), o["lse"].data_ptr(), o["sum"].data_ptr(), _stream())
    lse_in = o["lse"]
    if skip_fwd or o["rc_fwd"] != SET_OK:
        lse_in = torch.zeros(2 * T * B, device=_dev())
    o["rc_bwd"] = lib.set_xe_loss_bwd_f32(*args, lse_in.data_ptr(), d.data_ptr(), o["grad"].data_ptr(), V4 if ld_grad is None else ld_grad,
                                          _stream())
    torch.cuda.synchronize()
    return o


def _xe_contract(o, live):
    """bit-exact: padding columns and dead rows are 0, the sentinel tails keep their bits"""
    B, T, V, V4 = o["B"], o["T"], o["V"], o["V4"]
    n = T * B
    assert o["rc_fwd"] == SET_OK and o["rc_bwd"] == SET_OK
    assert _tail_kept(o["rowloss_bits"], n) and _tail_kept(o["lse_bits"], 2 * n) and _tail_kept(o["sum_bits"], 1)
    assert _tail_kept(o["grad_bits"], n * V4)
    g = o["grad_bits"][:n * V4].view(T, B, V4).cpu().numpy()
    assert not g[:, :, V:].any(), "padding columns"
    dead = np.arange(B)[None, :] >= np.array(live)[:, None]
    assert not g[dead].any(), "dead rows of the gradient"
    assert not o["rowloss_bits"][:n].view(T, B).cpu().numpy()[dead].any()
    lse = o["lse_bits"][:2 * n].view(2, T, B).cpu().numpy()
    assert not lse[0][dead].any() and not lse[1][dead].any()


def _xe_torch(x, caps, live, dloss):
    """torch's fp32 route on the device: F.cross_entropy per row, logsumexp, autograd; dead rows masked out"""
    B, T, V = x.shape
    leaf = torch.from_numpy(x).to(_dev()).requires_grad_(True)
    tg = torch.from_numpy(np.ascontiguousarray(caps[:, 1:])).to(_dev())
    mask = torch.from_numpy((np.arange(B)[:, None] < np.array(live)[None, :]).astype(np.float32)).to(_dev())   # (B, T)
    rows = F.cross_entropy(leaf.reshape(B * T, V), tg.reshape(-1), reduction="none").reshape(B, T) * mask
    total = rows.sum()
    (total * dloss).backward()
    lse = torch.logsumexp(leaf.detach(), 2) * mask
    return (rows.detach().t().cpu().numpy(), lse.t().cpu().numpy(), float(total.detach()),
            leaf.grad.transpose(0, 1).cpu().numpy())


def _sum_units(got, ref, x):
    return abs(float(got) - ref) / (O.UNIT * max(1.0, abs(ref), float(np.abs(x[np.isfinite(x)]).max())))


def _xe_errors(x, caps, lens, layout, module=True):
    """runs the ABI (twice) and the module path on one input; returns {quantity: (kernel, torch)} after the bit-exact checks"""
    B, T, V = x.shape
    live = O.live_of(lens, T)
    loss, lse, grad = O.xe_rows(x, caps[:, 1:], live)
    xt = x.transpose(1, 0, 2)
    scores, leaf = _place(x, layout)
    caps_d = torch.from_numpy(caps).to(_dev())
    o = _xe_abi(scores, caps_d, live)
    _xe_contract(o, live)
    again = _xe_abi(scores, caps_d, live)
    for k in ("rowloss_bits", "lse_bits", "sum_bits", "grad_bits"):
        assert torch.equal(o[k], again[k]), "two calls, two results: " + k
    n = T * B
    k_loss = o["rowloss"].view(T, B).cpu().numpy()
    k_lse = o["lse"][:n].view(T, B).cpu().numpy()
    k_lse2 = k_lse.astype(np.float64) + o["lse"][n:].view(T, B).cpu().numpy().astype(np.float64)
    k_grad = o["grad"].view(T, B, o["V4"])[:, :, :V].cpu().numpy()
    k_sum = float(o["sum"][0])
    t_loss, t_lse, t_sum, t_grad = _xe_torch(x, caps, live, DLOSS)
    ref_sum = float(loss.sum())
    e = {"loss": (O.row_units(k_loss, loss, xt), O.row_units(t_loss, loss, xt)),
         # the fp32 lse, and lse + remainder (held to the same bound: it must be at least as good)
         "lse": (max(O.row_units(k_lse, lse, xt), O.row_units(k_lse2, lse, xt)), O.row_units(t_lse, lse, xt)),
         "grad": (O.grad_units(k_grad, grad, DLOSS), O.grad_units(t_grad, grad, DLOSS)),
         "loss_sum": (_sum_units(k_sum, ref_sum, x), _sum_units(t_sum, ref_sum, x))}
    if module:
        from show_edit_tell_amd.train import xe_loss_sum
        leaf.requires_grad_(True)
        sc = {"batch_major": leaf, "time_major": leaf.transpose(0, 1), "slice": leaf[:, :, :V]}[layout]
        ls, ntok, packed, _ = xe_loss_sum(sc, caps_d, lens)
        assert packed is None and ntok == sum(lens)                            # the library's kernels ran, nothing was packed
        (ls * DLOSS).backward()
        mg = leaf.grad.transpose(0, 1) if layout != "time_major" else leaf.grad
        if layout == "slice":
            assert not mg[:, :, V:].contiguous().view(torch.int32).any()       # columns outside the slice: exact zeros
        mg = mg[:, :, :V].cpu().numpy()
        e["grad"] = (max(e["grad"][0], O.grad_units(mg, grad, DLOSS)), e["grad"][1])
        e["loss_sum"] = (max(e["loss_sum"][0], _sum_units(float(ls.detach()), ref_sum, x)), e["loss_sum"][1])
    return e, dict(loss=loss, lse=lse, grad=grad, k_loss=k_loss, k_grad=k_grad, k_lse=k_lse)


def _case_xe_shape(i):
    B, T, V, layout, kind = O.XE_SHAPES[i]
    x, caps = O.xe_family("randn3", B, T, V)
    return "xe_shapes", _xe_errors(x, caps, O.xe_lengths(kind, B, T), layout)[0]


def _case_xe_family(name, V):
    B, T = O.XE_FAMILY_B, O.XE_FAMILY_T
    x, caps = O.xe_family(name, B, T, V)
    e, d = _xe_errors(x, caps, [T] * B, "batch_major")
    if name == "equal":
        assert np.abs(d["loss"] - np.log(V)).max() < 1e-12
    if name == "neg_inf":
        hole = np.isneginf(x.transpose(1, 0, 2))
        assert hole.any() and not d["k_grad"][hole].any(), "gradient at a -inf score"
        assert np.isfinite(d["k_loss"]).all() and not np.isnan(d["k_grad"]).any() and np.isfinite(d["k_lse"]).all()
    return "xe_" + name, e


def _case_xe_t65():
    from show_edit_tell_amd.train import xe_loss_sum
    B, T, V = 2, O.XE_MAX_T + 1, 7
    lens = [T, 40]
    x, caps = O.xe_family("randn3", B, T, V)
    live = O.live_of(lens, T)
    loss, lse, grad = O.xe_rows(x, caps[:, 1:], live)
    leaf = torch.from_numpy(x).to(_dev()).requires_grad_(True)
    ls, ntok, packed, _ = xe_loss_sum(leaf, torch.from_numpy(caps).to(_dev()), lens)
    assert packed is not None and ntok == sum(lens)                            # past XE_MAX_T: the torch calls
    (ls * DLOSS).backward()
    g = O.grad_units(leaf.grad.transpose(0, 1).cpu().numpy(), grad, DLOSS)
    s = _sum_units(float(ls.detach()), float(loss.sum()), x)
    # the second figure is measured as for every other family: the per-row torch route, not the module's own result
    _, _, t_sum, t_grad = _xe_torch(x, caps, live, DLOSS)
    return "xe_t65_torch_path", {"grad": (g, O.grad_units(t_grad, grad, DLOSS)),
                                 "loss_sum": (s, _sum_units(t_sum, float(loss.sum()), x))}


def _case_xe_bad_target():
    """two targets outside [0, V): NaN exactly where the oracle has it (anywhere else counts as an infinite error), the
    other rows as accurate as ever.  torch raises on such a target, so its figure is taken on the same scores with the two
    targets replaced by word 0 and their rows left out."""
    B, T, V = 3, 2, 65
    x, caps = O.xe_family("randn3", B, T, V)
    good = caps.copy()
    caps[1, 1], caps[2, 2] = V, -1
    good[1, 1], good[2, 2] = 0, 0
    live = [B] * T
    loss, lse, grad = O.xe_rows(x, caps[:, 1:], live)
    o = _xe_abi(torch.from_numpy(x).to(_dev()), torch.from_numpy(caps).to(_dev()), live)
    _xe_contract(o, live)
    xt = x.transpose(1, 0, 2)
    bad = np.isnan(loss)
    assert bad.sum() == 2 and np.isnan(float(o["sum"][0]))
    t_loss, _, _, t_grad = _xe_torch(x, good, live, DLOSS)
    t_loss[bad], t_grad[bad] = np.nan, np.nan
    return "xe_bad_target", {"loss": (O.row_units(o["rowloss"].view(T, B).cpu().numpy(), loss, xt), O.row_units(t_loss, loss, xt)),
                             "grad": (O.grad_units(o["grad"].view(T, B, o["V4"])[:, :, :V].cpu().numpy(), grad, DLOSS),
                                      O.grad_units(t_grad, grad, DLOSS))}


@pytest.mark.parametrize("i", range(len(O.XE_SHAPES)), ids=["B%d_T%d_V%d_%s_%s" % s for s in O.XE_SHAPES])
def test_xe_shapes_strides_and_lengths(i):
    _hold(*_case_xe_shape(i))


@pytest.mark.parametrize("V", O.XE_FAMILY_VS)
@pytest.mark.parametrize("name", O.XE_FAMILIES)
def test_xe_row_families(name, V):
    _hold(*_case_xe_family(name, V))


def test_xe_beyond_64_timesteps_takes_the_torch_path_and_matches():
    _hold(*_case_xe_t65())


def test_xe_dloss_scales_the_gradient_and_zero_gives_zero():
    B, T, V = 3, 2, 257
    x, caps = O.xe_family("randn3", B, T, V)
    scores, caps_d = torch.from_numpy(x).to(_dev()), torch.from_numpy(caps).to(_dev())
    one, z = _xe_abi(scores, caps_d, [B] * T, dloss=1.0), _xe_abi(scores, caps_d, [B] * T, dloss=0.0)
    s = _xe_abi(scores, caps_d, [B] * T, dloss=DLOSS)
    assert not (z["grad"].cpu().numpy() != 0).any()
    g1, gs = one["grad"].cpu().numpy(), s["grad"].cpu().numpy()
    assert np.array_equal(gs, g1 * np.float32(DLOSS))                          # one rounding: the product with dloss


def test_xe_out_of_range_target_is_nan_in_its_row_only():
    _hold(*_case_xe_bad_target())


def test_xe_refusals_leave_the_outputs_untouched():
    B, V = 3, 5
    for what, T, live, ld, rc_f, rc_b in (
            ("T = 65", 65, [B] * 65, None, SET_ERR_UNSUPPORTED, SET_ERR_UNSUPPORTED),
            ("ld_grad", 4, [3, 3, 2, 1], V, SET_OK, SET_ERR_ARG),
            ("ld_grad rounded to 8", 4, [3, 3, 2, 1], 12, SET_OK, SET_ERR_ARG),
            ("live increases", 4, [3, 2, 3, 1], None, SET_ERR_ARG, SET_ERR_ARG),
            ("live above B", 4, [4, 3, 2, 1], None, SET_ERR_ARG, SET_ERR_ARG),
            ("live below 0", 4, [3, 2, 1, -1], None, SET_ERR_ARG, SET_ERR_ARG)):
        x, caps = O.xe_family("randn3", B, T, V)
        o = _xe_abi(torch.from_numpy(x).to(_dev()), torch.from_numpy(caps).to(_dev()), live, ld_grad=ld)
        assert (o["rc_fwd"], o["rc_bwd"]) == (rc_f, rc_b), (what, o["rc_fwd"], o["rc_bwd"])
        n = T * B
        assert _untouched(o["grad_bits"], n * o["V4"]), what
        if rc_f != SET_OK:
            assert _untouched(o["rowloss_bits"], n) and _untouched(o["lse_bits"], 2 * n) and _untouched(o["sum_bits"], 1), what
        # the backward alone (no forward before it) refuses the same tables
        o = _xe_abi(torch.from_numpy(x).to(_dev()), torch.from_numpy(caps).to(_dev()), live, ld_grad=ld, skip_fwd=True)
        assert o["rc_bwd"] == rc_b and _untouched(o["grad_bits"], n * o["V4"]), what


# ------------------------------------------------------------------------------------------------
# MSE
# ------------------------------------------------------------------------------------------------
def _mse_torch(a, b):
    ta, tb = (torch.from_numpy(v).to(_dev()).requires_grad_(True) for v in (a, b))
    s = ((ta - tb) ** 2).sum()
    s.backward()
    return float(s.detach()), ta.grad.cpu().numpy(), tb.grad.cpu().numpy()


def _case_mse(n, offset=0):
    """autograd_ops.mse_sum on views that start `offset` floats into their storage"""
    from show_edit_tell_amd.autograd_ops import mse_sum
    a, b = O.mse_inputs(n)
    ref = O.mse(a, b)
    bufs = [torch.zeros(n + offset, device=_dev()) for _ in range(2)]
    leaves = []
    for buf, v in zip(bufs, (a, b)):
        buf[offset:] = torch.from_numpy(v).to(_dev())
        leaves.append(buf.requires_grad_(True))
    out = []
    for _ in range(2):
        for l in leaves:
            l.grad = None
        s = mse_sum(leaves[0][offset:], leaves[1][offset:])
        s.backward()
        out.append((s.detach().clone(), leaves[0].grad[offset:].clone(), leaves[1].grad[offset:].clone()))
        assert leaves[0][offset:].data_ptr() % 16 == (4 * offset) % 16
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*out)), "two calls, two results"
    k = (float(out[0][0]), out[0][1].cpu().numpy(), out[0][2].cpu().numpy())
    t = _mse_torch(a, b)
    return "mse", {q: (O.tensor_units(k[j], ref[j]), O.tensor_units(t[j], ref[j])) for j, q in enumerate(("sum", "da", "db"))}


def _mse_abi(a, b, n, scale, dout, want_da, want_db, n_arg=None):
    lib = _lib()
    da, da_bits = _filled(n)
    db, db_bits = _filled(n)
    rc = lib.set_mse_bwd_f32(a.data_ptr(), b.data_ptr(), n if n_arg is None else n_arg, scale, None if dout is None else dout.data_ptr(),
                             da.data_ptr() if want_da else None, db.data_ptr() if want_db else None, _stream())
    torch.cuda.synchronize()
    return rc, da, da_bits, db, db_bits


def _case_mse_variants(n):
    """set_mse_bwd_f32 directly: da only, db only, dout = NULL with scale, dout given"""
    a, b = O.mse_inputs(n, seed=1)
    ref = O.mse(a, b)
    ad, bd = torch.from_numpy(a).to(_dev()), torch.from_numpy(b).to(_dev())
    dout = torch.tensor([0.75], device=_dev())
    t = _mse_torch(a, b)
    errs = {"da": (0.0, O.tensor_units(t[1], ref[1])), "db": (0.0, O.tensor_units(t[2], ref[2]))}
    for want_da, want_db, scale, d, factor in ((True, False, 2.0, None, 1.0), (False, True, 2.0, None, 1.0), (True, True, 0.5, None, 0.25),
                                               (True, True, 2.0, dout, 0.75), (False, True, 4.0, dout, 1.5)):
        rc, da, da_bits, db, db_bits = _mse_abi(ad, bd, n, scale, d, want_da, want_db)
        assert rc == SET_OK
        assert _tail_kept(da_bits, n) and _tail_kept(db_bits, n)
        for want, out, bits, j, q in ((want_da, da, da_bits, 1, "da"), (want_db, db, db_bits, 2, "db")):
            if not want:
                assert _untouched(bits, n), "an output that was not asked for"
            else:
                errs[q] = (max(errs[q][0], O.tensor_units(out.cpu().numpy(), ref[j] * factor) ), errs[q][1])
        if want_da and want_db:
            assert torch.equal(db, -da)
    return "mse", errs


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", O.MSE_SIZES)
def test_mse_sum_and_gradients(n, offset):
    _hold(*_case_mse(n, offset))


@pytest.mark.parametrize("n", [5, 4099, O.MSE_GRID_LIMIT + 5])
def test_mse_backward_variants(n):
    _hold(*_case_mse_variants(n))


def test_mse_refusals_leave_the_outputs_untouched():
    lib = _lib()
    n = 65
    a, b = (torch.from_numpy(v).to(_dev()) for v in O.mse_inputs(n))
    rc, da, da_bits, db, db_bits = _mse_abi(a, b, n, 2.0, None, False, False)           # both outputs NULL
    assert rc == SET_ERR_ARG and _untouched(da_bits, n) and _untouched(db_bits, n)
    rc, da, da_bits, db, db_bits = _mse_abi(a, b, n, 2.0, None, True, True, n_arg=0)
    assert rc == SET_ERR_ARG and _untouched(da_bits, n) and _untouched(db_bits, n)
    out, out_bits = _filled(1)
    assert lib.set_mse_sum_f32(a.data_ptr(), b.data_ptr(), 0, out.data_ptr(), _stream()) == SET_ERR_ARG
    assert lib.set_mse_sum_f32(a.data_ptr(), None, n, out.data_ptr(), _stream()) == SET_ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(out_bits, 1)


# ------------------------------------------------------------------------------------------------
# clip + Adam
# ------------------------------------------------------------------------------------------------
def _adam_setup(case, kernel_layout):
    """parameters, optimizer and a setter of the step's gradients.  kernel_layout: the case's special gradient placement
    (flat bucket views, a misaligned gradient) — the torch route gets plain tensors"""
    sizes = O.ADAM_CASES[case]["sizes"]
    ps = [torch.nn.Parameter(torch.from_numpy(v).to(_dev())) for v in O.adam_params(case)]
    groups = [dict({k: v for k, v in g.items() if k != "params"}, params=[ps[i] for i in g["params"]]) for g in O.adam_groups(case)]
    opt = torch.optim.Adam(groups)
    if case == "late":
        for p, s in zip(ps, O.adam_state(case)):
            opt.state[p] = dict(step=torch.tensor(float(s["step"])), exp_avg=torch.from_numpy(s["m"]).to(_dev()),
                                exp_avg_sq=torch.from_numpy(s["v"]).to(_dev()))
    views = None
    if kernel_layout and case == "flat":                   # 64-float aligned views at non-zero offsets of one flat buffer
        offs, off = [], 64
        for n in sizes:
            offs.append(off)
            off += (n + 63) // 64 * 64
        flat = torch.zeros(off, device=_dev())
        views = [flat[o:o + n] for o, n in zip(offs, sizes)]
        assert all(v.storage_offset() > 0 and v.storage_offset() % 64 == 0 and v.data_ptr() % 16 == 0 for v in views)
    if kernel_layout and case == "misaligned":             # the first gradient starts 4 bytes off a 16-byte boundary
        views = [torch.zeros(sizes[0] + 1, device=_dev())[1:]] + [torch.zeros(n, device=_dev()) for n in sizes[1:]]
        assert views[0].data_ptr() % 16 == 4

    def set_grads(gs):
        for i, (p, g) in enumerate(zip(ps, gs)):
            if views is None:
                p.grad = torch.from_numpy(g).to(_dev())
            else:
                views[i].copy_(torch.from_numpy(g))
                p.grad = views[i]
    return ps, opt, set_grads


def _adam_route(case, max_norm, scale_grads, kernel, nan_at=None):
    """four steps on one route; returns per step (p, m, v, norm, grads after the step) as numpy"""
    from show_edit_tell_amd import optim
    ps, opt, set_grads = _adam_setup(case, kernel)
    steps = []
    for it in range(O.ADAM_STEPS if nan_at is None else 1):
        gs = O.adam_grads(case, it)
        if nan_at is not None:
            gs[nan_at[0]][nan_at[1]] = np.nan
        set_grads(gs)
        if kernel:
            epoch = optim.weights_epoch()
            norm = optim.clip_grad_norm_and_step(ps, opt, max_norm, scale_grads=scale_grads)
            # the fused launch counts a weight update; the torch calls (misaligned gradient) do not
            assert optim.weights_epoch() - epoch == (0 if case == "misaligned" else 1)
        else:
            norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
        torch.cuda.synchronize()
        steps.append(dict(p=[p.detach().cpu().numpy() for p in ps], m=[opt.state[p]["exp_avg"].cpu().numpy() for p in ps],
                          v=[opt.state[p]["exp_avg_sq"].cpu().numpy() for p in ps], norm=float(norm),
                          g=[p.grad.cpu().numpy() for p in ps], g_in=gs, step=[int(opt.state[p]["step"]) for p in ps]))
    return steps


def _case_adam(case, max_norm, scale_grads):
    c = O.ADAM_CASES[case]
    groups = O.adam_groups(case)
    k_steps = _adam_route(case, max_norm, scale_grads, True)
    t_steps = _adam_route(case, max_norm, True, False)
    p, st = O.adam_params(case), O.adam_state(case)
    p0 = [v.copy() for v in p]
    errs = {q: (0.0, 0.0) for q in ("p", "m", "v", "norm", "grad")}

    def up(q, k, t):
        errs[q] = (max(errs[q][0], k), max(errs[q][1], t))
    for it in range(O.ADAM_STEPS):
        p, st, total, clipped = O.clip_adam(p, O.adam_grads(case, it), st, groups, max_norm)
        ks, ts = k_steps[it], t_steps[it]
        up("norm", O.tensor_units(ks["norm"], total), O.tensor_units(ts["norm"], total))
        for i in range(len(p)):
            assert ks["step"][i] == st[i]["step"]
            up("p", O.tensor_units(ks["p"][i], p[i]), O.tensor_units(ts["p"][i], p[i]))
            up("m", O.tensor_units(ks["m"][i], st[i]["m"]), O.tensor_units(ts["m"][i], st[i]["m"]))
            up("v", O.tensor_units(ks["v"][i], st[i]["v"]), O.tensor_units(ts["v"][i], st[i]["v"]))
            if scale_grads or case == "misaligned":
                up("grad", O.tensor_units(ks["g"][i], clipped[i]), O.tensor_units(ts["g"][i], clipped[i]))
            else:                                          # scale_grads = False leaves .grad as it was, bit for bit
                assert np.array_equal(ks["g"][i].view(np.uint32), ks["g_in"][i].view(np.uint32))
                up("grad", 0.0, O.tensor_units(ts["g"][i], clipped[i]))
        z = c["zero_grad"]
        if z is not None:                                  # zero gradient on zero state, weight_decay = 0: nothing moves
            assert np.array_equal(ks["p"][z].view(np.uint32), p0[z].view(np.uint32))
            assert not ks["m"][z].view(np.uint32).any() and not ks["v"][z].view(np.uint32).any()
    assert (max(s["norm"] for s in k_steps) > max_norm) == (max_norm < 1)     # 0.25 clips, 1e9 never does
    return "adam_%s_%g" % (case, max_norm), errs


@pytest.mark.parametrize("scale_grads", [False, True])
@pytest.mark.parametrize("max_norm", O.ADAM_MAX_NORMS)
@pytest.mark.parametrize("case", ["edges", "table40", "table41", "flat", "late"])
def test_clip_adam_four_steps(case, max_norm, scale_grads):
    _hold(*_case_adam(case, max_norm, scale_grads))


def test_clip_adam_with_a_misaligned_gradient_takes_the_torch_calls_and_matches():
    _hold(*_case_adam("misaligned", 0.25, True))


@pytest.mark.parametrize("scale_grads", [False, True])
def test_clip_adam_nan_gradient_poisons_every_parameter(scale_grads):
    k = _adam_route("nan", 0.25, scale_grads, True, nan_at=(1, 7))[0]
    t = _adam_route("nan", 0.25, True, False, nan_at=(1, 7))[0]
    assert np.isnan(k["norm"]) and np.isnan(t["norm"])
    for i in range(len(k["p"])):
        assert np.isnan(k["p"][i]).all() and np.isnan(t["p"][i]).all()


def _adam_abi(n_tensors=2, numel=(5, 300), step=1, beta1=0.9, eps=1e-8, misalign=False, ws_short=False, n_arg=None):
    lib = _lib()
    bufs = []                                              # per tensor: (p, g, m, v) pre-filled, with their bit views
    for n in numel:
        bufs.append([_filled(n + 4) for _ in range(4)])
    P, G, M, V = ((C.c_void_p * n_tensors)() for _ in range(4))
    for i in range(n_tensors):
        ptrs = [f.data_ptr() for f, _ in bufs[i]]
        if misalign and i == 1:
            ptrs[1] += 4
        P[i], G[i], M[i], V[i] = ptrs
    nel = (C.c_int64 * n_tensors)(*numel)
    stp = (C.c_int64 * n_tensors)(*([1] * (n_tensors - 1) + [step]))
    dbl = lambda v: (C.c_double * n_tensors)(*([v] * n_tensors))
    b1 = (C.c_double * n_tensors)(*([0.9] * (n_tensors - 1) + [beta1]))
    ep = (C.c_double * n_tensors)(*([1e-8] * (n_tensors - 1) + [eps]))
    need = lib.set_clip_adam_workspace_bytes(n_tensors, nel)
    chunks = sum((n + O.OPT_CHUNK - 1) // O.OPT_CHUNK for n in numel)
    assert need >= 4 * chunks
    ws_bytes = 4 * chunks - 4 if ws_short else need
    ws, ws_bits = _filled(need // 4 + 1)
    norm, norm_bits = _filled(1)
    rc = lib.set_clip_adam_f32(n_tensors if n_arg is None else n_arg, P, G, M, V, nel, stp, dbl(1e-3), b1, dbl(0.999), ep, dbl(0.0), 0.25, 1,
                               norm.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    torch.cuda.synchronize()
    clean = _untouched(norm_bits, 1) and _untouched(ws_bits, need // 4 + 1) and all(_untouched(b, n + 4) for i, n in enumerate(numel) for _, b in bufs[i])
    return rc, clean


def test_clip_adam_refusals_leave_parameters_and_state_untouched():
    for what, kw, want in (("step = 0", dict(step=0), SET_ERR_ARG), ("beta1 = 1", dict(beta1=1.0), SET_ERR_ARG),
                           ("negative eps", dict(eps=-1e-8), SET_ERR_ARG), ("NaN eps", dict(eps=float("nan")), SET_ERR_ARG),
                           ("misaligned pointer", dict(misalign=True), SET_ERR_UNSUPPORTED),
                           ("workspace one float short", dict(ws_short=True), SET_ERR_WORKSPACE),
                           ("n = 0", dict(n_arg=0), SET_ERR_ARG)):
        rc, clean = _adam_abi(**kw)
        assert rc == want and clean, (what, rc, clean)


# ------------------------------------------------------------------------------------------------
# the measured figures: python tests/test_hip_train_tail.py OUT.json
# ------------------------------------------------------------------------------------------------
def _all_cases():
    for i in range(len(O.XE_SHAPES)):
        yield _case_xe_shape(i)
    for name in O.XE_FAMILIES:
        for V in O.XE_FAMILY_VS:
            yield _case_xe_family(name, V)
    yield _case_xe_t65()
    yield _case_xe_bad_target()
    for n in O.MSE_SIZES:
        for offset in (0, 1):
            yield _case_mse(n, offset)
    for n in (5, 4099, O.MSE_GRID_LIMIT + 5):
        yield _case_mse_variants(n)
    for case in ("edges", "table40", "table41", "flat", "late"):
        for max_norm in O.ADAM_MAX_NORMS:
            for scale_grads in (False, True):
                yield _case_adam(case, max_norm, scale_grads)
    yield _case_adam("misaligned", 0.25, True)


if __name__ == "__main__":
    fam = {}
    for family, errs in _all_cases():
        for q, (k, t) in errs.items():
            d = fam.setdefault(family, {}).setdefault(q, {"kernel": 0.0, "torch_fp32": 0.0})
            d["kernel"], d["torch_fp32"] = max(d["kernel"], k), max(d["torch_fp32"], t)
    worst = {}
    for family, qs in fam.items():
        for q, d in qs.items():
            d["bound"] = 2.0 * d["torch_fp32"] + 2.0
            d["kernel_over_torch_fp32"] = d["kernel"] / d["torch_fp32"] if d["torch_fp32"] > 0 else None
            group = family.split("_")[0]
            w = worst.setdefault(group, {"kernel_over_bound": 0.0, "kernel_over_torch_fp32": 0.0})
            w["kernel_over_bound"] = max(w["kernel_over_bound"], d["kernel"] / d["bound"])
            w["kernel_over_torch_fp32"] = max(w["kernel_over_torch_fp32"], d["kernel_over_torch_fp32"] or 0.0)
    doc = {"what": "largest error against the float64 oracle (tests/train_tail_oracle.py) per case family, in units of 2^-24 x the "
                   "quantity's scale (see tests/test_hip_train_tail.py): the library's kernels and torch's fp32 route on the same "
                   "inputs; the tests bound the kernel by 2 x torch_fp32 + 2",
           "worst_ratios": worst, "families": fam}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for family in sorted(fam):
        for q, d in sorted(fam[family].items()):
            print("%-28s %-9s kernel %10.3f  torch fp32 %10.3f  %s" % (family, q, d["kernel"], d["torch_fp32"],
                                                                        "" if d["kernel"] <= d["bound"] else "ABOVE THE BOUND"))
