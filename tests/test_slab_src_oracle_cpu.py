"""CPU: tests/slab_src_oracle.py is pinned before it judges a kernel.  Every float64 closed form equals torch autograd on
the operator's forward written in torch (the forwards of tests/test_hip_backward_ops.py, oracle/editnet_torch.py and
oracle/xe_grad_torch.py) to 1e-12 of the largest entry; the ordered fp32 sum equals the float64 sum to fp32 rounding on
random data and exactly where every addition is exact."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import slab_src_oracle as SO
from oracle import editnet_torch as ET, philox_np as PH, xe_grad_torch as XG

REL = 1e-12


def rnd(gen, *shape, scale=1.0):
    return (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * scale


def leaf(gen, *shape, scale=1.0):
    return rnd(gen, *shape, scale=scale).requires_grad_(True)


def same(named):
    for name, got, ref in named:
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        assert scale > 0 and err <= REL * scale, (name, err, scale)


@pytest.mark.parametrize("M,D", [(1, 4), (5, 8), (7, 260)])
@pytest.mark.parametrize("with_dc", [False, True])
def test_lstm_cell_closed_form(M, D, with_dc):
    gen = torch.Generator().manual_seed(M + D)
    z, c = leaf(gen, M, 4 * D, scale=2.0), leaf(gen, M, D)
    eye, zero = torch.eye(4 * D, dtype=torch.float64), torch.zeros(4 * D, dtype=torch.float64)
    P = {"l.weight_ih": eye, "l.bias_ih": zero, "l.weight_hh": torch.zeros(4 * D, D, dtype=torch.float64), "l.bias_hh": zero}
    hn, cn = XG._nn_lstm_cell(P, "l", z, torch.zeros(M, D, dtype=torch.float64), c)
    dh, dc = rnd(gen, M, D), rnd(gen, M, D)
    if with_dc:
        torch.autograd.backward([hn, cn], [dh, dc])
    else:
        hn.backward(dh)
    i, f, g, o = z.detach().chunk(4, 1)
    gates = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], 1)
    dgates, dcp = SO.lstm_cell_bwd(dh, dc if with_dc else None, gates, c.detach(), cn.detach())
    same([("dgates", dgates, z.grad), ("dc_prev", dcp, c.grad)])


@pytest.mark.parametrize("M,D", [(1, 4), (5, 8), (7, 260)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_copy_gate_and_lstm_gates_closed_forms(M, D, p):
    """CopyLSTMCellC through oracle/editnet_torch.py with its output behind a Philox dropout: stage 1 (copy gate), the host's
    dcn = dcn_direct + du W_cnew, stage 2 (LSTM gates) reproduce autograd's gradients of every input"""
    gen = torch.Generator().manual_seed(10 * M + D)
    z, c, sel = leaf(gen, M, 4 * D, scale=2.0), leaf(gen, M, D), leaf(gen, M, D)
    Wn, Wm, bn = rnd(gen, D, D, scale=2 / math.sqrt(D)), rnd(gen, D, D, scale=2 / math.sqrt(D)), rnd(gen, D)
    zero = torch.zeros(4 * D, dtype=torch.float64)
    P = {"copy_lstm.x2h.weight": torch.eye(4 * D, dtype=torch.float64), "copy_lstm.x2h.bias": zero,
         "copy_lstm.h2h.weight": torch.zeros(4 * D, D, dtype=torch.float64), "copy_lstm.h2h.bias": zero,
         "copy_lstm.gate_cnew.weight": Wn, "copy_lstm.gate_cnew.bias": bn, "copy_lstm.gate_cmem.weight": Wm,
         "copy_lstm.gate_cmem.bias": torch.zeros(D, dtype=torch.float64)}
    h, mem = ET.copy_lstm(P, z, torch.zeros(M, D, dtype=torch.float64), c, sel)
    seed, off = 0x1_2345_6789, PH.site_offset(PH.SITE_OUT, 3)
    keep = PH.dropout_keep(seed, off, M, D, p) if p > 0 else None
    dh_a, dh_drop, dadp = rnd(gen, M, D), rnd(gen, M, D), rnd(gen, M, D)
    dropped = h if keep is None else h * torch.from_numpy(np.ascontiguousarray(keep)).double() / (1 - p)
    torch.autograd.backward([h, dropped, mem], [dh_a, dh_drop, dadp])
    # the saved tensors of the train-mode forward
    i, f, g, o = z.detach().chunk(4, 1)
    gates = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], 1)
    cn = gates[:, D:2 * D] * c.detach() + gates[:, :D] * gates[:, 2 * D:3 * D]
    cg = torch.sigmoid(F.linear(cn, Wn, bn) + F.linear(sel.detach(), Wm))
    dh = dh_a + SO.dropout_bwd(dh_drop, seed, off, p)
    du, dcm, dcn_d, dop = SO.copy_gate_bwd(dh, dadp, gates[:, 3 * D:], mem.detach(), cg, sel.detach(), cn)
    dgates, dcp = SO.lstm_gates_bwd(dcn_d + du @ Wn, dop, gates, c.detach())
    same([("dgates", dgates, z.grad), ("dc_prev", dcp, c.grad), ("dsel", dcm + du @ Wm, sel.grad)])
    if p > 0:
        assert 0 < int(keep.sum()) < keep.size or M * D < 8


@pytest.mark.parametrize("M,T,D", [(1, 1, 4), (5, 9, 8), (7, 9, 260)])
@pytest.mark.parametrize("acc", [False, True])
def test_select_closed_form(M, T, D, acc):
    gen = torch.Generator().manual_seed(M + T + D)
    Mem = leaf(gen, M, T, D)
    al = F.softmax(rnd(gen, M, T, scale=3.0), 1).requires_grad_(True)
    dsel = rnd(gen, M, D)
    ET.select_hard(Mem, al).backward(dsel)
    dM0 = rnd(gen, M, T, D) if acc else None
    dM, dal = SO.select_bwd(dsel, Mem.detach(), al.detach(), dM0)
    same([("dM", dM, Mem.grad + (dM0 if acc else 0)), ("dalpha", dal, al.grad)])
    if acc:                                                   # only the selected row changed
        changed = (dM != dM0).any(2)
        assert bool((changed.sum(1) <= 1).all()) and bool((changed.float().argmax(1) == al.detach().argmax(1)).all())


@pytest.mark.parametrize("M,D", [(1, 4), (5, 8), (7, 260)])
def test_context_gate_closed_form(M, D):
    gen = torch.Generator().manual_seed(M * D)
    a, b, c = leaf(gen, M, D, scale=2.0), leaf(gen, M, D, scale=2.0), leaf(gen, M, D, scale=2.0)
    zt, s, t = torch.sigmoid(a), torch.tanh(b), torch.tanh(c)
    dout = rnd(gen, M, D)
    (zt * s + (1 - zt) * t).backward(dout)
    dz, ds, dt = SO.context_gate_bwd(dout, zt.detach(), s.detach(), t.detach())
    same([("dz", dz, a.grad), ("ds", ds, b.grad), ("dt", dt, c.grad)])


@pytest.mark.parametrize("M,L,Dv,A", [(1, 1, 4, 4), (5, 7, 64, 32), (2, 36, 260, 64)])
@pytest.mark.parametrize("tanh", [False, True], ids=["relu", "tanh"])
@pytest.mark.parametrize("ext", [False, True], ids=["no-ext", "dalpha-ext"])
def test_attention_closed_form(M, L, Dv, A, tanh, ext):
    """the forward of tests/test_hip_backward_ops.py::test_attention_backward_kernel"""
    gen = torch.Generator().manual_seed(M + 10 * L + Dv + A)
    V, att1, att2 = rnd(gen, M, L, Dv), leaf(gen, M, L, A, scale=2.0), leaf(gen, M, A, scale=2.0)
    w = leaf(gen, A, scale=4 / math.sqrt(A))
    dctx, dal = rnd(gen, M, Dv), rnd(gen, M, L)
    pre = att1 + att2.unsqueeze(1)
    e = ((torch.tanh(pre) if tanh else torch.relu(pre)) * w).sum(2)
    e.retain_grad()
    alpha = F.softmax(e, 1)
    loss = ((V * alpha.unsqueeze(2)).sum(1) * dctx).sum()
    if ext:
        loss = loss + (alpha * dal).sum()
    loss.backward()
    datt1, datt2, dwf, de = SO.attention_bwd(dctx, dal if ext else None, alpha.detach(), V, att1.detach(), att2.detach(),
                                             w.detach(), tanh)
    named = [("datt1", datt1, att1.grad), ("datt2", datt2, att2.grad), ("dwfull", dwf.sum(0), w.grad)]
    if L > 1:                                                 # (one region: alpha = 1 and every gradient through e is zero)
        same(named + [("de", de, e.grad)])
    else:
        assert all(float(g.abs().max()) <= 1e-15 for _, g, _ in named) and float(de.abs().max()) <= 1e-15


def _entries(gen, M, D, make):
    return [SO.Entry(make(gen, 3, M, D), M, 3), SO.Entry(None, 0, 0), SO.Entry(make(gen, 5, M, D + 4), max(M - 2, 0), 5),
            SO.Entry(make(gen, 1, M, D), 1, 1), SO.Entry(make(gen, 9, M, D), M, 9)]


@pytest.mark.parametrize("M,D", [(1, 4), (5, 8), (70, 260)])
def test_ordered_sum_equals_the_float64_sum_to_fp32_rounding(M, D):
    gen = torch.Generator().manual_seed(M + D)
    ent = _entries(gen, M, D, lambda g, *s: rnd(g, *s).float())
    for base in (None, rnd(gen, M, D).float()):
        got, ref = SO.ordered_sum32(base, ent, M, D), SO.sum64(base, ent, M, D)
        assert got.dtype == torch.float32 and ref.dtype == torch.float64
        # 18 partials and the base, each below 1 in magnitude: every intermediate sum is below 19, and each of the 18 + 5
        # additions rounds by at most 2^-24 of its result
        assert float((got.double() - ref).abs().max()) <= 23 * 19 * 2.0 ** -24
    # rows that have left and empty entries contribute exactly nothing; the padding columns are not read
    r = max(M - 2, 0)
    for fn, dt in ((SO.ordered_sum32, torch.float32), (SO.sum64, torch.float64)):
        got = fn(None, [SO.Entry(ent[2].t, r, 5), SO.Entry(None, 0, 0)], M, D)
        assert float(got[r:].abs().sum()) == 0.0
        assert float((got[:r].double() - ent[2].t[:, :r, :D].double().sum(0)).abs().max() if r else 0.0) <= 5 * 5 * 2.0 ** -24


@pytest.mark.parametrize("M,D", [(1, 4), (5, 8), (70, 260)])
def test_ordered_sum_is_exact_on_small_integers(M, D):
    gen = torch.Generator().manual_seed(M * D)
    ints = lambda g, *s: torch.randint(-64, 65, s, generator=g).float()
    ent = _entries(gen, M, D, ints)
    for base in (None, ints(gen, M, D)):
        assert torch.equal(SO.ordered_sum32(base, ent, M, D).double(), SO.sum64(base, ent, M, D))


def test_ordered_sum_keeps_the_documented_order():
    """1e4 - 1e4 + 1e-3 in slab order is 1e-3; any order that adds 1e-3 to 1e4 first loses most of it.  Between entries the
    same holds in list order."""
    t = torch.tensor([1e4, -1e4, 1e-3]).view(3, 1, 1).expand(3, 2, 4).contiguous()
    assert torch.equal(SO.ordered_sum32(None, [SO.Entry(t, 2, 3)], 2, 4), torch.full((2, 4), 1e-3))
    rev = t.flip(0).contiguous()
    assert not torch.equal(SO.ordered_sum32(None, [SO.Entry(rev, 2, 3)], 2, 4), torch.full((2, 4), 1e-3))
    one = lambda v: SO.Entry(torch.full((1, 2, 4), v), 2, 1)
    assert torch.equal(SO.ordered_sum32(torch.full((2, 4), 1e4), [one(-1e4), one(1e-3)], 2, 4), torch.full((2, 4), 1e-3))
    assert not torch.equal(SO.ordered_sum32(torch.full((2, 4), 1e-3), [one(1e4), one(-1e4)], 2, 4), torch.full((2, 4), 1e-3))
