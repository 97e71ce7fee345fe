"""GPU: every autograd-wrapped operator of show_edit_tell_amd/autograd_ops.py ALONE, with a random upstream gradient,
against the same operator written in float64 torch on the CPU and differentiated by torch autograd — so that a failure
of tests/test_hip_grad_shapes.py names a kernel.  Batch sizes 1, 5, 64, 130 (both sides of the 64- and 128-row switches).

Tolerances, relative to max|ref| of each output gradient: 2e-6 * sqrt(K) * 4 for pure contractions over K (the bound of
test_gemm_general_layouts), 1e-4 for the fused operators (the element criterion of tests/test_hip_train.py::_check_grads).
A gradient that is mathematically zero (softmax shift invariance: d / d full_att.bias) is rounding noise on both sides:
the absolute floor is 1e-6 * the largest max|ref| among the operator's gradients, as in _check_grads.  Inputs whose float64
forward has a hard-select gap below 1e-4 or a ReLU pre-activation within 1e-6 * max(1, |a| + |b|) of zero are refused by
an assertion on the float64 side (seeds are chosen so that none occurs)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import editnet_torch as ET, philox_np as PH, xe_grad_torch as XG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = [1, 5, 64, 130]
FUSED = 1e-4


def ktol(K):
    return 2e-6 * math.sqrt(K) * 4


def rnd(gen, *shape, scale=1.0):
    return (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * scale


def f32(t64):
    """the fp32 value both sides start from: (device fp32 leaf, float64 leaf of the same numbers)"""
    v = t64.float()
    return v.to(DEV).requires_grad_(True), v.double().requires_grad_(True)


def pair(gen, *shape, scale=1.0):
    return f32(rnd(gen, *shape, scale=scale))


def check(named, tol, what):
    """named: [(name, device gradient, float64 gradient, tolerance or None)]"""
    floor = 1e-6 * max(float(r.abs().max()) for _, _, r, _ in named)
    for name, got, ref, t in named:
        assert got is not None, (what, name, "no gradient")
        got = got.detach().double().cpu()
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        lim = (tol if t is None else t) * scale + floor
        assert err <= lim, "%s %s: max err %.3e > %.3e (max|ref| %.3e)" % (what, name, err, lim, scale)


def no_kink(pre, a, b):
    assert not bool((pre.detach().abs() <= 1e-6 * torch.clamp(a.detach().abs() + b.detach().abs(), min=1.0)).any())


def gap_ok(alpha, mask=None):
    top = alpha.detach().topk(2, dim=1).values
    many = torch.ones(alpha.shape[0], dtype=torch.bool) if mask is None else mask.sum(1) > 1
    assert not bool(many.any()) or float((top[:, 0] - top[:, 1])[many].min()) >= 1e-4


def lens_for(B, T, mode):
    if mode == "equal":
        return torch.full((B,), T, dtype=torch.long)
    lens = (torch.arange(B) * 7 % T) + 1
    lens[0] = 1
    lens[-1] = T
    return lens


# ---------------------------------------------------------------------------------------------------------------------
# contractions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("N,K", [(1, 32), (3, 64), (37, 96), (64, 32)])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])
def test_linear(M, N, K, act):
    """N < 4 and N & 3 != 0 (padded contractions of dX, padded rows of dW), the bias gradient on both sides of the
    64-row switch of _colsum"""
    from show_edit_tell_amd import _lib, autograd_ops as A
    gen = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    x, x64 = pair(gen, M, K)
    w, w64 = pair(gen, N, K, scale=1 / math.sqrt(K))
    b, b64 = pair(gen, N)
    dy64 = rnd(gen, M, N)
    pre = F.linear(x64, w64, b64)
    if act == "relu":
        no_kink(pre, F.linear(x64, w64), b64.expand_as(pre))
    (torch.relu(pre) if act == "relu" else pre).backward(dy64)
    y = A.linear(x, w, b, _lib.ACT_RELU if act == "relu" else _lib.ACT_NONE)
    y.backward(dy64.float().to(DEV))
    check([("dx", x.grad, x64.grad, ktol(N)), ("dw", w.grad, w64.grad, ktol(M)), ("db", b.grad, b64.grad, ktol(M))],
          None, "linear M=%d N=%d K=%d %s" % (M, N, K, act))


@pytest.mark.parametrize("M", [1, 64, 129])
def test_linear_with_a_column_slice_weight(M):
    """the weight is a strided column slice of a wider leaf matrix: read in place in the forward and in dX, and the
    wider matrix receives the gradient in the slice's columns only"""
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(M)
    N, K = 37, 32
    x, x64 = pair(gen, M, K)
    W, W64 = pair(gen, N, 3 * K, scale=1 / math.sqrt(K))
    b, b64 = pair(gen, N)
    dy64 = rnd(gen, M, N)
    ref = F.linear(x64, W64[:, K:2 * K], b64)
    ref.backward(dy64)
    y = A.linear(x, W[:, K:2 * K], b)
    assert float((y.detach().double().cpu() - ref.detach()).abs().max()) <= ktol(K) * float(ref.detach().abs().max())
    y.backward(dy64.float().to(DEV))
    check([("dx", x.grad, x64.grad, ktol(N)), ("dW", W.grad, W64.grad, ktol(M)), ("db", b.grad, b64.grad, ktol(M))],
          None, "linear column slice M=%d" % M)


@pytest.mark.parametrize("M", [5, 64, 130])
def test_wgrad_blocks_and_colsum_group(M):
    """_wgrad_blocks: dW assembled from column blocks that contract over different row counts, fresh and accumulating into an
    existing .grad, refusal of a block that does not start on a multiple of 4; _colsum_group: several bias gradients in
    one pair of launches (>= 64 rows, cols % 4 == 0) and its one-by-one path (fewer rows, ragged columns), fresh and
    accumulating"""
    from show_edit_tell_amd import _lib, autograd_ops as A
    gen = torch.Generator().manual_seed(M + 31)
    N, K1, K2, M2 = 64, 32, 64, 7
    dy1, x1, dy2, x2 = rnd(gen, M, N).float(), rnd(gen, M, K1).float(), rnd(gen, M2, N).float(), rnd(gen, M2, K2).float()
    dW = torch.cat([dy1.double().t() @ x1.double(), dy2.double().t() @ x2.double()], 1)
    blocks = [(dy1.to(DEV), x1.to(DEV), 0), (dy2.to(DEV), x2.to(DEV), K1)]
    p = torch.nn.Parameter(torch.zeros(N, K1 + K2, device=DEV))
    assert A._wgrad_blocks(p, blocks) is None
    fresh = p.grad.clone()
    A._wgrad_blocks(p, blocks)
    check([("dW", fresh, dW, None), ("dW acc", p.grad, 2 * dW, None)], ktol(M), "wgrad_blocks M=%d" % M)
    with pytest.raises(_lib.SetError):
        A._wgrad_blocks(p, [(dy1.to(DEV), x1.to(DEV), 2)])
    # bias gradients
    dyr = rnd(gen, M, 37).float()
    q1, q2, q3 = (torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in (N, N, 37))
    g0 = rnd(gen, N).float()
    q2.grad = g0.to(DEV).clone()
    A._colsum_group([(dy1.to(DEV), [q1, q2]), (dyr.to(DEV), [q3])])
    check([("db", q1.grad, dy1.double().sum(0), None), ("db acc", q2.grad, dy1.double().sum(0) + g0.double(), None),
           ("db ragged", q3.grad, dyr.double().sum(0), None)], ktol(M), "colsum_group M=%d" % M)


def test_linear_refuses_a_ragged_input_feature_count():
    """K & 3 != 0: the forward contraction refuses before any launch (no silent fallback)"""
    from show_edit_tell_amd import _lib, autograd_ops as A
    gen = torch.Generator().manual_seed(3)
    x, _ = pair(gen, 5, 6)
    w, _ = pair(gen, 8, 6)
    b, _ = pair(gen, 8)
    with pytest.raises(_lib.SetError):
        A.linear(x, w, b).sum().backward()
    dy = torch.ones(5, 8, device=DEV)
    with pytest.raises(_lib.SetError):
        A._dgrad(dy, w.detach())
    with pytest.raises(_lib.SetError):
        A._wgrad_mm(dy, x.detach())


@pytest.mark.parametrize("rows", [(5, 64), (64, 130), (130, 200), (1, 128, 129)])
def test_dgrad_group_column_slices_and_accumulation(rows):
    """_dgrad_group: problems on one side / on both sides of the 128-row class boundary (grouped launch or one by
    one), weights that are strided column slices of a wider matrix, and out= accumulation into a non-zero buffer"""
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(sum(rows))
    N, K = 64, 32
    Wfull = rnd(gen, N, 3 * K).float()
    Wd = Wfull.to(DEV)
    pairs, refs = [], []
    for i, M in enumerate(rows):
        dy = rnd(gen, M, N).float()
        w64 = Wfull[:, (i % 3) * K:(i % 3 + 1) * K].double()
        out0 = rnd(gen, M, K).float() if i % 2 else None
        ref = dy.double() @ w64 + (0 if out0 is None else out0.double())
        pairs.append((dy.to(DEV), Wd[:, (i % 3) * K:(i % 3 + 1) * K], None if out0 is None else out0.to(DEV)))
        refs.append(ref)
    outs = A._dgrad_group(pairs)
    check([("dX%d" % i, o, r, None) for i, (o, r) in enumerate(zip(outs, refs))], ktol(N), "dgrad_group %s" % (rows,))


@pytest.mark.parametrize("N", [3, 37, 64])
@pytest.mark.parametrize("M", [1, 5, 64, 130])
def test_wgrad_colsum_ragged_and_accumulating(M, N):
    """_wgrad_mm (N < 4, N & 3 != 0: padded buffer) and _colsum (rows on both sides of 64, cols % 4 != 0), fresh and
    accumulating into a non-zero buffer"""
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(100 * M + N)
    K = 32
    dy, x, w0, b0 = rnd(gen, M, N).float(), rnd(gen, M, K).float(), rnd(gen, N, K).float(), rnd(gen, N).float()
    dW = dy.double().t() @ x.double()
    db = dy.double().sum(0)
    got_w = A._wgrad_mm(dy.to(DEV), x.to(DEV))
    acc_w = A._wgrad_mm(dy.to(DEV), x.to(DEV), out=w0.to(DEV))
    got_b = A._colsum(dy.to(DEV))
    acc_b = A._colsum(dy.to(DEV), out=b0.to(DEV))
    named = [("dW", got_w, dW, None), ("dW acc", acc_w, dW + w0.double(), None), ("db", got_b, db, None),
             ("db acc", acc_b, db + b0.double(), None)]
    if N & 3:
        # the same gradient living in a zero-padded (rows, N4) buffer, as the loss backward writes the score gradient: read in
        # place by both (the padded column sum needs >= 64 rows, below that it is the plain path again)
        view = A.zero_padded_rows(1, M, N, torch.device(DEV))[0]
        view.copy_(dy.to(DEV))
        assert A._padded_view(view) is not None
        named += [("dW padded view", A._wgrad_mm(view, x.to(DEV)), dW, None), ("db padded view", A._colsum(view), db, None),
                  ("db padded view acc", A._colsum(view, out=b0.to(DEV)), db + b0.double(), None)]
    check(named, ktol(M), "wgrad/colsum M=%d N=%d" % (M, N))


@pytest.mark.parametrize("B", BATCHES)
def test_embed_relu_scatter_accumulates_repeated_ids(B):
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B)
    V, D, T = 11, 64, 3
    ids = torch.randint(0, V, (B, T), generator=gen)
    ids[0, 0] = ids[-1, -1]                                  # at least one repeated id when B * T > 1
    tab, tab64 = pair(gen, V, D)
    dout = rnd(gen, B, T, D)
    torch.relu(F.embedding(ids, tab64)).backward(dout)
    A.embed_relu(ids.to(DEV), tab).backward(dout.float().to(DEV))
    check([("dtable", tab.grad, tab64.grad, None)], ktol(B * T), "embed_relu B=%d" % B)


@pytest.mark.parametrize("rows", [1, 5, 64, 130])
def test_philox_dropout_backward(rows):
    from show_edit_tell_amd import autograd_ops as A, rng
    gen = torch.Generator().manual_seed(rows)
    seed, off, p, cols = 0x1_2345_6789, rng.offset(rng.SITE_OUT, 3), 0.5, 64
    x, _ = pair(gen, rows, cols)
    dy = rnd(gen, rows, cols).float()
    y = A.philox_dropout(x, p, seed, off)
    y.backward(dy.to(DEV))
    keep = PH.dropout_keep(seed, off, rows, cols, p)
    assert np.array_equal(y.detach().cpu().numpy(), np.where(keep, x.detach().cpu().numpy() * 2, 0).astype(np.float32))
    assert np.array_equal(x.grad.cpu().numpy(), np.where(keep, dy.numpy() * 2, 0).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# cells
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_lstm_cell(B):
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B)
    K, D = 96, 64
    names = ["x", "h", "c", "w_ih", "w_hh", "b_ih", "b_hh"]
    shapes = [(B, K), (B, D), (B, D), (4 * D, K), (4 * D, D), (4 * D,), (4 * D,)]
    scales = [1, 1, 1, 3 / math.sqrt(K), 3 / math.sqrt(D), 1, 1]
    dev, ref = zip(*[pair(gen, *s, scale=sc) for s, sc in zip(shapes, scales)])
    dh, dc = rnd(gen, B, D), rnd(gen, B, D)
    P = {"l.weight_ih": ref[3], "l.weight_hh": ref[4], "l.bias_ih": ref[5], "l.bias_hh": ref[6]}
    hn, cn = XG._nn_lstm_cell(P, "l", ref[0], ref[1], ref[2])
    torch.autograd.backward([hn, cn], [dh, dc])
    h, c = A.lstm_cell(*dev)
    torch.autograd.backward([h, c], [dh.float().to(DEV), dc.float().to(DEV)])
    check([(n, d.grad, r.grad, None) for n, d, r in zip(names, dev, ref)], FUSED, "lstm_cell B=%d" % B)


@pytest.mark.parametrize("B", BATCHES)
def test_copy_lstm(B):
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B + 7)
    K, D = 96, 64
    names = ["x", "h2", "c2", "cmem", "x2h.weight", "x2h.bias", "h2h.weight", "h2h.bias", "gate_cnew.weight",
             "gate_cnew.bias", "gate_cmem.weight", "gate_cmem.bias"]
    shapes = [(B, K), (B, D), (B, D), (B, D), (4 * D, K), (4 * D,), (4 * D, D), (4 * D,), (D, D), (D,), (D, D), (D,)]
    scales = [1, 1, 1, 1, 3 / math.sqrt(K), 1, 3 / math.sqrt(D), 1, 3 / math.sqrt(D), 1, 3 / math.sqrt(D), 1]
    dev, ref = zip(*[pair(gen, *s, scale=sc) for s, sc in zip(shapes, scales)])
    P = {"copy_lstm." + n: r for n, r in zip(names[4:], ref[4:])}
    dh, dm = rnd(gen, B, D), rnd(gen, B, D)
    hn, mem = ET.copy_lstm(P, ref[0], ref[1], ref[2], ref[3])
    torch.autograd.backward([hn, mem], [dh, dm])
    h, m = A.copy_lstm(*dev)
    torch.autograd.backward([h, m], [dh.float().to(DEV), dm.float().to(DEV)])
    check([(n, d.grad, r.grad, None) for n, d, r in zip(names, dev, ref)], FUSED, "copy_lstm B=%d" % B)


def _encoder_ref(emb, lens, w_ih, b_ih, w_hh, b_hh, reverse):
    B, T, _ = emb.shape
    D = w_hh.shape[1]
    h, c = torch.zeros(B, D, dtype=torch.float64), torch.zeros(B, D, dtype=torch.float64)
    Hs, Ms = [None] * T, [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        act = (lens > t).double().unsqueeze(1)
        i, f, g, o = (F.linear(emb[:, t], w_ih, b_ih) + F.linear(h, w_hh, b_hh)).chunk(4, 1)
        cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        hn = torch.sigmoid(o) * torch.tanh(cn)
        h, c = act * hn + (1 - act) * h, act * cn + (1 - act) * c
        Hs[t], Ms[t] = act * hn, act * cn
    return torch.stack(Hs, 1), torch.stack(Ms, 1), h


@pytest.mark.parametrize("want_mem", [True, False], ids=["mem", "nomem"])
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("mode", ["ragged", "equal"])
@pytest.mark.parametrize("B", BATCHES)
def test_encoder_lstm(B, mode, reverse, want_mem):
    """the caption encoders' recurrence as one node over a shrinking set of live rows (lengths 1 .. T, all equal)"""
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B + 13)
    T, E, D = 5, 64, 64
    lens = lens_for(B, T, mode)
    names = ["emb", "w_ih", "b_ih", "w_hh", "b_hh"]
    shapes = [(B, T, E), (4 * D, E), (4 * D,), (4 * D, D), (4 * D,)]
    scales = [1, 3 / math.sqrt(E), 1, 3 / math.sqrt(D), 1]
    dev, ref = zip(*[pair(gen, *s, scale=sc) for s, sc in zip(shapes, scales)])
    live = (torch.arange(T)[None, :] < lens[:, None]).double().unsqueeze(2)
    # (outputs behind a row's length are constant zeros: in the models nothing sends a gradient there)
    dH, dM, dl = rnd(gen, B, T, D) * live, rnd(gen, B, T, D) * live, rnd(gen, B, D)
    H64, M64, last64 = _encoder_ref(ref[0], lens, *ref[1:], reverse)
    out = A.encoder_lstm(dev[0], lens.to(DEV), *dev[1:], reverse=reverse, want_mem=want_mem)
    up = lambda t: t.float().to(DEV)
    if want_mem:
        torch.autograd.backward([H64, M64, last64], [dH, dM, dl])
        torch.autograd.backward(list(out), [up(dH), up(dM), up(dl)])
    else:
        torch.autograd.backward([H64, last64], [dH, dl])
        torch.autograd.backward(list(out), [up(dH), up(dl)])
    assert float((out[0].detach().double().cpu() - H64.detach()).abs().max()) < 2e-5
    check([(n, d.grad, r.grad, None) for n, d, r in zip(names, dev, ref)], FUSED,
          "encoder_lstm B=%d %s %s %s" % (B, mode, "rev" if reverse else "fwd", "mem" if want_mem else "nomem"))


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _mask(B, T, mode):
    lens = lens_for(B, T, mode)
    return (torch.arange(T)[None, :] < lens[:, None]).double()


@pytest.mark.parametrize("mode", ["ragged", "equal"])
@pytest.mark.parametrize("B", BATCHES)
def test_caption_attention(B, mode):
    """gated caption attention; both outputs get an upstream gradient (alpha: the dalpha_ext input of the kernel)"""
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B + 17)
    T, D, At = 7, 64, 32
    mask = _mask(B, T, mode)
    lin = [("cap_features_att", At, D), ("cap_decoder_att", At, D), ("cap_full_att", 1, At), ("context_gate", D, 3 * D),
           ("sc_affine", D, D), ("tc_affine", D, 2 * D)]
    H, H64 = f32(rnd(gen, B, T, D) * mask[:, :, None])
    h1, h164 = pair(gen, B, D)
    word, word64 = pair(gen, B, D)
    dev, P = [], {}
    for n, o, i in lin:
        for sfx, shape, sc in ((".weight", (o, i), 3 / math.sqrt(i)), (".bias", (o,), 1.0)):
            d, r = pair(gen, *shape, scale=sc)
            dev.append(d)
            P["caption_attention." + n + sfx] = r
    dg, da = rnd(gen, B, D), rnd(gen, B, T)
    g64, a64 = ET.caption_attention(P, H64, h164, word64, mask)
    torch.autograd.backward([g64, a64], [dg, da])
    g, a = A.caption_attention(H, h1, word, mask.float().to(DEV), *dev)
    torch.autograd.backward([g, a], [dg.float().to(DEV), da.float().to(DEV)])
    named = [("H", H.grad, H64.grad, None), ("h1", h1.grad, h164.grad, None), ("word", word.grad, word64.grad, None)]
    named += [(k, d.grad, r.grad, None) for d, (k, r) in zip(dev, P.items())]
    check(named, FUSED, "caption_attention B=%d %s" % (B, mode))


@pytest.mark.parametrize("with_att1", [False, True], ids=["att1-inside", "att1-given"])
@pytest.mark.parametrize("B", BATCHES)
def test_dcnet_caption_attention(B, with_att1):
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B + 19)
    T, Dh, D, At = 6, 64, 128, 32
    mask = _mask(B, T, "ragged")
    feats, feats64 = f32(rnd(gen, B, T, Dh) * mask[:, :, None])
    h1, h164 = pair(gen, B, D)
    dev, P = [], {}
    for n, o, i in (("cap_features_att", At, Dh), ("cap_decoder_att", At, D), ("cap_full_att", 1, At)):
        for sfx, shape, sc in ((".weight", (o, i), 3 / math.sqrt(i)), (".bias", (o,), 1.0)):
            d, r = pair(gen, *shape, scale=sc)
            dev.append(d)
            P["caption_attention." + n + sfx] = r
    dctx = rnd(gen, B, Dh)
    XG.dcnet_caption_attention(P, feats64, h164, mask).backward(dctx)
    att1 = A.linear(feats, dev[0], dev[1]) if with_att1 else None
    A.dcnet_caption_attention(feats, h1, mask.float().to(DEV), *dev, att1_c=att1).backward(dctx.float().to(DEV))
    named = [("feats", feats.grad, feats64.grad, None), ("h1", h1.grad, h164.grad, None)]
    named += [(k, d.grad, r.grad, None) for d, (k, r) in zip(dev, P.items())]
    check(named, FUSED, "dcnet_caption_attention B=%d" % B)


VA_SHAPES = [(5, L, 64, 32) for L in (1, 2, 5, 6, 7, 36, 49, 100, 256)] + \
            [(M, 7, 64, 32) for M in (1, 64, 130)] + [(3, 36, 2048, 64), (2, 49, 2048, 512)]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "rmask"])
@pytest.mark.parametrize("M,L,Dv,At", VA_SHAPES)
def test_visual_attention_from_att1(M, L, Dv, At, masked):
    """ReLU additive attention over L regions (L up to ATTB_MAX = 256, the largest the host-side check admits), with
    and without the adaptive model's region mask"""
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(M * 1000 + L + Dv)
    D = 64
    X = rnd(gen, M, L, Dv).abs().float()
    rmask = None
    if masked:
        n = (torch.arange(M) * 5 % L) + 1
        n[0] = L
        rmask = (torch.arange(L)[None, :] < n[:, None]).double()
    att1, att164 = pair(gen, M, L, At, scale=2.0)
    h1, h164 = pair(gen, M, D)
    dw, dw64 = pair(gen, At, D, scale=3 / math.sqrt(D))
    db, db64 = pair(gen, At)
    fw, fw64 = pair(gen, 1, At, scale=4 / math.sqrt(At))
    fb, fb64 = pair(gen, 1)
    dctx = rnd(gen, M, Dv)
    att2 = F.linear(h164, dw64, db64).unsqueeze(1)
    pre = att164 + att2
    no_kink(pre, att164, att2.expand_as(pre))
    e = F.linear(torch.relu(pre), fw64, fb64).squeeze(2)
    if masked:
        e = e.masked_fill(rmask == 0, -1e10)
    (X.double() * F.softmax(e, 1).unsqueeze(2)).sum(1).backward(dctx)
    cx = A.visual_attention_from_att1(X.to(DEV), att1, h1, dw, db, fw, fb, None if rmask is None else rmask.float().to(DEV))
    cx.backward(dctx.float().to(DEV))
    check([("att1", att1.grad, att164.grad, None), ("h1", h1.grad, h164.grad, None), ("dec_w", dw.grad, dw64.grad, None),
           ("dec_b", db.grad, db64.grad, None), ("full_w", fw.grad, fw64.grad, None), ("full_b", fb.grad, fb64.grad, None)],
          FUSED, "visual_attention M=%d L=%d Dv=%d A=%d" % (M, L, Dv, At))


@pytest.mark.parametrize("acc", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("tanh,want_dv", [(True, True), (False, False), (False, True), (True, False)],
                         ids=["tanh-dV", "relu", "relu-dV", "tanh"])
@pytest.mark.parametrize("M,L,Dv,At", [(5, 1, 64, 32), (5, 2, 64, 32), (3, 5, 64, 1024), (2, 7, 2048, 32), (5, 36, 128, 64),
                                       (2, 49, 64, 32), (1, 100, 64, 32), (2, 256, 64, 32), (64, 6, 64, 32),
                                       (130, 6, 64, 32)])
def test_attention_backward_kernel(M, L, Dv, At, tanh, want_dv, acc):
    """set_attention_bwd_acc_f32 directly — both kernel forms (with dV: 256 threads per sample; without: the wide form), A up
    to 1024 and Dv up to 2048 (more than the attention forwards admit), a non-zero dalpha_ext, and the accumulate-into-
    existing-gradient modes acc_datt1 / acc_dv with non-zero initial buffers"""
    from show_edit_tell_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(M + 10 * L + Dv + At)
    V64 = rnd(gen, M, L, Dv).float().double().requires_grad_(True)
    att1 = rnd(gen, M, L, At, scale=2.0).float().double().requires_grad_(True)
    att2 = rnd(gen, M, At, scale=2.0).float().double().requires_grad_(True)
    w = rnd(gen, At, scale=4 / math.sqrt(At)).float().double().requires_grad_(True)
    dctx, dal = rnd(gen, M, Dv).float().double(), rnd(gen, M, L).float().double()
    pre = att1 + att2.unsqueeze(1)
    if not tanh:
        no_kink(pre, att1, att2.unsqueeze(1).expand_as(pre))
    e = ((torch.tanh(pre) if tanh else torch.relu(pre)) * w).sum(2)
    e.retain_grad()
    alpha64 = F.softmax(e, 1)
    alpha = alpha64.detach().float()                     # the kernel's alpha input: the float64 softmax rounded once
    ctx = (V64 * alpha64.unsqueeze(2)).sum(1)
    ((ctx * dctx).sum() + (alpha64 * dal).sum()).backward()
    d = lambda t: t.detach().float().to(DEV).contiguous()
    datt1_0 = rnd(gen, M, L, At).float() if acc else torch.zeros(M, L, At)
    dV_0 = rnd(gen, M, L, Dv).float() if acc else torch.zeros(M, L, Dv)
    datt1, dV = datt1_0.to(DEV).clone(), (dV_0.to(DEV).clone() if want_dv else None)
    datt2, dwf = torch.empty(M, At, device=DEV), torch.empty(M, At, device=DEV)
    de = torch.empty(M, L, device=DEV)
    ins = [d(dctx), d(dal), alpha.to(DEV), d(V64), d(att1), d(att2), d(w)]
    rc = lib.set_attention_bwd_acc_f32(*[_lib.ptr(t) for t in ins], _lib.ptr(datt1), _lib.ptr(datt2), _lib.ptr(dwf),
                                       _lib.ptr(dV), _lib.ptr(de), M, L, Dv, At, int(tanh), int(acc), int(acc), At,
                                       _lib.stream_of(torch.device(DEV)))
    assert rc == 0
    named = [("datt1", datt1, att1.grad + datt1_0.double(), None), ("datt2", datt2, att2.grad, None),
             ("de", de, e.grad, None), ("dwfull", dwf.sum(0), w.grad, None)]
    if want_dv:
        named.append(("dV", dV, V64.grad + dV_0.double(), None))
    check(named, FUSED, "attention_bwd M=%d L=%d Dv=%d A=%d" % (M, L, Dv, At))


def test_attention_backward_refuses_what_it_does_not_support():
    """L > ATTB_MAX, A > 1024, Dv > 2048: SET_ERR_UNSUPPORTED from the host-side check, before any launch"""
    from show_edit_tell_amd import _lib, autograd_ops as A
    z = lambda *s: torch.zeros(*s, device=DEV)
    for M, L, Dv, At in ((1, 257, 64, 32), (1, 4, 64, 1028), (1, 4, 2052, 32)):
        with pytest.raises(_lib.SetError):
            A._attention_bwd(z(M, Dv), None, z(M, L), z(M, L, Dv), z(M, L, At), z(M, At), z(At), False, False)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("B", BATCHES)
def test_select(B, T, soft):
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B * 10 + T)
    D = 64
    Mem, Mem64 = pair(gen, B, T, D)
    al, al64 = f32(F.softmax(rnd(gen, B, T, scale=3.0), 1))
    dsel = rnd(gen, B, D)
    if not soft and T > 1:
        gap_ok(al64)
    ref = (Mem64 * al64.unsqueeze(2)).sum(1) if soft else ET.select_hard(Mem64, al64)
    ref.backward(dsel)
    (A.select_soft(Mem, al) if soft else A.select(Mem, al)).backward(dsel.float().to(DEV))
    check([("dM", Mem.grad, Mem64.grad, None), ("dalpha", al.grad, al64.grad, None)], FUSED,
          "select B=%d T=%d %s" % (B, T, "soft" if soft else "hard"))


# ---------------------------------------------------------------------------------------------------------------------
# losses / sampling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_mse_sum(B):
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B)
    a, a64 = pair(gen, B, 64)
    b, b64 = pair(gen, B, 64)
    ((a64 - b64) ** 2).sum().mul(0.3).backward()
    A.mse_sum(a, b).mul(0.3).backward()
    check([("da", a.grad, a64.grad, None), ("db", b.grad, b64.grad, None)], 1e-6, "mse_sum B=%d" % B)


@pytest.mark.parametrize("V", [37, 203, 1003])
@pytest.mark.parametrize("B", BATCHES)
def test_sample_pick_logprob_gradient(B, V):
    """d log_softmax(logits)[drawn word] / d logits = upstream * (onehot - softmax), at the word the device drew"""
    from show_edit_tell_amd import autograd_ops as A
    gen = torch.Generator().manual_seed(B + V)
    lg, lg64 = pair(gen, B, V, scale=3.0)
    g = rnd(gen, B)
    st = A.SampleState(B, 4, V - 2, -1, torch.device(DEV), seed=0x1_0000_0003, offset=5)
    logp = A.sample_pick(lg, st, 0)
    ids = st.seq[:, 0].cpu()
    ref = F.log_softmax(lg64, 1).gather(1, ids[:, None]).squeeze(1)
    assert float((logp.detach().double().cpu() - ref.detach()).abs().max()) < 1e-5
    ref.backward(g)
    logp.backward(g.float().to(DEV))
    check([("dlogits", lg.grad, lg64.grad, None)], FUSED, "sample_pick B=%d V=%d" % (B, V))
