"""ORACLE (test infrastructure) for the split-K partial consumers (include/set_hip.h SetSlabSrc, the *_src_f32 entry points):
the documented value of a gradient given as base + a list of addends that are still partials, in fp32 with the documented
order of additions and in float64, and the float64 closed forms of the six operators' backward written from the formulas at
the top of each kernel in csrc/backward.hip.  tests/test_slab_src_oracle_cpu.py pins every closed form to torch autograd
before tests/test_hip_slab_src.py lets it judge a kernel.  No GPU is needed to import or run this module."""
import collections

import numpy as np
import torch

from oracle import philox_np as PH

# one addend as the host describes it.  t: (nslab, rows_alloc, ld) float32 (None for an entry without partials); rows: the
# rows the entry declares (the buffer may hold more: the test fills those with NaN); slab_stride: floats between two
# partials (None: the tensor's own, rows_alloc * ld)
Entry = collections.namedtuple("Entry", "t rows nslab slab_stride", defaults=(None,))


def _entry_sum(e, M, D, dtype):
    s = torch.zeros(M, D, dtype=dtype)
    r = min(e.rows, M)
    if e.nslab > 0 and r > 0:
        for k in range(e.nslab):                              # slab 0 first, starting from +0
            s[:r] = s[:r] + e.t[k, :r, :D].to(dtype)
    return s


def ordered_sum32(base, entries, M, D):
    """the header's value in fp32: v = base (or 0); for each entry in list order: v = v + (its slabs added in slab order
    starting from +0).  Rows m >= entry.rows and entries with nslab == 0 contribute exactly 0."""
    v = torch.zeros(M, D, dtype=torch.float32) if base is None else base.detach().cpu().float().clone()
    for e in entries:
        v = v + _entry_sum(e, M, D, torch.float32)
    return v


def sum64(base, entries, M, D):
    v = torch.zeros(M, D, dtype=torch.float64) if base is None else base.detach().cpu().double().clone()
    for e in entries:
        v = v + _entry_sum(e, M, D, torch.float64)
    return v


def src_array(entries, device):
    """host entries -> (ctypes array of _lib.SlabSrc or None, count, the device tensors that must stay alive)"""
    from show_edit_tell_amd import _lib
    if not entries:
        return None, 0, []
    arr, keep = (_lib.SlabSrc * len(entries))(), []
    for i, e in enumerate(entries):
        if e.t is None:
            arr[i] = _lib.SlabSrc(None, 0, 0, e.nslab, e.rows)
            continue
        t = e.t.to(device).contiguous()
        keep.append(t)
        stride = t.stride(0) if e.slab_stride is None else e.slab_stride
        arr[i] = _lib.SlabSrc(t.data_ptr(), stride, t.shape[2], e.nslab, e.rows)
    return arr, len(entries), keep


# ---------------------------------------------------------------------------------------------------------------------
# float64 closed forms (csrc/backward.hip).  `gates` holds the post-activation (i, f, g, o) blocks of width D side by side.
# ---------------------------------------------------------------------------------------------------------------------
def lstm_cell_bwd(dh, dc, gates, c_prev, c_new):
    """c' = f c + i g ; h' = o tanh(c') (editnet.py:235-242) -> (dgates (M, 4D) pre-activation gradients, dc_prev)"""
    i, f, g, o = gates.chunk(4, 1)
    tc = torch.tanh(c_new)
    dct = (0 if dc is None else dc) + dh * o * (1 - tc * tc)
    dgates = torch.cat([dct * g * i * (1 - i), dct * c_prev * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return dgates, dct * f


def dropout_bwd(dy, seed, offset, p):
    """backward of the Philox dropout of set_dropout_bwd_philox_f32: element (row, col) is kept iff the word col % 4 of
    counter (row, col / 4, offset), key seed, is >= p as a 24-bit uniform; kept elements are scaled by 1 / (1 - p)"""
    if p <= 0:
        return dy
    keep = PH.dropout_keep(seed, offset, dy.shape[0], dy.shape[1], p)
    return dy * torch.from_numpy(np.ascontiguousarray(keep)).to(dy.dtype) / (1.0 - p)


def copy_gate_bwd(dh, dadp, ogate, adp, cg, cmem, c_new):
    """cg = sig(u) ; adp = cg cm + (1 - cg) cn ; h = o tanh(adp) (editnet.py:281-283) -> (du, dcm_direct, dcn_direct, do_pre)"""
    ta = torch.tanh(adp)
    dat = (0 if dadp is None else dadp) + dh * ogate * (1 - ta * ta)
    return dat * (cmem - c_new) * cg * (1 - cg), dat * cg, dat * (1 - cg), dh * ta * ogate * (1 - ogate)


def lstm_gates_bwd(dcn, do_pre, gates, c_prev):
    """the LSTM part of the copy cell given d c_new and the o-gate's pre-activation gradient -> (dgates, dc_prev)"""
    i, f, g, _ = gates.chunk(4, 1)
    return torch.cat([dcn * g * i * (1 - i), dcn * c_prev * f * (1 - f), dcn * i * (1 - g * g), do_pre], 1), dcn * f


def select_bwd(dsel, Mem, alpha, dM0=None):
    """sel = w M[j*], w = a + (1 - a_detached), j* = the first arg-max of alpha (editnet.py:409-420): dM[b, j*] = w dsel,
    dalpha[b, j*] = <dsel, M[b, j*]>, zero elsewhere.  dM0: the accumulating form adds to it (only row j* changes)."""
    B = alpha.shape[0]
    val, idx = alpha.max(1)
    rows = torch.arange(B)
    dM = torch.zeros_like(Mem) if dM0 is None else dM0.clone()
    dM[rows, idx] = dM[rows, idx] + (val + (1 - val)).unsqueeze(1) * dsel
    dalpha = torch.zeros_like(alpha)
    dalpha[rows, idx] = (dsel * Mem[rows, idx]).sum(1)
    return dM, dalpha


def context_gate_bwd(dout, zt, s, t):
    """out = zt s + (1 - zt) t with zt = sig(.), s = tanh(.), t = tanh(.) (editnet.py:378-380) -> pre-activation gradients"""
    return dout * (s - t) * zt * (1 - zt), dout * zt * (1 - s * s), dout * (1 - zt) * (1 - t * t)


def attention_bwd(dctx, dalpha_ext, alpha, V, att1, att2, w_full, use_tanh):
    """additive attention (editnet.py:370-376 tanh, :443-446 ReLU): ctx = sum_l alpha_l V_l, alpha = softmax(e),
    e_l = <w_full, act(att1_l + att2)> -> (datt1 (M, L, A), datt2 (M, A), dwfull_part (M, A), de (M, L))"""
    dalpha = (V * dctx.unsqueeze(1)).sum(2)
    if dalpha_ext is not None:
        dalpha = dalpha + dalpha_ext
    de = alpha * (dalpha - (alpha * dalpha).sum(1, keepdim=True))
    pre = att1 + att2.unsqueeze(1)
    if use_tanh:
        act = torch.tanh(pre)
        dact = 1 - act * act
    else:
        act = torch.relu(pre)
        dact = (pre > 0).to(pre.dtype)
    datt1 = de.unsqueeze(2) * w_full * dact
    return datt1, datt1.sum(1), (de.unsqueeze(2) * act).sum(1), de
