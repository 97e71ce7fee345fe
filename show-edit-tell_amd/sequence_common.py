"""What the two whole-sequence training nodes (`xe_sequence.py` EditNet, `dcnet_sequence.py` DCNet) share around their
recurrent steps: the thin C-ABI callers, the recurrent state logs, the log and backward of a sampled rollout, the score
head (fc over the log of its inputs) and the table of parameter gradients.  Host-side only."""
import ctypes as C

import torch

from . import _lib
from . import autograd_ops as A
from ._lib import check, ptr, stream_of


def _z(*shape, dev):
    return torch.zeros(*shape, dtype=torch.float32, device=dev)


def _e(*shape, dev):
    return torch.empty(*shape, dtype=torch.float32, device=dev)


def _rows(t2d, n):
    return t2d if t2d.shape[0] == n else t2d[:n]


class _Ops:
    """thin, allocation-free callers of the C ABI for one (device, stream)"""

    def __init__(self, dev):
        self.lib = _lib.load()
        self.dev = dev
        self.st = stream_of(dev)
        self._ws = {}

    def ws(self, key, nbytes):
        w = self._ws.get(key)
        if w is None or w.numel() < nbytes:
            w = self._ws[key] = torch.empty(max(16, nbytes), dtype=torch.uint8, device=self.dev)
        return w

    def pack(self, dst, rows, srcs, accumulate=False):
        """dst[:rows, :sum(cols)] (+)= [src0 | src1 | ...]; srcs: 2-D views with unit inner stride"""
        n = len(srcs)
        ps = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
        ls = (C.c_int64 * n)(*[s.stride(0) for s in srcs])
        cs = (C.c_int * n)(*[s.shape[1] for s in srcs])
        check(self.lib.set_pack_f32(dst.data_ptr(), dst.stride(0), rows, n, ps, ls, cs, int(accumulate), self.st), "set_pack_f32")

    def dropout(self, x, y, rows, cols, p, seed, offset):
        check(self.lib.set_dropout_f32(x.data_ptr(), x.stride(-2), y.data_ptr(), y.stride(-2), rows, cols, p, seed, offset,
                                       self.st), "set_dropout_f32")

    def dropout_bwd(self, dy, y, dx, rows, cols, scale, accumulate):
        check(self.lib.set_dropout_bwd_f32(dy.data_ptr(), dy.stride(-2), y.data_ptr(), y.stride(-2), dx.data_ptr(),
                                           dx.stride(-2), rows, cols, scale, int(accumulate), self.st), "set_dropout_bwd_f32")

    def linear(self, x, w, b, y, M):
        """y[:M] = x[:M] w^T + b   (x, y: 2-D views, unit inner stride)"""
        K, N = w.shape[1], w.shape[0]
        ws = self.ws("lin", self.lib.set_linear_workspace_bytes(M, N, K))
        check(self.lib.set_linear_f32(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), ptr(b), y.data_ptr(), y.stride(0),
                                      M, N, K, _lib.ACT_NONE, ws.data_ptr(), ws.numel(), self.st), "set_linear_f32")


def _dvalues(alpha, dctx, ops):
    """dH (B, Tc, D) = sum_t alpha[t, b, :] (outer) dctx[t, b, :] over the per-sequence logs (rows of finished sequences are
    zero in both), one launch"""
    T, B, Tc = alpha.shape
    D = dctx.shape[2]
    dH = torch.empty(B, Tc, D, dtype=torch.float32, device=alpha.device)
    check(ops.lib.set_attention_dvalues_f32(alpha.data_ptr(), dctx.data_ptr(), dH.data_ptr(), T, B, Tc, D, 0, ops.st),
          "set_attention_dvalues_f32")
    return dH


def gg(items):
    """[(dy, w_view, out, accumulate)] -> out (+)= dy . w, one grouped launch"""
    A.gemm_group([(dy, wv, dy.shape[0], wv.shape[1], dy.shape[1], out, acc) for dy, wv, out, acc in items], False, True)


def state_logs(T, B, D, uniform, dev):
    """the logs of the two recurrent states: slot t = state BEFORE step t; slot 0 = the zero initial state"""
    L = {}
    for k in ("H1", "C1", "H2", "C2"):
        L[k] = (_e if uniform else _z)(T + 1, B, D, dev=dev)
        if uniform:
            L[k][0].zero_()
    return L


def fc_inputs(L, cfg):
    """(T, B, D) rows the score head reads: h2 after every step, through the output dropout where there is one"""
    return L["H2D"] if (cfg.train and cfg.p_out > 0) else L["H2"][1:]


def dropout_scale(cfg, p):
    """what the backward of a dropout site of probability p multiplies the kept elements by"""
    return 1.0 / (1.0 - p) if (cfg.train and p > 0) else 1.0


def last_hidden(H2, lens):
    """h2 of every row at its last step = slot len_b of the state log (slot 0 holds the zero initial state: a row of decode
    length 0), before the output dropout; row order"""
    idx = torch.tensor(lens, dtype=torch.long, device=H2.device)
    return H2[idx, torch.arange(H2.shape[1], device=H2.device)]


def last_hidden_bwd_step(ops, DH2, dlast, bts, t):
    """rows whose last step this is, [bts[t + 1], bts[t]): d(last hidden) `dlast` (None: no such output) joins dh2"""
    b0 = bts[t + 1] if t + 1 < len(bts) else 0
    if dlast is not None and bts[t] > b0:
        ops.pack(DH2[b0:], bts[t] - b0, [dlast[b0:bts[t]]], accumulate=True)


def score_head(ops, hout, fc_w, fc_b, bts, uniform):
    """scores (B, T, V) of the logged fc inputs hout (T, B, D)"""
    T, B, D = hout.shape
    V = fc_w.shape[0]
    if uniform:                        # fc over all timesteps at once: (T, B, V), returned as its (B, T, V) view
        pred_tb = _e(T, B, V, dev=ops.dev)
        ops.linear(hout.reshape(T * B, D), fc_w, fc_b, pred_tb.view(T * B, V), T * B)
        return pred_tb.transpose(0, 1)
    out = _z(B, T, V, dev=ops.dev)     # rows that left the batch keep zero scores (editnet.py:547)
    for t in range(T):
        ops.linear(hout[t], fc_w, fc_b, out[:, t], bts[t])
    return out


def score_head_bwd(dp2, hout, fc_w, fc_b, need_w, need_b):
    """d scores (T * B, V) -> (d hout (T, B, D), g fc_w, g fc_b): d hout for all timesteps in one contraction; fc.weight's
    gradient is final here (eager: its all-reduce runs underneath the BPTT loop in the data-parallel step)"""
    T, B, D = hout.shape
    dH2D = A._dgrad(dp2, fc_w).view(T, B, D)
    g_b = A._bgrad(fc_b, dp2) if need_b else None
    g_w = A._wgrad(fc_w, dp2, hout.reshape(T * B, D), eager=True) if need_w else None
    return dH2D, g_w, g_b


class RolloutLog:
    """SampleState of a free-running sampled rollout (editnet_rl.py:514-547, dcnet_rl.py:305-344: the token of step t is what the
    sampling epilogue drew at step t - 1) and its per-step logs, kept in the node's log dict L: LOGITS, RAW, LSE, LOGP, KEY"""

    def __init__(self, L, ro, B, T, V, dev):
        self.state = A.SampleState(B, T, ro["start_idx"], ro["end_idx"], dev, seed=ro.get("seed"), offset=ro.get("offset", 0))
        self.L, self.T, self.B, self.V = L, T, B, V
        L["RAW"] = torch.empty(T, B, dtype=torch.long, device=dev)
        L["LSE"], L["LOGP"] = _e(T, B, dev=dev), _e(T, B, dev=dev)
        self.opts = ro.get("opts")         # _lib.SampleOpts or None: with options every step also logs its kept set's threshold
        if self.opts is None:
            L["LOGITS"] = _e(T, B, V, dev=dev)
        else:
            L["KEY"] = torch.empty(T, B, dtype=torch.int32, device=dev)
            # rows padded to 16 bytes: the pick reads them into registers (the word enumeration of the fused no-grad rollout:
            # the same seed draws the same words) and the backward reads them as float4
            L["LOGITS"] = _e(T, B, (V + 3) & ~3, dev=dev)[:, :, :V]
        self.tokens, self.seq = self.state.tokens, self.state.seq

    def step(self, ops, hz, fc_w, fc_b, t):
        """scores of step t from its fc input hz, then the device sampling epilogue"""
        s, L, B, V, T = self.state, self.L, self.B, self.V, self.T
        lg = L["LOGITS"][t]
        ops.linear(hz, fc_w, fc_b, lg, B)
        tail = (B, V, t, T, s.end_idx, s.seed, s.offset, s.seq.data_ptr(), s.tokens[t + 1].data_ptr(), s.unfinished.data_ptr(),
                s.alive.data_ptr(), L["RAW"][t].data_ptr(), L["LSE"][t].data_ptr(), L["LOGP"][t].data_ptr(), ops.st)
        if self.opts is not None:
            check(ops.lib.set_sample_pick_opts_key_f32(lg.data_ptr(), L["LOGITS"].stride(1), *tail, C.byref(self.opts),
                                                       L["KEY"][t].data_ptr()), "set_sample_pick_opts_key_f32")
        else:
            check(ops.lib.set_sample_pick_f32(lg.data_ptr(), V, *tail), "set_sample_pick_f32")

    def backward(self, ops, dlogp):
        """d seq_logp (B, T) -> d scores of every step as (T * B, V) rows (sampling epilogue backward); frees the score log"""
        L, T, B, V = self.L, self.T, self.B, self.V
        dl = dlogp.t().contiguous()                            # (T, B)
        dp = A.zero_padded_rows(T, B, V, ops.dev)      # rows padded to 16 bytes: the fc contractions read them in place
        if self.opts is not None:          # the truncated log-prob: all T * B rows of the (contiguous) logs in ONE launch
            check(ops.lib.set_sample_logp_bwd_opts_f32(L["LOGITS"].data_ptr(), L["LOGITS"].stride(1), L["LSE"].data_ptr(),
                                                       L["RAW"].data_ptr(), L["KEY"].data_ptr(), dl.data_ptr(), dp.data_ptr(),
                                                       dp.stride(1), T * B, V, C.byref(self.opts), ops.st),
                  "set_sample_logp_bwd_opts_f32")
        for t in (range(T) if self.opts is None else ()):
            check(ops.lib.set_sample_logp_bwd_f32(L["LOGITS"][t].data_ptr(), V, L["LSE"][t].data_ptr(), L["RAW"][t].data_ptr(),
                                                  dl[t].data_ptr(), dp[t].data_ptr(), dp.stride(1), B, V, ops.st),
                  "set_sample_logp_bwd_f32")
        L["LOGITS"] = None
        return dp.as_strided((T * B, V), (dp.stride(1), 1), dp.storage_offset())


class ParamGrads:
    """the gradients a node's backward returns for its parameters, in `names` order; frozen parameters (`need` False:
    requires_grad False) get no gradient and no contraction"""

    def __init__(self, names, params, need):
        self.idx = {n: i for i, n in enumerate(names)}
        self.params, self.need = params, need
        self.g = [None] * len(names)

    def wants(self, name):
        return self.need[self.idx[name]]

    def put(self, name, grad):
        self.g[self.idx[name]] = grad

    def W(self, name, dy, x, hi=None):
        """weight gradient dy^T x over the log rows [0, hi)"""
        if self.wants(name):
            self.put(name, A._wgrad(self.params[self.idx[name]], dy[:hi], x[:hi]))

    def Bg(self, name, dy):
        if self.wants(name):
            self.put(name, A._bgrad(self.params[self.idx[name]], dy))

    def blocks(self, name, blocks):
        """weight gradient assembled from column blocks [(dy, x, first column)] (`autograd_ops._wgrad_blocks`)"""
        if self.wants(name):
            self.put(name, A._wgrad_blocks(self.params[self.idx[name]], blocks))

    def embedding(self, name, ids, drows):
        """gradient of an embedding table: the rows drows scattered to the words ids fed to the steps"""
        if self.wants(name):
            self.put(name, torch.zeros_like(self.params[self.idx[name]]).index_add_(0, ids, drows))

    def tuple(self):
        return tuple(self.g)
