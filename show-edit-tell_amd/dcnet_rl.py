"""DCNet free-running decode on MI355X (reference `dcnet_rl.py:256-361`)."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, stream_of
from .dcnet import DAE as _DAE_XE
from .dcnet import CaptionAttention, CaptionEncoder, Embedding  # noqa: F401
from .editnet import _i64c, _require_cuda


class DAE(_DAE_XE):
    """reference dcnet_rl.py:256-346: forward(word_map, prev, prevlen, sample_max, sample_rl)"""

    max_len = 18

    def forward(self, word_map, encoded_previous_captions, previous_cap_length, sample_max=True, sample_rl=False,
                temperature=1.0, top_k=0, top_p=1.0, sampler="cdf", constraints=None):
        """temperature / top_k / top_p / sampler: see editnet_rl.DecoderC.forward (no-grad sampled rollout only; "gumbel" is one
        persistent launch for 1 .. 8 rows with the token table built, the per-step kernels with the same draws otherwise).
        constraints: see editnet_rl.DecoderC.forward (no-grad greedy decode and no-grad sampled decode with sampler="cdf")"""
        if sampler != "cdf":
            _lib.check_sampler_name(sampler, top_k, top_p)
        _require_cuda(encoded_previous_captions, "previous captions")
        opts = _lib.sample_opts(temperature, top_k, top_p)
        grad_path = self._grad_path()
        gumbel = _lib.check_sampler(sampler, opts, sample_max, sample_rl, grad_path)
        if opts is not None:
            _lib.refuse_sample_opts(sample_max, sample_rl, grad_path)
        cons = None
        if constraints is not None:
            cons = _lib.decode_constraints(constraints, word_map, self.vocab_size, sample_max, sample_rl, grad_path, gumbel)
        if grad_path:
            return self._rollout_autograd(word_map, encoded_previous_captions, previous_cap_length, sample_max, sample_rl)
        lib = _lib.load()
        dev = encoded_previous_captions.device
        prev = _i64c(encoded_previous_captions)
        plen = _i64c(previous_cap_length.reshape(-1))
        B, max_len = prev.shape[0], self.max_len
        dims = self._dims(B, prev.shape[1], max_len + 1)
        ws = self._workspace(dims)
        w = self._weights(dims)
        with self._row_limits_scope(lib, B):
            seq = torch.empty(B, max_len, dtype=torch.long, device=dev)
            seq_logp = torch.empty(B, max_len, dtype=torch.float32, device=dev)
            if cons is not None:     # the constrained loops: per-step kernels at every batch size
                copts, banned = _lib.constraints_struct(cons, dev)               # (banned: alive until the call is enqueued)
                head = (C.byref(w), C.byref(dims), ptr(prev), ptr(plen), int(word_map['<start>']), int(word_map['<end>']), max_len)
                tail = (ptr(seq), ptr(seq_logp), ptr(ws), ws.numel(), stream_of(dev))
                if sample_rl:
                    from . import rng
                    check(lib.set_dcnet_sample_constrained(*head, rng.next_seed(), rng.offset(rng.SITE_ROLLOUT), *tail,
                                                           C.byref(opts) if opts is not None else None, C.byref(copts)),
                          "set_dcnet_sample_constrained")
                else:
                    check(lib.set_dcnet_greedy_constrained(*head, *tail, C.byref(copts)), "set_dcnet_greedy_constrained")
                if banned is not None:
                    banned.record_stream(torch.cuda.current_stream(dev))
                return seq, seq_logp
            if sample_rl:        # multinomial sampling, eval mode, no gradients: fused device loop, Philox epilogue
                from . import rng
                # (a NULL SetSampleOpts* is the call without options, bit for bit: include/set_hip.h)
                args = (C.byref(w), C.byref(dims), ptr(prev), ptr(plen), int(word_map['<start>']),
                        int(word_map['<end>']), max_len, rng.next_seed(), rng.offset(rng.SITE_ROLLOUT),
                        ptr(seq), ptr(seq_logp), ptr(ws), ws.numel(), stream_of(dev),
                        C.byref(opts) if opts is not None else None)
                if gumbel:
                    # one persistent launch where it applies (1 .. 8 rows, token table), the per-step loop with the same draws
                    # otherwise
                    rc = lib.set_dcnet_gumbel_persistent(*args)
                    if rc == 2:                          # SET_ERR_UNSUPPORTED: nothing was touched
                        check(lib.set_dcnet_sample_gumbel(*args), "set_dcnet_sample_gumbel")
                    else:
                        check(rc, "set_dcnet_gumbel_persistent")
                    return seq, seq_logp
                check(lib.set_dcnet_sample_opts(*args), "set_dcnet_sample_opts")
                return seq, seq_logp
            check(lib.set_dcnet_greedy(C.byref(w), C.byref(dims), ptr(prev), ptr(plen), int(word_map['<start>']),
                                       int(word_map['<end>']), max_len, ptr(seq), ptr(seq_logp), ptr(ws), ws.numel(),
                                       stream_of(dev)), "set_dcnet_greedy")
            return seq, seq_logp

    def sample_rollout(self, word_map, encoded_previous_captions, previous_cap_length, temperature=1.0, top_k=0, top_p=1.0,
                       constraints=None):
        """see editnet_rl.DecoderC.sample_rollout"""
        _lib.refuse_constraints(constraints, "sample_rollout")
        _require_cuda(encoded_previous_captions, "previous captions")
        return self._sample_rollout((word_map, encoded_previous_captions, previous_cap_length), {}, temperature, top_k, top_p)


def _dae_rollout(self, word_map, encoded_previous_captions, previous_cap_length, sample_max, sample_rl, opts=None):
    """dcnet_rl.py:286-346 over autograd-wrapped HIP operators (sampled SCST rollout / multinomial sampling).  opts: see
    editnet_rl.DecoderC._rollout_autograd."""
    import torch.nn.functional as F
    from . import autograd_ops as A
    from . import rng
    dev = encoded_previous_captions.device
    B, max_len = encoded_previous_captions.shape[0], self.max_len
    seed = self.__dict__["_fwd_seed"] = rng.next_seed()       # one seed per forward call (rng.py)
    training, p_emb, p_out = self.training, self.embed.dropout.p, self.dropout.p
    seq = torch.zeros(B, max_len, dtype=torch.long, device=dev)
    logps = []
    it = torch.full((B,), int(word_map['<start>']), dtype=torch.long, device=dev)
    h1, c1 = self.init_hidden_state(B)
    h2, c2 = self.init_hidden_state(B)
    enc, final_hidden, mask = self._encoder_autograd(encoded_previous_captions, previous_cap_length, seed)
    ca = self.caption_attention
    att1_c = A.linear(enc, ca.cap_features_att.weight, ca.cap_features_att.bias)
    from . import editnet as _editnet
    if sample_rl and _editnet._XE_SEQUENCE:       # the sampled rollout as ONE autograd node (dcnet_sequence.py, rollout mode)
        from . import dcnet_sequence as S
        cfg = S.SeqConfig([], training, p_emb, 0.0, p_out, seed,
                          rollout=dict(max_len=max_len, start_idx=int(word_map['<start>']), end_idx=int(word_map['<end>']),
                                       seed=seed, offset=rng.offset(rng.SITE_ROLLOUT), opts=opts))
        return S.dcnet_sequence(cfg, enc, final_hidden, mask, att1_c, torch.zeros(1, 1, dtype=torch.long, device=dev),
                                S.dae_params(self))
    unfinished = None
    state = (A.SampleState(B, max_len, word_map['<start>'], word_map['<end>'], dev, seed=seed,
                           offset=rng.offset(rng.SITE_ROLLOUT)) if sample_rl else None)
    for t in range(max_len + 1):
        if sample_rl:
            it = state.tokens[t]
        emb = A.philox_dropout(A.embed_relu(it, self.embed.embedding.weight), p_emb, seed, rng.offset(rng.SITE_EMBED, t), training)
        h1, c1, h2, c2 = self._step_autograd(emb, final_hidden, enc, mask, h1, c1, h2, c2, att1_c)
        logits = A.linear(A.philox_dropout(h2, p_out, seed, rng.offset(rng.SITE_OUT, t), training), self.fc.weight, self.fc.bias)
        if t == max_len:
            break
        if sample_rl:                    # dcnet_rl.py:320-340 on the device (Philox draw), no host sync
            logps.append(A.sample_pick(logits, state, t, opts))
            continue
        sample_logp, it = torch.max(F.log_softmax(logits, dim=1), 1)
        it = it.clone()
        it[it == int(word_map['<end>'])] = 0
        unfinished = (it > 0) if t == 0 else unfinished * (it > 0)
        it = it * unfinished.type_as(it)
        seq[:, t] = it
        logps.append(sample_logp.view(-1))
        if unfinished.sum() == 0:
            break
    if sample_rl:
        seq = state.seq
    seq_logp = torch.stack(logps, 1)
    if seq_logp.shape[1] < max_len:
        seq_logp = torch.cat([seq_logp, seq_logp.new_zeros(B, max_len - seq_logp.shape[1])], 1)
    return seq, seq_logp


DAE._rollout_autograd = _dae_rollout


class DAEWithAR(nn.Module):
    """reference dcnet_rl.py:348-361: wraps a trained DAE (+ an `affine_hidden` layer for the MSE
    variant).  The reference loads 'BEST_checkpoint_3_dae.pth.tar' inside __init__; here the DAE is
    passed in (or loaded from `checkpoint` if given) so the class is usable without that file."""

    def __init__(self, dae=None, checkpoint=None):
        super().__init__()
        if dae is None:
            if checkpoint is None:
                checkpoint = 'BEST_checkpoint_3_dae.pth.tar'
            dae = torch.load(checkpoint, weights_only=False)['dae']
        self.dae = dae
        decoder_dim = self.dae.decoder_dim
        self.affine_hidden = nn.Linear(decoder_dim, decoder_dim)

    def forward(self, *args, **kwargs):
        return self.dae(*args, **kwargs)

    def sample_rollout(self, *args, **kwargs):
        return self.dae.sample_rollout(*args, **kwargs)
