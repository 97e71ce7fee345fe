"""Stage 2 of DCNet training on MI355X (reference `dcnet_with_mse.py`): the stage-1 DAE wrapped in `DAEWithAR` and trained
on XE + MSE(affine_hidden(decoder_last_hidden), gd_final_hidden) (`train.dcnet_mse_train_step`).

`DAE` is `dcnet.DAE` with the reference's six-output forward (`dcnet_with_mse.py:303-343`).  Besides the teacher-forced
scores it returns `gd_final_hidden`, the caption encoder run on the sorted ground-truth captions (`:322`; in train mode its
embedding dropout is its own Philox site, rng.SITE_ENC2_EMBED), and `decoder_last_hidden`, every row's h2 at its last
step before the output dropout (`:321, 341`).  No-grad: `set_dcnet_xe_forward_hidden` (for B <= 8 one persistent launch)
and the caption encoder's fused path.  Grad-enabled: the whole-sequence node or the per-operator route
(`dcnet.DAE._forward_autograd(..., hidden=True)`) and the encoder's autograd operators.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from . import dcnet as _dcnet
from ._lib import check, ptr, stream_of
from .dcnet import CaptionAttention, CaptionEncoder, Embedding  # noqa: F401
from .editnet import _HipLinear, _i64c, _require_cuda


class DAE(_dcnet.DAE):
    """reference dcnet_with_mse.py:273-343"""

    def forward(self, encoded_captions, caption_lengths, encoded_previous_captions, previous_cap_length):
        """returns (predictions, encoded_captions sorted, decode_lengths, sort_ind, gd_final_hidden, decoder_last_hidden)"""
        _require_cuda(encoded_captions, "captions")
        if self._grad_path():
            return self._forward_autograd(encoded_captions, caption_lengths, encoded_previous_captions,
                                          previous_cap_length, hidden=True)
        caption_lengths, sort_ind = caption_lengths.squeeze(1).sort(dim=0, descending=True, stable=True)
        caps = _i64c(encoded_captions[sort_ind])
        prev = _i64c(encoded_previous_captions[sort_ind])
        plen = _i64c(previous_cap_length[sort_ind].reshape(-1))
        _, gd_final_hidden, _ = self._encode(caps, caption_lengths)                 # dcnet_with_mse.py:322
        decode_lengths = (caption_lengths - 1).tolist()
        predictions, last = self._xe_forward_hidden(caps, decode_lengths, prev, plen)
        return predictions, caps, decode_lengths, sort_ind, gd_final_hidden, last

    def _xe_forward_hidden(self, caps, decode_lengths, prev, plen, want_last=True):
        """the teacher-forced loop on sorted inputs: (predictions (B, maxT, V), decoder_last_hidden (B, D) or None)"""
        lib = _lib.load()
        dev = caps.device
        B = caps.shape[0]
        maxT = max(decode_lengths)
        dims = self._dims(B, prev.shape[1], maxT)
        ws = self._workspace(dims)
        w = self._weights(dims)
        predictions = torch.empty(B, maxT, self.vocab_size, dtype=torch.float32, device=dev)
        last = torch.empty(B, self.decoder_dim, dtype=torch.float32, device=dev) if want_last else None
        dl = (C.c_int * B)(*decode_lengths)
        check(lib.set_dcnet_xe_forward_hidden(C.byref(w), C.byref(dims), ptr(caps), caps.shape[1], dl, ptr(prev), ptr(plen),
                                              ptr(predictions), ptr(last), ptr(ws), ws.numel(), stream_of(dev)),
              "set_dcnet_xe_forward_hidden")
        return predictions, last


class DAEWithAR(nn.Module):
    """reference dcnet_with_mse.py:345-360: a trained DAE + `affine_hidden` (nn.Linear(D, D), default initialisation).
    As in dcnet_rl.DAEWithAR the DAE is passed in (or loaded from `checkpoint`, default the reference's
    'BEST_checkpoint_3_dae.pth.tar').  A stage-1 `dcnet.DAE` is taken over in place — its class becomes this module's `DAE`,
    no weight is copied — which is what unpickling the stage-1 checkpoint inside dcnet_with_mse.py does.  state_dict keys
    `dae.*`, `affine_hidden.*`: the stage-3 `dcnet_rl.DAEWithAR` loads them strictly."""

    def __init__(self, dae=None, checkpoint=None):
        super().__init__()
        if dae is None:
            if checkpoint is None:
                checkpoint = 'BEST_checkpoint_3_dae.pth.tar'
            dae = torch.load(checkpoint, weights_only=False)['dae']
        if type(dae) is _dcnet.DAE:
            dae.__class__ = DAE
        elif not isinstance(dae, DAE):
            raise TypeError("DAEWithAR wraps a dcnet.DAE (stage 1) or a dcnet_with_mse.DAE, got %s" % type(dae).__name__)
        self.dae = dae
        decoder_dim = self.dae.decoder_dim
        self.affine_hidden = _HipLinear(decoder_dim, decoder_dim).to(self.dae.fc.weight.device)

    def forward(self, *args):
        scores, caps_sorted, decode_lengths, sort_ind, gd_final_hidden, decoder_last_hidden = self.dae(*args)
        decoder_last_hidden = self.affine_hidden(decoder_last_hidden)
        return scores, caps_sorted, decode_lengths, sort_ind, gd_final_hidden, decoder_last_hidden
