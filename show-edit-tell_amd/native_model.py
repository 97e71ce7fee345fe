"""The runtime plumbing that `editnet.DecoderC` and `dcnet.DAE` (and their RL / adaptive / MSE subclasses) share: what of a
module is runtime state and must not travel, the inference-time token table and its invalidation rules, the workspace cache,
the packed weight pointers and the thread-local row limits.  A model declares what differs:

  _ABI                        "editnet" / "dcnet": the C entry points are set_<abi>_workspace_bytes, _token_table_bytes,
                              _token_table_workspace_bytes, _build_token_table and _ws_tensor (include/set_hip.h)
  _DIMS_CLS, _WEIGHTS_CLS,    the ctypes structs of _lib.py and the (field, state_dict key) table
  _WEIGHT_FIELDS
  _DISPLAY, _HANDLE           how messages name the model ("EditNet") and an instance of it ("decoder")
  _DIMS_HINT                  appended to the refusal of unsupported dims
  _token_table_sources()      the six parameter tensors the token table is derived from
  _token_table_supported(d)   whether the kernels take a table at these dims
  _dims(...)                  the dims struct of a call (the signatures differ)

The decode loops themselves (`forward`, `_forward_autograd`, `_rollout_autograd`) stay with the models.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, stream_of


class NativeModel(nn.Module):
    _ABI = _DIMS_CLS = _WEIGHTS_CLS = _WEIGHT_FIELDS = None
    _DISPLAY = _HANDLE = None
    _DIMS_HINT = ""

    # Optional per-row cap on the caption length of the no-grad free-running loops (include/set_hip.h set_decode_row_limits):
    # an int32 device tensor of B entries, or None.  Row b is ended by the loop after at most row_limits[b] words.
    row_limits = None

    def __init__(self):
        super().__init__()
        self._ws = None
        self._ws_key = None

    # ---- runtime state is NOT part of the module's persistent state --------------------------------------
    # The reference checkpoints pickle the whole module (editnet.py:168-175 `'decoder': decoder`, dcnet.py:131-138) and
    # callers may copy.deepcopy a model: GPU workspaces, the derived token table, prologues run ahead and the last autograd
    # graph must not travel.
    _RUNTIME_ATTRS = ("_ws", "_ws_key", "_ws_cache", "_tok_state", "_last_hidden", "_fwd_seed", "_fed_tokens", "_grad_buckets",
                      "_caplens_host", "_ahead", "_ahead_free", "_ahead_hits", "_ahead_busy")

    def __getstate__(self):
        state = dict(self.__dict__)
        for k in self._RUNTIME_ATTRS:
            state.pop(k, None)
        state["_ws"] = state["_ws_key"] = None
        return state

    def invalidate_token_table(self):
        """Drop the derived inference-time token table (see _token_table).  It is rebuilt automatically after two
        further no-grad calls.  Called on every train() <-> eval() switch, load_state_dict() and device / dtype move;
        call it yourself after writing weights in a way autograd cannot see (`p.data.add_()`, `dist.broadcast(p.data)`,
        raw-pointer updates): such writes do not bump `tensor._version`, which is all the cache can observe
        without a device->host synchronisation (SET_TOKEN_TABLE_VERIFY=1 adds that check for debugging)."""
        self.__dict__.pop("_tok_state", None)

    def train(self, mode=True):
        if bool(mode) != self.training:          # an actual train <-> eval switch (eval() on an eval module keeps the table)
            self.invalidate_token_table()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self.invalidate_token_table()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_token_table()
        for k in ("_ws_cache", "_ahead", "_ahead_free", "_grad_buckets"):
            self.__dict__.pop(k, None)
        self._ws = self._ws_key = None
        return super()._apply(fn, *args, **kwargs)

    # ---- reference API ---------------------------------------------------------------------
    def init_hidden_state(self, batch_size):
        dev = self.fc.weight.device          # the parameters' device (the reference uses a module global)
        h = torch.zeros(batch_size, self.decoder_dim, device=dev)
        c = torch.zeros(batch_size, self.decoder_dim, device=dev)
        return h, c

    # ---- runtime plumbing ------------------------------------------------------------------
    def _grad_path(self):
        """True when a call of the model runs the autograd route: train mode (dropout), or gradients are wanted"""
        return self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))

    def _sample_rollout(self, lead, tail, temperature, top_k, top_p):
        """The body of the models' `sample_rollout(...)`: one sampled rollout -> (seq, seqLogprobs) under temperature / top_k /
        top_p (include/set_hip.h SetSampleOpts).  `forward` refuses the options where gradients flow; here the grad path (train
        mode, or parameters that require grad) runs the autograd rollout with them: seqLogprobs are the log-probs of the
        distribution sampled from and their backward holds every step's kept set constant (set_sample_logp_bwd_opts_f32).
        Without gradients, and with neutral options, this is forward(sample_max=False, sample_rl=True, ...) call for call.
        lead / tail: the model's positional arguments before, and keyword arguments after, (sample_max, sample_rl)."""
        opts = _lib.sample_opts(temperature, top_k, top_p)
        if opts is None or not self._grad_path():
            return self.forward(*lead, sample_max=False, sample_rl=True, **tail, temperature=temperature, top_k=top_k, top_p=top_p)
        return self._rollout_autograd(*lead, False, True, **tail, opts=opts)

    def _entry(self, lib, what):
        return getattr(lib, "set_%s_%s" % (self._ABI, what))

    def _weights(self, dims=None):
        """Pack the parameter pointers; with `dims` (the no-grad decode paths), also attach the inference-time token
        table when it is valid (see _token_table)."""
        w = _lib.pack_weights(self._WEIGHTS_CLS, self._WEIGHT_FIELDS, dict(self.named_parameters()), self.fc.weight.device)
        if dims is not None:
            tab = self._token_table(dims)
            if tab is not None:
                w.tok_table = tab.data_ptr()
        return w

    # The contractions of the step (and of the caption encoder) whose only input is a token are folded into a per-word
    # table (include/set_hip.h: tok_table; EditNet (V,10D), DCNet (V,4D+8C)).  The table is derived from six parameter
    # tensors (_token_table_sources) and is rebuilt whenever any of them changes (tensor._version / data_ptr), on every
    # train()/eval() switch, load_state_dict() and device move (invalidate_token_table); it is only built once the same
    # weights have been seen on two consecutive no-grad calls, so SCST training (weights change every
    # iteration, and the loop toggles eval()/train()) never pays for it.  In-place writes through `.data`
    # are invisible to `_version`: call invalidate_token_table() after them.
    # SET_TOKEN_TABLE=0 disables, =1 forces, SET_TOKEN_TABLE_VERIFY=1 re-checks a checksum of the six
    # source tensors on every use (one device->host sync per call; debugging aid).
    def _token_table(self, dims):
        mode = os.environ.get("SET_TOKEN_TABLE", "auto")
        if mode == "0" or not self._token_table_supported(dims):
            return None
        src = self._token_table_sources()
        from . import optim as _optim
        sig = tuple((t.data_ptr(), t._version) for t in src) + (_optim.weights_epoch(),)
        st = self.__dict__.setdefault("_tok_state", {"sig": None, "seen": 0, "table": None})
        if st["sig"] != sig:
            st.update(sig=sig, seen=1, table=None)
        else:
            st["seen"] += 1
        if st["table"] is None and (mode == "1" or st["seen"] >= 2):
            lib = _lib.load()
            dev = self.fc.weight.device
            table = torch.empty(self._entry(lib, "token_table_bytes")(C.byref(dims)) // 4, dtype=torch.float32, device=dev)
            ws = torch.empty(self._entry(lib, "token_table_workspace_bytes")(C.byref(dims)), dtype=torch.uint8, device=dev)
            w = self._weights()
            check(self._entry(lib, "build_token_table")(C.byref(w), C.byref(dims), ptr(table), ptr(ws), ws.numel(),
                                                        stream_of(dev)), "set_%s_build_token_table" % self._ABI)
            torch.cuda.current_stream(dev).synchronize()        # other streams may use the table next
            st["table"] = table
            st["check"] = torch.stack([t.detach().double().sum() for t in src]).cpu()
        if st["table"] is not None and os.environ.get("SET_TOKEN_TABLE_VERIFY") == "1":
            now = torch.stack([t.detach().double().sum() for t in src]).cpu()
            if not torch.equal(now, st["check"]):
                raise _lib.SetError("token table is stale: a source weight changed without bumping tensor._version "
                                    "(in-place .data write?); call %s.invalidate_token_table()" % self._HANDLE)
        return st["table"]

    def _dims_key(self, dims):
        return tuple(getattr(dims, f) for f, _ in self._DIMS_CLS._fields_) + (str(self.fc.weight.device),)

    def _new_workspace(self, dims):
        """A fresh workspace for `dims` on the parameters' device; dims the library does not take are refused here."""
        dev = self.fc.weight.device
        n = self._entry(_lib.load(), "workspace_bytes")(C.byref(dims))
        if n == 0:
            key = self._dims_key(dims) + (torch.cuda.current_stream(dev).cuda_stream,)
            raise _lib.SetError("unsupported %s dims %r%s" % (self._DISPLAY, key, self._DIMS_HINT))
        return torch.empty(n, dtype=torch.uint8, device=dev)

    def _workspace(self, dims):
        """One workspace per (dims, device, stream): concurrent decodes on different streams (the self-critical step runs
        the greedy baseline on a side stream underneath the sampled rollout) must not share recurrent state or split-K
        slabs."""
        key = self._dims_key(dims) + (torch.cuda.current_stream(self.fc.weight.device).cuda_stream,)
        cache = self.__dict__.setdefault("_ws_cache", {})
        ws = cache.get(key)
        if ws is None:
            if len(cache) >= 24:             # (before the allocation: the freed blocks can serve it)
                cache.clear()
            ws = cache[key] = self._new_workspace(dims)
        self._ws, self._ws_key = ws, key
        return ws

    def ws_tensor(self, dims, name, shape, dtype=torch.float32, ws=None):
        """View of a named workspace tensor; `ws`: the workspace buffer (default: the one the last call used)."""
        ws = self._ws if ws is None else ws
        p = self._entry(_lib.load(), "ws_tensor")(C.byref(dims), ptr(ws), name.encode())
        if not p:
            raise KeyError(name)
        off = p - ws.data_ptr()
        return ws[off:off + math.prod(shape) * dtype.itemsize].view(dtype).view(*shape)

    def _row_limits_scope(self, lib, B):
        """Context manager: `row_limits` checked (here, before anything is set) against the B rows of the call and handed to
        the library for the enqueues inside the scope.  The limit pointer is thread-local state of the library that every
        greedy pick of this host thread reads: it is set for the duration of the caller's enqueue only (it used to stay set: a
        later caller with another B, or after the tensor was freed, would have read it)."""
        limits = self.row_limits
        if limits is not None:
            if limits.dtype != torch.int32 or not limits.is_cuda or limits.numel() != B:
                raise _lib.SetError("row_limits must be an int32 device tensor with one entry per row")
            limits = limits.contiguous()
        return _RowLimitsScope(lib, limits)


class _RowLimitsScope:
    """set_decode_row_limits(limits) on entry; cleared on exit only if one was set (a plain class: this sits on the latency
    path of every small-batch decode, and a generator-based context manager costs four times as much)"""
    __slots__ = ("lib", "limits")

    def __init__(self, lib, limits):
        self.lib, self.limits = lib, limits

    def __enter__(self):
        self.lib.set_decode_row_limits(ptr(self.limits))

    def __exit__(self, *exc):
        if self.limits is not None:
            self.lib.set_decode_row_limits(None)
