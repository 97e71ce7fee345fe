"""What the device metrics share on the Python side (ciderd.DeviceCiderD, bleu.DeviceBleu): the two limits and the 0 rule of
csrc/ngram_wave.h, the flattening of reference sets into one padded upload, the prepared-reference record and the tensor
plumbing of a scorer that lives on one device.  numpy only at import: torch is imported where a device is touched, so the
numpy-only use of `bleu` and `ciderd` keeps working.

A sentence is at most DEVICE_MAX_LEN ids (one wave holds it, one position per lane) and every id lies in [0, DEVICE_PACK_LIMIT)
(four ids + 1 in the 16-bit fields of one 64-bit key).  What counts as the sentence: without lengths a row is cut after its
first 0 and the 0 stays a token (the SCST convention: <end> is rewarded); with lengths the row is exactly that long (validation
passes the position of the first 0: <end> is no token).
"""
from __future__ import annotations

import numpy as np

DEVICE_PACK_LIMIT = 65534
DEVICE_MAX_LEN = 64


def cut_after_zero(c):
    """the list cut AFTER its first 0 (the 0 stays a token); no 0: the whole list"""
    c = [int(w) for w in c]
    return c[:c.index(0) + 1] if 0 in c else c


def strip_end(ref_sets):
    """reference sets with every list cut BEFORE its first 0: <end> is not a token (the validation convention)"""
    out = []
    for refs in ref_sets:
        cut = []
        for c in refs:
            c = [int(w) for w in c]
            cut.append(c[:c.index(0)] if 0 in c else c)
        out.append(cut)
    return out


class PreparedRefs:
    """Reference sets prepared on the device (prepare_refs of a device scorer): the records in that metric's layout, their row
    length, the set offsets (device int64, n_sets + 1) and the host-side counts the score call validates with.  A scorer may
    keep the upload the records were made from — tokens (n_refs, L) int64 and lens (n_refs,) int32 on the device, host_lens the
    same lengths as numpy — so that another metric of the same corpus need not upload it again (ciderd.DeviceCiderD.from_refs)."""
    def __init__(self, recs, L, n_refs, set_off, n_sets, max_set, tokens=None, lens=None, host_lens=None):
        self.recs, self.L, self.n_refs, self.set_off, self.n_sets, self.max_set = recs, L, n_refs, set_off, n_sets, max_set
        self.tokens, self.lens, self.host_lens = tokens, lens, host_lens


def pack_ref_sets(sets, metric_name, allow_empty):
    """Reference sets (per image a list of id lists, already cut by cut_after_zero or strip_end) -> (tok (max(1, R), L) int64
    zero-padded, lens (max(1, R),) int32, off (n_sets + 1,) int64 set offsets, R, L, max_set): the input of one upload.  The
    arrays keep one padded row when there is no reference at all.  ValueError: an empty set where the metric needs a reference
    (allow_empty=False), a reference longer than DEVICE_MAX_LEN."""
    if not allow_empty:
        for i, refs in enumerate(sets):
            if not len(refs):
                raise ValueError("reference set %d is empty: %s needs at least one reference per hypothesis" % (i, metric_name))
    flat = [c for refs in sets for c in refs]
    L = max([1] + [len(c) for c in flat])
    if L > DEVICE_MAX_LEN:
        raise ValueError("a reference of %d ids: the device %s scorer takes at most %d" % (L, metric_name, DEVICE_MAX_LEN))
    R = len(flat)
    tok = np.zeros((max(1, R), L), dtype=np.int64)
    lens = np.zeros(max(1, R), dtype=np.int32)
    for i, c in enumerate(flat):
        tok[i, :len(c)] = c
        lens[i] = len(c)
    off = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in sets], out=off[1:])
    return tok, lens, off, R, L, max([0] + [len(r) for r in sets])


def resolve_device(dev):
    """torch.device(dev), a bare "cuda" resolved to the current device's index (the key of the per-device scorer caches)"""
    import torch
    dev = torch.device(dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class DeviceSentenceScorer:
    """Base of a metric's scorer on one device: the device, and id / index tensors in the form the native calls take.
    A subclass names its metric and keeps prepare_refs, score_token_ids, pair_scores and its native calls."""
    METRIC = None

    def __init__(self, dev):
        from . import _lib
        self.dev = resolve_device(dev)
        if self.dev.type != "cuda":
            raise _lib.SetError("the device %s scorer needs a GPU device, got %s" % (self.METRIC, self.dev))
        self._lib = _lib.load()

    def _tokens(self, t):
        """sentences -> (S, L >= 1) int64 on the device, unit stride along a row"""
        import torch
        from . import _lib
        t = torch.as_tensor(t)
        if t.dim() != 2:
            raise ValueError("sentences are rows of a 2-D id tensor, got shape %s" % (tuple(t.shape),))
        t = t.to(self.dev, torch.int64)
        if t.shape[1] == 0:
            t = t.new_zeros(t.shape[0], 1)
        if t.shape[1] > DEVICE_MAX_LEN:
            raise _lib.SetError("the device %s scorer takes sentences of at most %d ids, got rows of %d"
                                % (self.METRIC, DEVICE_MAX_LEN, t.shape[1]))
        return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()

    def _i32(self, x, n, what):
        import torch
        if x is None:
            return None
        x = torch.as_tensor(x).reshape(-1).to(self.dev, torch.int32).contiguous()
        if x.numel() != n:
            raise ValueError("%s has %d entries for %d sentences" % (what, x.numel(), n))
        return x

    def _self_refs(self, t, n_per_image):
        """(NI * n, L) candidates, n per image, as each other's references: (PreparedRefs whose set s holds the n rows of image
        s — `recs` left for the subclass to fill with the rows' records —, (NI * n,) int32 owner set of every row)"""
        import torch
        n = int(n_per_image)
        if n < 1 or t.shape[0] % n:
            raise ValueError("%d candidates are not %d per image" % (t.shape[0], n))
        NI = t.shape[0] // n
        off = torch.arange(0, (NI + 1) * n, n, dtype=torch.int64, device=self.dev)
        owner = torch.arange(NI, dtype=torch.int32, device=self.dev).repeat_interleave(n)
        return PreparedRefs(None, t.shape[1], NI * n, off, NI, n), owner
