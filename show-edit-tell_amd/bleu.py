"""BLEU for validation and for the self-critical reward: coco-caption's `BleuScorer` with n = 4 and option "closest"
(Papineni et al., ACL 2002, as the COCO caption evaluation computes it), restated here because the reference's `evaluate()`
returns `cocoEval.eval['Bleu_4']` from an un-vendored scorer.  A sentence is a list of tokens; a hypothesis h has a non-empty
list of references R.

Statistics of one hypothesis (integers), k = 1..4:
    guess[k]   = max(0, len(h) - k + 1)
    correct[k] = sum over the distinct k-grams g of h: min(count_h(g), max over r in R of count_r(g))
    testlen    = len(h)
    reflen     = the len(r) that minimises (|len(r) - testlen|, len(r)): the closest, of two equally close the shorter
Score from statistics — of one sentence, or of a corpus from the statistics summed over its hypotheses — in double:
    b = 1;  for k in 1..4:  b *= (correct[k] + 1e-15) / (guess[k] + 1e-9);  bleu[k] = b ** (1 / k)
    ratio = (testlen + 1e-15) / (reflen + 1e-9);  if ratio < 1: bleu[k] *= exp(1 - 1 / ratio)
so identical hypothesis and reference score a hair under 1 and guess[k] = 0 contributes a factor 1e-6: coco's behaviour.

`Bleu` is the pure-Python host scorer; `DeviceBleu` the same numbers from id tensors in device memory (csrc/bleu_device.hip,
include/set_hip.h set_bleu_device_*) within the limits of device_metric.py, which also states what counts as the sentence
(shared with ciderd.py): without lengths a row is cut after its first 0 and the 0 stays a token (the SCST convention: <end> is
rewarded); with lengths the row is exactly that long (validation passes the position of the first 0: <end> is no token, as in
cocoEval's word strings).
"""
from __future__ import annotations

import math
from collections import Counter

import numpy as np

from .device_metric import (DEVICE_MAX_LEN, DEVICE_PACK_LIMIT, DeviceSentenceScorer, PreparedRefs as PreparedBleuRefs, cut_after_zero,
                            pack_ref_sets, resolve_device, strip_end)

TINY, SMALL = 1e-15, 1e-9
STATS_COLUMNS = 10                 # correct[1..4], guess[1..4], testlen, reflen


def _grams(words, k):
    return Counter(tuple(words[i:i + k]) for i in range(len(words) - k + 1))


class Bleu:
    """The host scorer.  Pure Python: validation runs it once per epoch, and it is the readable statement that the device
    route is tested against."""

    def __init__(self, n=4):
        if int(n) != 4:
            raise ValueError("Bleu scores the orders 1..4 (coco's n = 4), got n = %r" % (n,))
        self.n = 4

    @staticmethod
    def sentence_stats(hyp, refs):
        """the ten integers of one hypothesis (a list of tokens) against its references (a list of such lists)"""
        hyp = list(hyp)
        ref_counts = [[_grams(list(r), k) for r in refs] for k in range(1, 5)]
        correct = []
        for k in range(1, 5):
            c = 0
            for g, ch in _grams(hyp, k).items():
                c += min(ch, max([rc[g] for rc in ref_counts[k - 1]] + [0]))
            correct.append(c)
        guess = [max(0, len(hyp) - k + 1) for k in range(1, 5)]
        reflen = min(((abs(len(r) - len(hyp)), len(r)) for r in refs), default=(0, 0))[1]
        return correct + guess + [len(hyp), reflen]

    @staticmethod
    def scores_from_stats(stats):
        """bleu[1..4] from ten numbers (a sentence's, or the corpus sum), Python floats"""
        s = [float(x) for x in stats]
        b, out = 1.0, []
        for k in range(1, 5):
            b *= (s[k - 1] + TINY) / (s[3 + k] + SMALL)
            out.append(b ** (1.0 / k))
        ratio = (s[8] + TINY) / (s[9] + SMALL)
        if ratio < 1.0:
            f = math.exp(1.0 - 1.0 / ratio)
            out = [x * f for x in out]
        return out

    @staticmethod
    def corpus_from_stats(stats):
        """The four corpus scores from per-sentence statistics (N, 10): the statistics are SUMMED, then scored (not the mean
        of the sentence scores).  numpy / lists -> a list of 4 floats; a torch tensor -> a (4,) float64 tensor on its device,
        computed there (nothing is read back)."""
        try:
            import torch
        except ImportError:                                       # numpy-only use
            torch = None
        if torch is not None and torch.is_tensor(stats):
            s = stats.reshape(-1, STATS_COLUMNS).to(torch.int64).sum(0).to(torch.float64)
            b = torch.cumprod((s[0:4] + TINY) / (s[4:8] + SMALL), 0)
            out = b ** (1.0 / torch.arange(1, 5, dtype=torch.float64, device=s.device))
            ratio = (s[8] + TINY) / (s[9] + SMALL)
            f = torch.where(ratio < 1.0, torch.exp(1.0 - 1.0 / ratio), torch.ones_like(ratio))
            return out * f
        s = np.asarray(stats, dtype=np.int64).reshape(-1, STATS_COLUMNS).sum(0)
        return Bleu.scores_from_stats([int(x) for x in s])

    def _score_lists(self, pairs):
        """pairs: iterable of (hypothesis token list, list of reference token lists) -> (stats (N, 10) int64, scores (N, 4))"""
        pairs = list(pairs)
        stats = np.zeros((len(pairs), STATS_COLUMNS), dtype=np.int64)
        scores = np.zeros((len(pairs), 4), dtype=np.float64)
        for i, (h, refs) in enumerate(pairs):
            if not len(refs):
                raise ValueError("hypothesis %d has no reference" % i)
            stats[i] = self.sentence_stats(h, refs)
            scores[i] = self.scores_from_stats(stats[i])
        return stats, scores

    def compute_score(self, gts, res):
        """coco's call: gts = {image_id: [reference strings]}; res = {image_id: [one string]} or, as CiderD.compute_score takes
        it, [{'image_id': id, 'caption': [string]}].  Strings are split at whitespace.  Returns ([Bleu_1..4 of the corpus],
        [[per-sentence Bleu_k] for k in 1..4])."""
        if isinstance(res, dict):
            res = [{'image_id': k, 'caption': v} for k, v in res.items()]
        pairs = []
        for r in res:
            cap = r['caption']
            cap = cap[0] if isinstance(cap, (list, tuple)) else cap
            pairs.append((cap.split(), [s.split() for s in gts[r['image_id']]]))
        stats, scores = self._score_lists(pairs)
        return self.corpus_from_stats(stats), [scores[:, k].tolist() for k in range(4)]

    def score_token_ids(self, hyps, hyp_set, ref_sets, hyp_lens=None):
        """`hyps` (N, L) ids, `hyp_set` (N,) index of each row's reference set, `ref_sets` = list of reference sets, each a
        list of id lists (as ciderd.ground_truth_lists returns them; cut after their first 0).  hyp_lens=None: a row is cut
        after its first 0 and the 0 stays (no 0: the whole row); else (N,) lengths, clamped to [0, L].
        Returns (stats int64 (N, 10), scores float64 (N, 4))."""
        hyps = np.asarray(hyps.cpu() if hasattr(hyps, 'cpu') else hyps, dtype=np.int64)
        if hyps.ndim != 2:
            raise ValueError("sentences are rows of a 2-D id array, got shape %s" % (hyps.shape,))
        N, L = hyps.shape
        hyp_set = np.asarray(hyp_set.cpu() if hasattr(hyp_set, 'cpu') else hyp_set).reshape(-1)
        if hyp_set.shape[0] != N:
            raise ValueError("hyp_set has %d entries for %d sentences" % (hyp_set.shape[0], N))
        if hyp_lens is not None:
            hyp_lens = np.asarray(hyp_lens.cpu() if hasattr(hyp_lens, 'cpu') else hyp_lens).reshape(-1)
            if hyp_lens.shape[0] != N:
                raise ValueError("hyp_lens has %d entries for %d sentences" % (hyp_lens.shape[0], N))
        refs = [[cut_after_zero(c) for c in rs] for rs in ref_sets]
        pairs = []
        for i in range(N):
            row = hyps[i].tolist()
            row = cut_after_zero(row) if hyp_lens is None else row[:min(max(int(hyp_lens[i]), 0), L)]
            pairs.append((row, refs[int(hyp_set[i])]))
        return self._score_lists(pairs)


# ---- the device route (csrc/bleu_device.hip, include/set_hip.h set_bleu_device_*) --------------------------------------------
class DeviceBleu(DeviceSentenceScorer):
    """BLEU on one device: every call is enqueued on the current stream of that device and reads nothing back.  Stateless on
    the native side (there is no table): an instance only remembers its device."""
    METRIC = "BLEU"

    def __init__(self, dev):
        from . import _lib
        super().__init__(dev)
        for name in ("set_bleu_device_ref_bytes", "set_bleu_device_prepare", "set_bleu_device_score"):
            if name in _lib.MISSING:
                raise _lib.SetError("the native library does not export %s" % name)

    def _prepare(self, t, ln):
        """(R, L) device ids [+ (R,) device int32 lengths] -> the record buffer"""
        import torch
        from . import _lib
        R, L = t.shape
        recs = torch.empty(R * (8 + 4 * L), dtype=torch.int64, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = self._lib.set_bleu_device_prepare(t.data_ptr(), t.stride(0), None if ln is None else ln.data_ptr(), R, L,
                                                   recs.data_ptr(), _lib.stream_of(self.dev))
        _lib.check(rc, "set_bleu_device_prepare")
        return recs

    def prepare_refs(self, ref_sets, count_end=True):
        """Reference sets as ciderd.ground_truth_lists returns them (per image a list of id lists) -> PreparedBleuRefs: one
        upload and one launch, independent of the rollout (issue it first and it runs underneath).  References are cut after
        their first 0 (count_end=False: before it, the validation convention).  An empty set or a reference longer than 64
        ids is refused."""
        import torch
        sets = strip_end(ref_sets) if not count_end else [[cut_after_zero(c) for c in refs] for refs in ref_sets]
        tok, ln, off, R, L, max_set = pack_ref_sets(sets, self.METRIC, False)
        t, l = torch.from_numpy(tok[:R]).to(self.dev), torch.from_numpy(ln[:R]).to(self.dev)
        # the upload stays with the records: the corpus CIDEr of the same sets is built from it (ciderd.DeviceCiderD.from_refs)
        return PreparedBleuRefs(self._prepare(t, l), L, R, torch.from_numpy(off).to(self.dev), len(sets), max_set, t, l, ln[:R])

    def score_token_ids(self, hyps, hyp_set, refs, hyp_lens=None, return_pairs=False):
        """Device twin of Bleu.score_token_ids: `hyps` (N, L) ids, `hyp_set` (N,) index of each row's reference set, `refs` a
        PreparedBleuRefs (or reference sets, prepared here), hyp_lens as on the host.  Returns device tensors (stats int32
        (N, 10), scores float64 (N, 4)); return_pairs=True: also (N, max set size) float64 with the sentence BLEU-4 against
        every single reference of the set (columns beyond a smaller set stay 0)."""
        import torch
        from . import _lib
        if not isinstance(refs, PreparedBleuRefs):
            refs = self.prepare_refs(refs)
        t = self._tokens(hyps)
        N, L = t.shape
        so = self._i32(hyp_set, N, "hyp_set")
        ln = self._i32(hyp_lens, N, "hyp_lens")
        stats = torch.empty(N, STATS_COLUMNS, dtype=torch.int32, device=self.dev)
        scores = torch.empty(N, 4, dtype=torch.float64, device=self.dev)
        pair_ld = max(1, refs.max_set)
        pairs = torch.zeros(N, pair_ld, dtype=torch.float64, device=self.dev) if return_pairs else None
        with torch.cuda.device(self.dev):
            rc = self._lib.set_bleu_device_score(
                t.data_ptr(), t.stride(0), None if ln is None else ln.data_ptr(), N, L, so.data_ptr(), refs.recs.data_ptr(),
                refs.L, refs.n_refs, refs.set_off.data_ptr(), refs.n_sets, refs.max_set, stats.data_ptr(), scores.data_ptr(),
                None if pairs is None else pairs.data_ptr(), pair_ld, _lib.stream_of(self.dev))
        _lib.check(rc, "set_bleu_device_score")
        return (stats, scores, pairs) if return_pairs else (stats, scores)

    def corpus_score(self, hyps, hyp_set, refs, hyp_lens=None):
        """Bleu_1..4 of the corpus: the rows' statistics summed as int64 on the device, the formula in double there.
        Returns a (4,) float64 device tensor; nothing is read back."""
        return Bleu.corpus_from_stats(self.score_token_ids(hyps, hyp_set, refs, hyp_lens)[0])

    def pair_scores(self, candidates, n_per_image):
        """(NI * n, L) candidates, n per image -> (NI * n, n): the sentence BLEU-4 of row i against candidate r of its own
        image as the only reference (what evaluate.consensus_rerank reads).  Rows are cut after their first 0; the candidates
        are prepared once on the device and serve as references."""
        t = self._tokens(candidates)
        refs, owner = self._self_refs(t, n_per_image)
        refs.recs = self._prepare(t, None)
        return self.score_token_ids(t, owner, refs, return_pairs=True)[2]


_device_scorers = {}


def device_scorer(dev):
    """the DeviceBleu of `dev`, made at the first call"""
    dev = resolve_device(dev)
    if dev not in _device_scorers:
        _device_scorers[dev] = DeviceBleu(dev)
    return _device_scorers[dev]
