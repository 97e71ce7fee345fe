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

from .device_metric import (DEVICE_MAX_LEN, DEVICE_PACK_LIMIT, DeviceSentenceScorer, HostSentenceScorer,
                            PreparedRefs as PreparedBleuRefs, RecordScorer, coco_pairs, cut_after_zero, pack_ref_sets, resolve_device,
                            strip_end)      # the unused ones: names this module has always exposed

TINY, SMALL = 1e-15, 1e-9
STATS_COLUMNS = 10                 # correct[1..4], guess[1..4], testlen, reflen


def _grams(words, k):
    return Counter(tuple(words[i:i + k]) for i in range(len(words) - k + 1))


class Bleu(HostSentenceScorer):
    """The host scorer.  Pure Python: validation runs it once per epoch, and it is the readable statement that the device
    route is tested against.  score_token_ids (device_metric.HostSentenceScorer) returns (stats int64 (N, 10), scores (N, 4))."""
    STATS_COLUMNS = STATS_COLUMNS
    SCORE_SHAPE = (4,)

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

    _sentence_score = scores_from_stats

    def compute_score(self, gts, res):
        """coco's call: gts = {image_id: [reference strings]}; res = {image_id: [one string]} or, as CiderD.compute_score takes
        it, [{'image_id': id, 'caption': [string]}].  Strings are split at whitespace.  Returns ([Bleu_1..4 of the corpus],
        [[per-sentence Bleu_k] for k in 1..4])."""
        stats, scores = self._score_lists(coco_pairs(gts, res))
        return self.corpus_from_stats(stats), [scores[:, k].tolist() for k in range(4)]


# ---- the device route (csrc/bleu_device.hip, include/set_hip.h set_bleu_device_*) --------------------------------------------
class DeviceBleu(RecordScorer):
    """BLEU on one device: every call is enqueued on the current stream of that device and reads nothing back.  Stateless on
    the native side (there is no table): an instance only remembers its device.  prepare_refs, score_token_ids (stats int32
    (N, 10), scores float64 (N, 4), pairs: the sentence BLEU-4) and pair_scores are device_metric.RecordScorer's."""
    METRIC = "BLEU"
    NATIVE = ("set_bleu_device_ref_bytes", "set_bleu_device_prepare", "set_bleu_device_score")
    SCORE_ENTRY = "set_bleu_device_score"
    STATS_COLUMNS = STATS_COLUMNS
    SCORE_SHAPE = (4,)

    def corpus_score(self, hyps, hyp_set, refs, hyp_lens=None):
        """Bleu_1..4 of the corpus: the rows' statistics summed as int64 on the device, the formula in double there.
        Returns a (4,) float64 device tensor; nothing is read back."""
        return Bleu.corpus_from_stats(self.score_token_ids(hyps, hyp_set, refs, hyp_lens)[0])


def device_scorer(dev):
    """the DeviceBleu of `dev`, made at the first call"""
    return DeviceBleu.of_device(dev)
