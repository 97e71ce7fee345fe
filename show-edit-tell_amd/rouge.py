"""ROUGE-L for validation, for consensus reranking and for the self-critical reward: coco-caption's `Rouge` (Lin, ACL 2004
workshop; beta = 1.2, as the COCO caption evaluation computes its `ROUGE_L`), restated here on token lists because the
reference's `evaluate()` returns `cocoEval.eval['ROUGE_L']` from an un-vendored scorer.  A sentence is a list of tokens; a
hypothesis h has a non-empty list of references R.

    lcs(h, r) = the length of the longest common subsequence of h and r
    P  = max over r of lcs(h, r) / len(h)
    Rc = max over r of lcs(h, r) / len(r)
    score = (1 + beta^2) * P * Rc / (Rc + beta^2 * P)  when P and Rc are non-zero, else 0     (double, in this order)
The corpus score is the MEAN of the sentence scores (not a score of summed statistics).  What coco leaves to a division by
zero: a hypothesis of no tokens scores 0; a reference of no tokens contributes recall 0 and precision 0.

Statistics of one hypothesis (integers) (lcs_p, len_h, lcs_r, len_r): lcs_p = the largest LCS over the set; (lcs_r, len_r) =
LCS and length of the reference of the largest recall, recalls compared exactly as fractions (cross-multiplied), of equal
recalls the first in set order; references with len_r = 0 are skipped unless all are empty: then (0, 0).  The score is a
function of these four integers alone: P = lcs_p / len_h, Rc = lcs_r / len_r.

`RougeL` is the pure-Python host scorer; `DeviceRougeL` the same numbers from id tensors in device memory
(csrc/rouge_device.hip, include/set_hip.h set_rouge_device_score) within the limits of device_metric.py, which also states what
counts as the sentence (shared with bleu.py and ciderd.py): without lengths a row is cut after its first 0 and the 0 stays a
token; with lengths the row is exactly that long.  The device scorer reads BLEU's prepared reference records: one
preparation serves both metrics.
"""
from __future__ import annotations

import numpy as np

from .device_metric import (DeviceSentenceScorer, HostSentenceScorer, PreparedRefs, RecordScorer, coco_pairs, cut_after_zero,
                            pack_ref_sets, resolve_device, strip_end)      # the unused ones: names this module has always exposed

BETA = 1.2
STATS_COLUMNS = 4                  # lcs_p, len_h, lcs_r, len_r


def lcs_length(a, b):
    """length of the longest common subsequence: the (len(a) + 1) x (len(b) + 1) table, one row at a time"""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


class RougeL(HostSentenceScorer):
    """The host scorer.  Pure Python: validation runs it once per epoch, and it is the readable statement that the device
    route is tested against.  score_token_ids (device_metric.HostSentenceScorer) returns (stats int64 (N, 4), scores (N,))."""
    STATS_COLUMNS = STATS_COLUMNS

    def __init__(self, beta=BETA):
        beta = float(beta)
        if not (beta > 0.0 and beta != float("inf")):
            raise ValueError("beta must be finite and positive, got %r" % (beta,))
        self.beta = beta

    @staticmethod
    def sentence_stats(hyp, refs):
        """the four integers of one hypothesis (a list of tokens) against its references (a list of such lists)"""
        hyp = list(hyp)
        lcs_p = lcs_r = len_r = 0
        for r in refs:
            r = list(r)
            l = lcs_length(hyp, r)
            lcs_p = max(lcs_p, l)
            if len(r) > 0 and (len_r == 0 or l * len_r > lcs_r * len(r)):        # a larger recall; the first of equal ones stays
                lcs_r, len_r = l, len(r)
        return [lcs_p, len(hyp), lcs_r, len_r]

    def score_from_stats(self, stats):
        """the sentence score from its four integers, a Python float"""
        lcs_p, len_h, lcs_r, len_r = (int(x) for x in stats)
        if lcs_p <= 0 or lcs_r <= 0 or len_h <= 0 or len_r <= 0:
            return 0.0
        beta2 = self.beta * self.beta
        P = float(lcs_p) / float(len_h)
        Rc = float(lcs_r) / float(len_r)
        return (1.0 + beta2) * P * Rc / (Rc + beta2 * P)

    _sentence_score = score_from_stats

    def compute_score(self, gts, res):
        """coco's call: gts = {image_id: [reference strings]}; res = {image_id: [one string]} or, as CiderD.compute_score takes
        it, [{'image_id': id, 'caption': [string]}].  Strings are split at whitespace.  Returns (the mean of the sentence
        scores, [per-sentence score])."""
        _, scores = self._score_lists(coco_pairs(gts, res))
        return (float(np.mean(scores)) if len(scores) else 0.0), scores.tolist()


# ---- the device route (csrc/rouge_device.hip, include/set_hip.h set_rouge_device_score) --------------------------------------
class DeviceRougeL(RecordScorer):
    """ROUGE-L on one device: every call is enqueued on the current stream of that device and reads nothing back.  Stateless
    on the native side: an instance remembers its device and beta.  prepare_refs, score_token_ids (stats int32 (N, 4), scores
    float64 (N,)) and pair_scores are device_metric.RecordScorer's: the records are BLEU's."""
    METRIC = "ROUGE-L"
    NATIVE = ("set_bleu_device_prepare", "set_rouge_device_score")
    SCORE_ENTRY = "set_rouge_device_score"
    STATS_COLUMNS = STATS_COLUMNS

    def __init__(self, dev, beta=BETA):
        super().__init__(dev)
        self.beta = RougeL(beta).beta

    def _extra(self):
        return (self.beta,)

    def corpus_score(self, hyps, hyp_set, refs, hyp_lens=None):
        """ROUGE_L of the corpus: the mean of the rows' scores, taken on the device (no row: 0).  Returns a 0-d float64 device
        tensor; nothing is read back."""
        scores = self.score_token_ids(hyps, hyp_set, refs, hyp_lens)[1]
        return scores.mean() if scores.numel() else scores.new_zeros(())


def device_scorer(dev):
    """the DeviceRougeL (beta = 1.2) of `dev`, made at the first call"""
    return DeviceRougeL.of_device(dev)
