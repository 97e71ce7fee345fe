"""Word edit distance: how far a caption is from a reference in words, and which edit turned one word sequence into another —
the measure of HOW MUCH an editing model edited.  A sentence is a list of tokens; a hypothesis h has a non-empty list of
references R.

    d(h, r)   = the unit-cost Levenshtein distance: substitution, insertion and deletion cost 1 each
    sim(h, r) = (m - d) / m with m = max(len(h), len(r)), one double division of two integers; 1.0 when both are empty
Against a set the reference of the largest similarity is chosen: similarities compared exactly as fractions (cross-multiplied,
empty against empty as 1/1), of equal ones the first in set order.  Statistics of one hypothesis (integers)
(dist, len_h, len_r, ref), ref = the chosen reference's position in its set; the score is sim of those integers alone.
Corpus: `similarity` = the MEAN of the sentence scores; `wer` = sum dist / sum len_r over the chosen references (0 when that sum
is 0), the word error rate.

`alignment(src, hyp)` is the canonical edit script that turns src into hyp, read off the full table D[i][j] (i over src, j over
hyp) from (len(src), len(hyp)) backwards; at every cell the first rule that applies is taken:
    1. i > 0, j > 0, src[i-1] == hyp[j-1] and D[i][j] == D[i-1][j-1]:  keep
    2. i > 0, j > 0 and D[i][j] == D[i-1][j-1] + 1:                    substitute
    3. j > 0 and D[i][j] == D[i][j-1] + 1:                             insert (hyp[j-1] has no source word)
    4. otherwise:                                                      delete src[i-1]
so keep + sub + ins == len(hyp), keep + sub + del == len(src) and sub + ins + del == d.

`EditDistance` is the pure-Python host scorer; `DeviceEditDistance` the same numbers from id tensors in device memory
(csrc/editdist_device.hip, include/set_hip.h set_edit_device_score / set_edit_device_align) within the limits of
device_metric.py, which also states what counts as the sentence (shared with bleu.py, rouge.py and ciderd.py): without lengths
a row is cut after its first 0 and the 0 stays a token; with lengths the row is exactly that long.  The device scorer reads
BLEU's prepared reference records: one preparation serves all three metrics.  Not built: weighted costs, transpositions,
sentences above 64 ids on the device, a self-critical reward term.
"""
from __future__ import annotations

import numpy as np

from .device_metric import (DeviceSentenceScorer, HostSentenceScorer, PreparedRefs, RecordScorer, cut_after_zero, id_rows,
                            resolve_device)
from .rouge import DeviceRougeL      # noqa: F401  (names this module has always exposed)

STATS_COLUMNS = 4                  # dist, len_h, len_r, ref
ALIGN_COLUMNS = 8                  # dist, len_h, len_s, keep, sub, ins, del, unchanged
KEEP, SUB, INS, DEL = 1, 2, 3, 3   # op codes: per hypothesis position keep / substitute / insert, per source position kept / substituted / deleted
OP_NAMES = {KEEP: "keep", SUB: "substitute", INS: "insert"}


def distance_table(a, b):
    """D[i][j] = distance of a[:i] and b[:j]: the (len(a) + 1) x (len(b) + 1) table"""
    D = [list(range(len(b) + 1))]
    for i, x in enumerate(a):
        row = [i + 1]
        for j, y in enumerate(b):
            row.append(min(D[i][j] + (0 if x == y else 1), D[i][j + 1] + 1, row[j] + 1))
        D.append(row)
    return D


def distance(a, b):
    """unit-cost Levenshtein distance of two token lists, one table row at a time"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a):
        cur = [i + 1]
        for j, y in enumerate(b):
            cur.append(min(prev[j] + (0 if x == y else 1), prev[j + 1] + 1, cur[j] + 1))
        prev = cur
    return prev[len(b)]


def similarity(dist, len_h, len_r):
    m = max(int(len_h), int(len_r))
    return 1.0 if m <= 0 else float(m - int(dist)) / float(m)


def alignment(src, hyp):
    """The canonical edit script from src to hyp (module docstring) -> (hyp_ops: per hypothesis position 1 keep / 2 substitute /
    3 insert; hyp_src: per hypothesis position the aligned source position or -1; src_ops: per source position 1 kept /
    2 substituted / 3 deleted; (keep, sub, ins, del))."""
    src, hyp = list(src), list(hyp)
    D = distance_table(src, hyp)
    i, j = len(src), len(hyp)
    hyp_ops, hyp_src, src_ops = [0] * j, [-1] * j, [0] * i
    keep = sub = ins = dele = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and src[i - 1] == hyp[j - 1] and D[i][j] == D[i - 1][j - 1]:
            hyp_ops[j - 1], hyp_src[j - 1], src_ops[i - 1] = KEEP, i - 1, KEEP
            keep, i, j = keep + 1, i - 1, j - 1
        elif i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + 1:
            hyp_ops[j - 1], hyp_src[j - 1], src_ops[i - 1] = SUB, i - 1, SUB
            sub, i, j = sub + 1, i - 1, j - 1
        elif j > 0 and D[i][j] == D[i][j - 1] + 1:
            hyp_ops[j - 1] = INS
            ins, j = ins + 1, j - 1
        else:
            src_ops[i - 1] = DEL
            dele, i = dele + 1, i - 1
    return hyp_ops, hyp_src, src_ops, (keep, sub, ins, dele)


class EditDistance(HostSentenceScorer):
    """The host scorer.  Pure Python: the readable statement that the device route is tested against.  score_token_ids
    (device_metric.HostSentenceScorer) returns (stats int64 (N, 4), scores (N,))."""
    STATS_COLUMNS = STATS_COLUMNS
    LENS_CHECKED_FIRST = True

    @staticmethod
    def sentence_stats(hyp, refs):
        """the four integers of one hypothesis (a list of tokens) against its references (a list of such lists)"""
        hyp = list(hyp)
        best = None                                                # (numerator, denominator) of the chosen similarity
        out = [len(hyp), len(hyp), 0, -1]
        for k, r in enumerate(refs):
            r = list(r)
            d, m = distance(hyp, r), max(len(hyp), len(r))
            num, den = (m - d, m) if m > 0 else (1, 1)
            if best is None or num * best[1] > best[0] * den:      # a larger similarity; the first of equal ones stays
                best, out = (num, den), [d, len(hyp), len(r), k]
        return out

    @staticmethod
    def score_from_stats(stats):
        """the sentence score from its four integers, a Python float"""
        return similarity(stats[0], stats[1], stats[2])

    _sentence_score = score_from_stats

    def corpus_score(self, hyps, hyp_set, ref_sets, hyp_lens=None):
        """{'similarity': the mean of the rows' scores, 'wer': sum dist / sum len_r of the chosen references} (no row, or no
        reference word: 0), Python floats"""
        stats, scores = self.score_token_ids(hyps, hyp_set, ref_sets, hyp_lens)
        words = int(stats[:, 2].sum())
        return {"similarity": float(np.mean(scores)) if len(scores) else 0.0,
                "wer": float(int(stats[:, 0].sum())) / float(words) if words > 0 else 0.0}

    def align_token_ids(self, hyps, srcs, hyp_lens=None, src_lens=None):
        """Row i of `hyps` (N, L) against row i of `srcs` (N, Ls), lengths as in score_token_ids -> (stats int64 (N, 8) = dist,
        len_h, len_s, keep, sub, ins, del, unchanged; hyp_ops int8 (N, L); hyp_src int32 (N, L), -1 where there is none;
        src_ops int8 (N, Ls)); positions at and beyond a sentence's length hold op 0 and source -1."""
        H, S = id_rows(hyps, hyp_lens, "hyp_lens"), id_rows(srcs, src_lens, "src_lens")
        if len(H) != len(S):
            raise ValueError("%d hypotheses for %d sources" % (len(H), len(S)))
        N, L, Ls = len(H), np.shape(hyps)[1], np.shape(srcs)[1]
        stats = np.zeros((N, ALIGN_COLUMNS), dtype=np.int64)
        hyp_ops, hyp_src = np.zeros((N, L), dtype=np.int8), np.full((N, L), -1, dtype=np.int32)
        src_ops = np.zeros((N, Ls), dtype=np.int8)
        for i, (h, s) in enumerate(zip(H, S)):
            ho, hs, so, (keep, sub, ins, dele) = alignment(s, h)
            d = distance(h, s)
            stats[i] = [d, len(h), len(s), keep, sub, ins, dele, 1 if d == 0 else 0]
            hyp_ops[i, :len(h)], hyp_src[i, :len(h)], src_ops[i, :len(s)] = ho, hs, so
        return stats, hyp_ops, hyp_src, src_ops


# ---- the device route (csrc/editdist_device.hip, include/set_hip.h set_edit_device_score / set_edit_device_align) ------------
class DeviceEditDistance(RecordScorer):
    """Word edit distance on one device: every call is enqueued on the current stream of that device and reads nothing back.
    Stateless on the native side.  prepare_refs, score_token_ids (stats int32 (N, 4), scores float64 (N,)) and pair_scores are
    device_metric.RecordScorer's: the records are BLEU's."""
    METRIC = "edit distance"
    NATIVE = ("set_bleu_device_prepare", "set_edit_device_score", "set_edit_device_align")
    SCORE_ENTRY = "set_edit_device_score"
    STATS_COLUMNS = STATS_COLUMNS

    def corpus_score(self, hyps, hyp_set, refs, hyp_lens=None):
        """{'similarity', 'wer'} of the corpus as 0-d float64 device tensors, reduced on the device (no row, or no reference
        word: 0; a refused row makes both NaN); nothing is read back."""
        import torch
        stats, scores = self.score_token_ids(hyps, hyp_set, refs, hyp_lens)
        if not scores.numel():
            return {"similarity": scores.new_zeros(()), "wer": scores.new_zeros(())}
        dist, words = stats[:, 0].sum().double(), stats[:, 2].sum().double()
        wer = torch.where(words > 0, dist / torch.where(words > 0, words, torch.ones_like(words)), torch.zeros_like(words))
        wer = torch.where((stats[:, 1] < 0).any(), torch.full_like(wer, float("nan")), wer)
        return {"similarity": scores.mean(), "wer": wer}

    def align_token_ids(self, hyps, srcs, hyp_lens=None, src_lens=None):
        """Device twin of EditDistance.align_token_ids: row i of `hyps` (N, L) against row i of `srcs` (N, Ls).  Returns device
        tensors (stats int32 (N, 8), hyp_ops int8 (N, L), hyp_src int32 (N, L), src_ops int8 (N, Ls)).  A row with an id outside
        [0, 65534) inside a sentence: stats -1, ops 0, sources -1."""
        import torch
        from . import _lib
        h, s = self._tokens(hyps), self._tokens(srcs)
        N, L = h.shape
        Ls = s.shape[1]
        if s.shape[0] != N:
            raise ValueError("%d hypotheses for %d sources" % (N, s.shape[0]))
        hl, sl = self._i32(hyp_lens, N, "hyp_lens"), self._i32(src_lens, N, "src_lens")
        stats = torch.empty(N, ALIGN_COLUMNS, dtype=torch.int32, device=self.dev)
        hyp_ops = torch.empty(N, L, dtype=torch.int8, device=self.dev)
        hyp_src = torch.empty(N, L, dtype=torch.int32, device=self.dev)
        src_ops = torch.empty(N, Ls, dtype=torch.int8, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = self._lib.set_edit_device_align(
                h.data_ptr(), h.stride(0), None if hl is None else hl.data_ptr(), N, L, s.data_ptr(), s.stride(0),
                None if sl is None else sl.data_ptr(), Ls, stats.data_ptr(), hyp_ops.data_ptr(), L, hyp_src.data_ptr(),
                src_ops.data_ptr(), Ls, _lib.stream_of(self.dev))
        _lib.check(rc, "set_edit_device_align")
        return stats, hyp_ops, hyp_src, src_ops


def device_scorer(dev):
    """the DeviceEditDistance of `dev`, made at the first call"""
    return DeviceEditDistance.of_device(dev)
