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

from .device_metric import DeviceSentenceScorer, PreparedRefs, cut_after_zero, pack_ref_sets, resolve_device, strip_end

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


class RougeL:
    """The host scorer.  Pure Python: validation runs it once per epoch, and it is the readable statement that the device
    route is tested against."""

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

    def _score_lists(self, pairs):
        """pairs: iterable of (hypothesis token list, list of reference token lists) -> (stats (N, 4) int64, scores (N,))"""
        pairs = list(pairs)
        stats = np.zeros((len(pairs), STATS_COLUMNS), dtype=np.int64)
        scores = np.zeros(len(pairs), dtype=np.float64)
        for i, (h, refs) in enumerate(pairs):
            if not len(refs):
                raise ValueError("hypothesis %d has no reference" % i)
            stats[i] = self.sentence_stats(h, refs)
            scores[i] = self.score_from_stats(stats[i])
        return stats, scores

    def compute_score(self, gts, res):
        """coco's call: gts = {image_id: [reference strings]}; res = {image_id: [one string]} or, as CiderD.compute_score takes
        it, [{'image_id': id, 'caption': [string]}].  Strings are split at whitespace.  Returns (the mean of the sentence
        scores, [per-sentence score])."""
        if isinstance(res, dict):
            res = [{'image_id': k, 'caption': v} for k, v in res.items()]
        pairs = []
        for r in res:
            cap = r['caption']
            cap = cap[0] if isinstance(cap, (list, tuple)) else cap
            pairs.append((cap.split(), [s.split() for s in gts[r['image_id']]]))
        _, scores = self._score_lists(pairs)
        return (float(np.mean(scores)) if len(scores) else 0.0), scores.tolist()

    def score_token_ids(self, hyps, hyp_set, ref_sets, hyp_lens=None):
        """`hyps` (N, L) ids, `hyp_set` (N,) index of each row's reference set, `ref_sets` = list of reference sets, each a
        list of id lists (as ciderd.ground_truth_lists returns them; cut after their first 0).  hyp_lens=None: a row is cut
        after its first 0 and the 0 stays (no 0: the whole row); else (N,) lengths, clamped to [0, L].
        Returns (stats int64 (N, 4), scores float64 (N,))."""
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


# ---- the device route (csrc/rouge_device.hip, include/set_hip.h set_rouge_device_score) --------------------------------------
class DeviceRougeL(DeviceSentenceScorer):
    """ROUGE-L on one device: every call is enqueued on the current stream of that device and reads nothing back.  Stateless
    on the native side: an instance remembers its device and beta.  Its prepared references are bleu.DeviceBleu's (the same
    native call, the same records): either scorer's PreparedRefs serves the other."""
    METRIC = "ROUGE-L"

    def __init__(self, dev, beta=BETA):
        from . import _lib
        super().__init__(dev)
        for name in ("set_bleu_device_prepare", "set_rouge_device_score"):
            if name in _lib.MISSING:
                raise _lib.SetError("the native library does not export %s" % name)
        self.beta = RougeL(beta).beta

    def _prepare(self, t, ln):
        """(R, L) device ids [+ (R,) device int32 lengths] -> the record buffer (BLEU's layout)"""
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
        """Reference sets as ciderd.ground_truth_lists returns them (per image a list of id lists) -> PreparedRefs, under the
        rules of bleu.DeviceBleu.prepare_refs: cut after their first 0 (count_end=False: before it, the validation
        convention); an empty set or a reference longer than 64 ids is refused."""
        import torch
        sets = strip_end(ref_sets) if not count_end else [[cut_after_zero(c) for c in refs] for refs in ref_sets]
        tok, ln, off, R, L, max_set = pack_ref_sets(sets, self.METRIC, False)
        recs = self._prepare(torch.from_numpy(tok[:R]).to(self.dev), torch.from_numpy(ln[:R]).to(self.dev))
        return PreparedRefs(recs, L, R, torch.from_numpy(off).to(self.dev), len(sets), max_set)

    def score_token_ids(self, hyps, hyp_set, refs, hyp_lens=None, return_pairs=False):
        """Device twin of RougeL.score_token_ids: `hyps` (N, L) ids, `hyp_set` (N,) index of each row's reference set, `refs` a
        PreparedRefs (or reference sets, prepared here), hyp_lens as on the host.  Returns device tensors (stats int32 (N, 4),
        scores float64 (N,)); return_pairs=True: also (N, max set size) float64 with the score against every single reference
        of the set (columns beyond a smaller set stay 0)."""
        import torch
        from . import _lib
        if not isinstance(refs, PreparedRefs):
            refs = self.prepare_refs(refs)
        t = self._tokens(hyps)
        N, L = t.shape
        so = self._i32(hyp_set, N, "hyp_set")
        ln = self._i32(hyp_lens, N, "hyp_lens")
        stats = torch.empty(N, STATS_COLUMNS, dtype=torch.int32, device=self.dev)
        scores = torch.empty(N, dtype=torch.float64, device=self.dev)
        pair_ld = max(1, refs.max_set)
        pairs = torch.zeros(N, pair_ld, dtype=torch.float64, device=self.dev) if return_pairs else None
        with torch.cuda.device(self.dev):
            rc = self._lib.set_rouge_device_score(
                t.data_ptr(), t.stride(0), None if ln is None else ln.data_ptr(), N, L, so.data_ptr(), refs.recs.data_ptr(),
                refs.L, refs.n_refs, refs.set_off.data_ptr(), refs.n_sets, refs.max_set, self.beta, stats.data_ptr(),
                scores.data_ptr(), None if pairs is None else pairs.data_ptr(), pair_ld, _lib.stream_of(self.dev))
        _lib.check(rc, "set_rouge_device_score")
        return (stats, scores, pairs) if return_pairs else (stats, scores)

    def corpus_score(self, hyps, hyp_set, refs, hyp_lens=None):
        """ROUGE_L of the corpus: the mean of the rows' scores, taken on the device (no row: 0).  Returns a 0-d float64 device
        tensor; nothing is read back."""
        scores = self.score_token_ids(hyps, hyp_set, refs, hyp_lens)[1]
        return scores.mean() if scores.numel() else scores.new_zeros(())

    def pair_scores(self, candidates, n_per_image):
        """(NI * n, L) candidates, n per image -> (NI * n, n): the ROUGE-L of row i against candidate r of its own image as the
        only reference (what evaluate.consensus_rerank reads).  Rows are cut after their first 0; the candidates are prepared
        once on the device and serve as references."""
        t = self._tokens(candidates)
        refs, owner = self._self_refs(t, n_per_image)
        refs.recs = self._prepare(t, None)
        return self.score_token_ids(t, owner, refs, return_pairs=True)[2]


_device_scorers = {}


def device_scorer(dev):
    """the DeviceRougeL (beta = 1.2) of `dev`, made at the first call"""
    dev = resolve_device(dev)
    if dev not in _device_scorers:
        _device_scorers[dev] = DeviceRougeL(dev)
    return _device_scorers[dev]
