"""What the sentence metrics share on the Python side (ciderd.DeviceCiderD, bleu.DeviceBleu, rouge.DeviceRougeL,
editdist.DeviceEditDistance and the host scorers bleu.Bleu, rouge.RougeL, editdist.EditDistance): the two limits and the 0 rule
of csrc/ngram_wave.h, the flattening of reference sets into one padded upload, the prepared-reference record, the one front of
a scorer that lives on one device (DeviceSentenceScorer; RecordScorer for the three that read BLEU's records) and the one front
of a host scorer (HostSentenceScorer).  numpy only at import: torch is imported where a device is touched, so the numpy-only
use of `bleu`, `rouge`, `editdist` and `ciderd` keeps working.

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


def _host(x):
    return x.cpu() if hasattr(x, 'cpu') else x


def _entries(x, n, what):
    """x as a flat numpy array of n entries"""
    x = np.asarray(_host(x)).reshape(-1)
    if x.shape[0] != n:
        raise ValueError("%s has %d entries for %d sentences" % (what, x.shape[0], n))
    return x


def _id_array(x):
    x = np.asarray(_host(x), dtype=np.int64)
    if x.ndim != 2:
        raise ValueError("sentences are rows of a 2-D id array, got shape %s" % (x.shape,))
    return x


def id_rows(x, lens, what):
    """(N, L) ids [+ (N,) lengths] -> the N sentences as lists: lens=None the 0 rule (cut_after_zero), else exactly that long,
    clamped to [0, L]"""
    x = _id_array(x)
    N, L = x.shape
    if lens is None:
        return [cut_after_zero(x[i].tolist()) for i in range(N)]
    lens = _entries(lens, N, what)
    return [x[i].tolist()[:min(max(int(lens[i]), 0), L)] for i in range(N)]


def coco_pairs(gts, res):
    """coco's call -> [(hypothesis word list, list of reference word lists)]: gts = {image_id: [reference strings]}; res =
    {image_id: [one string]} or, as CiderD.compute_score takes it, [{'image_id': id, 'caption': [string]}].  Strings are split
    at whitespace."""
    if isinstance(res, dict):
        res = [{'image_id': k, 'caption': v} for k, v in res.items()]
    pairs = []
    for r in res:
        cap = r['caption']
        cap = cap[0] if isinstance(cap, (list, tuple)) else cap
        pairs.append((cap.split(), [s.split() for s in gts[r['image_id']]]))
    return pairs


class HostSentenceScorer:
    """Base of a metric's pure-Python host scorer.  A subclass states sentence_stats(hyp, refs), its STATS_COLUMNS, the shape of
    one sentence's score and, as _sentence_score, the score of one row of statistics."""
    STATS_COLUMNS = None
    SCORE_SHAPE = ()
    LENS_CHECKED_FIRST = False                 # which size error a call with BOTH a wrong hyp_set and a wrong hyp_lens raises

    def _score_lists(self, pairs):
        """pairs: iterable of (hypothesis token list, list of reference token lists) -> (stats (N, STATS_COLUMNS) int64, scores
        (N,) + SCORE_SHAPE float64)"""
        pairs = list(pairs)
        stats = np.zeros((len(pairs), self.STATS_COLUMNS), dtype=np.int64)
        scores = np.zeros((len(pairs),) + self.SCORE_SHAPE, dtype=np.float64)
        for i, (h, refs) in enumerate(pairs):
            if not len(refs):
                raise ValueError("hypothesis %d has no reference" % i)
            stats[i] = self.sentence_stats(h, refs)
            scores[i] = self._sentence_score(stats[i])
        return stats, scores

    def score_token_ids(self, hyps, hyp_set, ref_sets, hyp_lens=None):
        """`hyps` (N, L) ids, `hyp_set` (N,) index of each row's reference set, `ref_sets` = list of reference sets, each a
        list of id lists (as ciderd.ground_truth_lists returns them; cut after their first 0).  hyp_lens=None: a row is cut
        after its first 0 and the 0 stays (no 0: the whole row); else (N,) lengths, clamped to [0, L].
        Returns (stats int64 (N, STATS_COLUMNS), scores float64 (N,) + SCORE_SHAPE)."""
        hyps = _id_array(hyps)
        if not self.LENS_CHECKED_FIRST:
            hyp_set = _entries(hyp_set, len(hyps), "hyp_set")
        rows = id_rows(hyps, hyp_lens, "hyp_lens")
        hyp_set = _entries(hyp_set, len(rows), "hyp_set")
        refs = [[cut_after_zero(c) for c in rs] for rs in ref_sets]
        return self._score_lists((row, refs[int(s)]) for row, s in zip(rows, hyp_set))


def resolve_device(dev):
    """torch.device(dev), a bare "cuda" resolved to the current device's index (the key of the per-device scorer caches)"""
    import torch
    dev = torch.device(dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class DeviceSentenceScorer:
    """Base of a metric's scorer on one device: the device, id / index tensors in the form the native calls take, the front of
    a score call and pair_scores.  A subclass names its metric and the native entries it needs, and states _prepare (the
    records of rows on the device) and prepare_refs."""
    METRIC = None
    NATIVE = ()                                # the entries the library must export for this scorer
    _per_device = {}                           # (class, device) -> the scorer `of_device` made

    def __init__(self, dev):
        from . import _lib
        self.dev = resolve_device(dev)
        if self.dev.type != "cuda":
            raise _lib.SetError("the device %s scorer needs a GPU device, got %s" % (self.METRIC, self.dev))
        self._lib = _lib.load()
        for name in self.NATIVE:
            if name in _lib.MISSING:
                raise _lib.SetError("the native library does not export %s" % name)

    @classmethod
    def of_device(cls, dev):
        """the scorer of this class on `dev` (default construction), made at the first call: each module's device_scorer"""
        key = (cls, resolve_device(dev))
        if key not in DeviceSentenceScorer._per_device:
            DeviceSentenceScorer._per_device[key] = cls(key[1])
        return DeviceSentenceScorer._per_device[key]

    def _score_rows(self, entry, outputs, hyps, hyp_set, refs, hyp_lens, return_pairs, lead=(), extra=()):
        """The front of a score call: refs prepared here unless they are PreparedRefs, rows, set indices and lengths as device
        tensors, the optional (N, max set size) pair scores (columns beyond a smaller set stay 0), then
        entry(*lead, <rows, set indices, records, offsets and counts>, *extra, <outputs(N)>, pairs, pair_ld, stream).
        Returns the tensors of outputs(N) [+ pairs] as a tuple."""
        import torch
        from . import _lib
        if not isinstance(refs, PreparedRefs):
            refs = self.prepare_refs(refs)
        t = self._tokens(hyps)
        N, L = t.shape
        so = self._i32(hyp_set, N, "hyp_set")
        ln = self._i32(hyp_lens, N, "hyp_lens")
        out = outputs(N)
        pair_ld = max(1, refs.max_set)
        pairs = torch.zeros(N, pair_ld, dtype=torch.float64, device=self.dev) if return_pairs else None
        with torch.cuda.device(self.dev):
            rc = getattr(self._lib, entry)(
                *lead, t.data_ptr(), t.stride(0), None if ln is None else ln.data_ptr(), N, L, so.data_ptr(), refs.recs.data_ptr(),
                refs.L, refs.n_refs, refs.set_off.data_ptr(), refs.n_sets, refs.max_set, *extra, *(o.data_ptr() for o in out),
                None if pairs is None else pairs.data_ptr(), pair_ld, _lib.stream_of(self.dev))
        _lib.check(rc, entry)
        return out + (pairs,) if return_pairs else out

    def pair_scores(self, candidates, n_per_image):
        """(NI * n, L) candidates, n per image -> (NI * n, n): the metric's sentence score (BLEU: BLEU-4) of row i against
        candidate r of its own image as the only reference (what evaluate.consensus_rerank reads).  Rows are cut after their
        first 0; the candidates are prepared once on the device and serve as references."""
        t = self._tokens(candidates)
        refs, owner = self._self_refs(t, n_per_image)
        refs.recs = self._prepare(t, None)
        return self.score_token_ids(t, owner, refs, return_pairs=True)[-1]

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


class RecordScorer(DeviceSentenceScorer):
    """Base of the three scorers that read BLEU's prepared records (csrc/ngram_wave.h ref_rec_words, written by
    set_bleu_device_prepare, walked by RefWalk): bleu.DeviceBleu, rouge.DeviceRougeL, editdist.DeviceEditDistance.  One
    preparation serves all three, and either scorer's PreparedRefs serves the others.  A subclass declares METRIC, NATIVE,
    SCORE_ENTRY (its native score entry), STATS_COLUMNS, SCORE_SHAPE (of one row's scores) and, where the entry takes more
    than the shared arguments, _extra()."""
    SCORE_ENTRY = None
    STATS_COLUMNS = None
    SCORE_SHAPE = ()

    def _extra(self):
        """what the native score entry takes between max_set and stats"""
        return ()

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
        """Reference sets as ciderd.ground_truth_lists returns them (per image a list of id lists) -> PreparedRefs: one
        upload and one launch, independent of the rollout (issue it first and it runs underneath).  References are cut after
        their first 0 (count_end=False: before it, the validation convention).  An empty set or a reference longer than 64
        ids is refused.  The upload (tokens, lens, host lens) stays with the records, R * L * 8 bytes held as long as they
        are: the corpus CIDEr of the same sets is built from it (ciderd.DeviceCiderD.from_refs), whichever scorer prepared."""
        import torch
        sets = strip_end(ref_sets) if not count_end else [[cut_after_zero(c) for c in refs] for refs in ref_sets]
        tok, ln, off, R, L, max_set = pack_ref_sets(sets, self.METRIC, False)
        t, l = torch.from_numpy(tok[:R]).to(self.dev), torch.from_numpy(ln[:R]).to(self.dev)
        return PreparedRefs(self._prepare(t, l), L, R, torch.from_numpy(off).to(self.dev), len(sets), max_set, t, l, ln[:R])

    def score_token_ids(self, hyps, hyp_set, refs, hyp_lens=None, return_pairs=False):
        """Device twin of the host scorer's score_token_ids: `hyps` (N, L) ids, `hyp_set` (N,) index of each row's reference
        set, `refs` a PreparedRefs (or reference sets, prepared here), hyp_lens as on the host.  Returns device tensors (stats
        int32 (N, STATS_COLUMNS), scores float64 (N,) + SCORE_SHAPE); return_pairs=True: also (N, max set size) float64 with
        the sentence score (BLEU: BLEU-4) against every single reference of the set (columns beyond a smaller set stay 0)."""
        import torch
        outputs = lambda N: (torch.empty(N, self.STATS_COLUMNS, dtype=torch.int32, device=self.dev),
                             torch.empty((N,) + self.SCORE_SHAPE, dtype=torch.float64, device=self.dev))
        return self._score_rows(self.SCORE_ENTRY, outputs, hyps, hyp_set, refs, hyp_lens, return_pairs, extra=self._extra())
