"""Build-owned CIDEr-D scorer for the SCST reward.

The reference does not contain its scorer: `editnet_rl.py:576-578` imports `CiderD` from the un-vendored
`ruotianluo/cider` checkout (version unpinned), so reward VALUES are "parity unpinned" (SURVEY.md §8c.3).
This module restates the published CIDEr-D metric (Vedantam et al., CVPR 2015, §"CIDEr-D"; the variant
with a precomputed document-frequency table that self-critical training uses):

    g_n(s)      tf-idf vector over the n-grams of s, n = 1..4:  tf(ngram) * (log N_docs - log max(1, df(ngram)))
    sim_n(c, r) = sum_ngram min(g(c), g(r)) * g(r) / (|g(c)| |g(r)|) * exp(-(l_c - l_r)^2 / (2 sigma^2)),  sigma = 6
    CIDEr-D(c)  = 10 / (4 |refs|) * sum_n sum_r sim_n(c, r)

with l = number of bigrams of the sentence (the length the public implementations use).  The document
frequency table has the format `preprocess_rl.py:7-55` writes: {n-gram tuple of token strings: number of
images whose reference set contains it} plus `ref_len` = number of images.

Two conventions share this formula and differ in the table alone.  The SCST REWARD scores against a table pickled beforehand
from the training set (`CiderD(df, ref_len)`).  The CORPUS score that validation reports — cocoEval's `CIDEr`, the first value
of the reference's `evaluate()` — takes df and N from the reference sets of the corpus being scored (`CiderD.from_corpus`,
`corpus_cider`; on the device `DeviceCiderD.from_refs`, `evaluate.validation_cider`).

Host-side, per-sample work (strings and dictionaries): it shards with the batch and never touches the GPU.
`compute_score` runs on the native implementation in csrc/ciderd_host.hip (`set_ciderd_*`, host pointers): in Python
the scorer was half of the SCST step's wall time at 5 samples per image.  The pure-Python `score` below is the
readable statement of the metric and the cross-check of the native one (tests/test_ciderd.py); identical
(reference set, caption) pairs of a batch — e.g. the greedy baseline repeated for every sample — are scored once.
"""
from __future__ import annotations

import math
from collections import Counter

import numpy as np

from .device_metric import (DEVICE_MAX_LEN, DEVICE_PACK_LIMIT, DeviceSentenceScorer, PreparedRefs, cut_after_zero, pack_ref_sets,
                            resolve_device, strip_end)


def ngram_counts(sentence, n=4):
    """Counter of all 1..n-grams (tuples of token strings) of a whitespace-tokenised sentence."""
    words = sentence.split()
    c = Counter()
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            c[tuple(words[i:i + k])] += 1
    return c


def document_frequency(reference_sets, n=4):
    """df table over a corpus: reference_sets = iterable of lists of reference sentences (one list per
    image).  Returns (df dict, number of images) -- the two fields `preprocess_rl.py` pickles."""
    df, docs = Counter(), 0
    for refs in reference_sets:
        seen = set()
        for r in refs:
            seen.update(ngram_counts(r, n).keys())
        for g in seen:
            df[g] += 1
        docs += 1
    return dict(df), docs


class CiderD:
    def __init__(self, df, ref_len, n=4, sigma=6.0):
        """df: n-gram -> document count; ref_len: number of documents the table was built from"""
        self.df = df
        self.ref_len = float(ref_len)
        self.log_ref_len = math.log(float(ref_len))
        self.n = n
        self.sigma = sigma
        self._tok = {}           # token string -> int id (interned for the native scorer)
        self._native = None

    @classmethod
    def from_corpus(cls, reference_sets, n=4, sigma=6.0):
        """The scorer of cocoEval's `CIDEr`: the same formula with the df table and the number of documents taken from the
        reference sets of the corpus that is scored (one list of reference sentences per image)."""
        return cls(*document_frequency(reference_sets, n), n, sigma)

    # ---- native scorer (csrc/ciderd_host.hip) -------------------------------------------------------------
    def _ids(self, sentence):
        tok = self._tok
        return [tok.setdefault(w, len(tok)) for w in sentence.split()]

    def _handle(self):
        """Build the native df table once (None if the library is unavailable: pure-Python scoring then)."""
        if self._native is None:
            try:
                from . import _lib
                lib = _lib.load()
                if "set_ciderd_create" in _lib.MISSING:
                    raise _lib.SetError("library without CIDEr-D")
            except Exception:
                self._native = False
                return None
            grams = [g for g in self.df if 1 <= len(g) <= 4]
            toks = np.zeros((max(1, len(grams)), 4), dtype=np.int64)
            lens = np.zeros(max(1, len(grams)), dtype=np.int32)
            cnt = np.zeros(max(1, len(grams)), dtype=np.float64)
            tok = self._tok
            for i, g in enumerate(grams):
                lens[i] = len(g)
                cnt[i] = self.df[g]
                for j, w in enumerate(g):
                    toks[i, j] = tok.setdefault(w, len(tok))
            h = lib.set_ciderd_create(toks.ctypes.data, lens.ctypes.data, cnt.ctypes.data, len(grams), self.ref_len,
                                      self.n, self.sigma)
            if not h:
                self._native = False
                return None
            self._native = (lib, h)
        return self._native or None

    def __del__(self):
        if isinstance(getattr(self, "_native", None), tuple):
            lib, h = self._native
            try:
                lib.set_ciderd_destroy(h)
            except Exception:
                pass

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_native"] = None
        return st

    def _vector(self, counts):
        vec = [dict() for _ in range(self.n)]
        norm = [0.0] * self.n
        length = 0
        for g, tf in counts.items():
            k = len(g) - 1
            w = float(tf) * (self.log_ref_len - math.log(max(1.0, self.df.get(g, 0.0))))
            vec[k][g] = w
            norm[k] += w * w
            if k == 1:
                length += tf
        return vec, [math.sqrt(x) for x in norm], length

    def _similarity(self, hyp, ref):
        (vh, nh, lh), (vr, nr, lr) = hyp, ref
        delta = float(lh - lr)
        penalty = math.exp(-(delta * delta) / (2.0 * self.sigma * self.sigma))
        out = np.zeros(self.n)
        for k in range(self.n):
            s = 0.0
            for g, w in vh[k].items():
                wr = vr[k].get(g)
                if wr is not None:
                    s += min(w, wr) * wr
            if nh[k] != 0.0 and nr[k] != 0.0:
                s /= nh[k] * nr[k]
            out[k] = s * penalty
        return out

    def score(self, hypothesis, references):
        """CIDEr-D of one sentence against its reference sentences."""
        hyp = self._vector(ngram_counts(hypothesis, self.n))
        tot = np.zeros(self.n)
        for r in references:
            tot += self._similarity(hyp, self._vector(ngram_counts(r, self.n)))
        return float(tot.mean() / max(1, len(references)) * 10.0)

    def compute_score(self, gts, res):
        """Same call shape as the external scorer at editnet_rl.py:636: gts = {image_id: [ref strings]},
        res = [{'image_id': id, 'caption': [string]}].  Returns (mean score, per-entry scores)."""
        nat = self._handle()
        if nat is None:
            return self._compute_score_py(gts, res)
        lib, h = nat
        # reference sets and (set, caption) pairs are de-duplicated by content
        set_index, sets = {}, []
        pair_index, pairs = {}, []
        which = np.zeros(len(res), dtype=np.int64)
        for i, r in enumerate(res):
            refs = gts[r['image_id']]
            key = tuple(refs)
            si = set_index.get(key)
            if si is None:
                si = set_index[key] = len(sets)
                sets.append(refs)
            pk = (si, r['caption'][0])
            pi = pair_index.get(pk)
            if pi is None:
                pi = pair_index[pk] = len(pairs)
                pairs.append(pk)
            which[i] = pi
        ref_tok, ref_off, set_off = [], [0], [0]
        for refs in sets:
            for sref in refs:
                ref_tok += self._ids(sref)
                ref_off.append(len(ref_tok))
            set_off.append(len(ref_off) - 1)
        hyp_tok, hyp_off, set_of = [], [0], []
        for si, cap in pairs:
            hyp_tok += self._ids(cap)
            hyp_off.append(len(hyp_tok))
            set_of.append(si)
        a = lambda x, dt: np.ascontiguousarray(np.asarray(x if len(x) else [0], dtype=dt))
        ht, ho, so = a(hyp_tok, np.int64), a(hyp_off, np.int64), a(set_of, np.int32)
        rt, ro, rs = a(ref_tok, np.int64), a(ref_off, np.int64), a(set_off, np.int64)
        out = np.zeros(max(1, len(pairs)), dtype=np.float64)
        rc = lib.set_ciderd_score(h, ht.ctypes.data, ho.ctypes.data, len(pairs), so.ctypes.data, rt.ctypes.data,
                                  ro.ctypes.data, rs.ctypes.data, len(sets), out.ctypes.data)
        if rc != 0:
            raise RuntimeError("set_ciderd_score failed with code %d" % rc)
        scores = out[which] if len(res) else np.zeros(0)
        return float(scores.mean()) if len(res) else 0.0, scores

    def _lut_for(self, max_id):
        """vocabulary id -> interned index of the word str(id) (the reward plumbing stringifies token ids,
        editnet_rl.py:601-609), as a numpy lookup table grown on demand"""
        lut = getattr(self, "_lut", None)
        if lut is None or lut.shape[0] <= max_id:
            n0 = 0 if lut is None else lut.shape[0]
            n1 = max(max_id + 1, 2 * n0, 1024)
            new = np.empty(n1, dtype=np.int64)
            if n0:
                new[:n0] = lut
            tok = self._tok
            for i in range(n0, n1):
                new[i] = tok.setdefault(str(i), len(tok))
            self._lut = lut = new
        return lut

    def score_token_ids(self, hyps, hyp_set, ref_sets):
        """Integer fast path of compute_score for the self-critical reward: `hyps` (N, L) int array of decoded captions
        (0 = <end>, everything after the first 0 is ignored, the 0 itself is a word), `hyp_set` (N,) index of each
        caption's reference set, `ref_sets` = list of reference sets, each a list of id lists (as ground_truth_lists
        returns them).  Same scores as compute_score on the stringified ids; needs the native scorer."""
        nat = self._handle()
        if nat is None:
            raise RuntimeError("score_token_ids needs the native CIDEr-D scorer")
        lib, h = nat
        hyps = np.ascontiguousarray(hyps, dtype=np.int64)
        N, L = hyps.shape
        is0 = hyps == 0
        first0 = np.where(is0.any(1), is0.argmax(1), L - 1)          # keep the first 0; no 0 -> the whole row
        lens = first0 + 1
        keep = np.arange(L)[None, :] < lens[:, None]
        # references are cut after their first 0 as well (tokens_to_str / array_to_str do the same on the string path;
        # lists from ground_truth_lists carry no interior 0)
        flat_refs = [cut_after_zero(c) for refs in ref_sets for c in refs]
        ref_len = np.fromiter((len(c) for c in flat_refs), dtype=np.int64, count=len(flat_refs))
        ref_flat = np.fromiter((w for c in flat_refs for w in c), dtype=np.int64, count=int(ref_len.sum()))
        max_id = int(max(hyps.max(initial=0), ref_flat.max(initial=0)))
        lut = self._lut_for(max_id)
        ht = np.ascontiguousarray(lut[hyps[keep]])
        ho = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(lens, out=ho[1:])
        so = np.ascontiguousarray(hyp_set, dtype=np.int32)
        rt = np.ascontiguousarray(lut[ref_flat]) if ref_flat.size else np.zeros(1, dtype=np.int64)
        ro = np.zeros(len(flat_refs) + 1, dtype=np.int64)
        np.cumsum(ref_len, out=ro[1:])
        rs = np.zeros(len(ref_sets) + 1, dtype=np.int64)
        np.cumsum(np.fromiter((len(r) for r in ref_sets), dtype=np.int64, count=len(ref_sets)), out=rs[1:])
        out = np.zeros(max(1, N), dtype=np.float64)
        rc = lib.set_ciderd_score(h, ht.ctypes.data, ho.ctypes.data, N, so.ctypes.data, rt.ctypes.data, ro.ctypes.data,
                                  rs.ctypes.data, len(ref_sets), out.ctypes.data)
        if rc != 0:
            raise RuntimeError("set_ciderd_score failed with code %d" % rc)
        return out[:N]

    def _compute_score_py(self, gts, res):
        """pure-Python twin of compute_score (cross-check; also the fallback when the library is not built)"""
        cache = {}
        scores = np.zeros(len(res))
        for i, r in enumerate(res):
            key = r['image_id']
            refs = gts[key]
            rk = tuple(refs)
            if rk not in cache:
                cache[rk] = [self._vector(ngram_counts(s, self.n)) for s in refs]
            hyp = self._vector(ngram_counts(r['caption'][0], self.n))
            tot = np.zeros(self.n)
            for rv in cache[rk]:
                tot += self._similarity(hyp, rv)
            scores[i] = tot.mean() / max(1, len(refs)) * 10.0
        return float(scores.mean()) if len(res) else 0.0, scores


def corpus_cider(gts, res, n=4, sigma=6.0):
    """cocoEval's `CIDEr` of a corpus (the first value of the reference's evaluate(), `eval/eval rl/eval_full.py:235`), in the
    call shape of CiderD.compute_score: gts = {image_id: [reference strings]}, res = [{'image_id': id, 'caption': [string]}] (or
    coco's {image_id: [string]}).  The sentence formula is the one above; what differs from the SCST reward is the table: df
    and the number of documents N come from ALL reference sets of `gts`, the corpus that is scored — an n-gram counts once per
    image however often it occurs in that image's references, and log N is the idf's ceiling.  A corpus of one image scores
    0.0 (log 1 = 0: every weight vanishes), as in coco-caption.  Pure Python: the readable statement that
    DeviceCiderD.from_refs and evaluate.validation_cider are tested against.  Returns (mean score, per-entry scores)."""
    if isinstance(res, dict):
        res = [{'image_id': k, 'caption': v} for k, v in res.items()]
    return CiderD.from_corpus(gts.values(), n, sigma)._compute_score_py(gts, res)


# ---- the reward plumbing of editnet_rl.py:584-646 ------------------------------------------------------
def tokens_to_str(ids):
    """ids of one caption -> space-joined string, cut after the first 0 (the decoder writes 0 for <end>
    and everything after it; the 0 itself is kept as the end-of-sentence token, editnet_rl.py:601-609)."""
    out = []
    for w in ids:
        out.append(str(int(w)))
        if int(w) == 0:
            break
    return ' '.join(out)


def ground_truth_lists(allcaps, word_map):
    """(B, n_refs, L) ids -> per image list of id lists without <start>/<pad>, <end> rewritten to 0
    (editnet_rl.py:584-599)."""
    drop = {int(word_map['<start>']), int(word_map['<pad>'])}
    end = int(word_map['<end>'])
    out = []
    for caps in np.asarray(allcaps.cpu() if hasattr(allcaps, 'cpu') else allcaps).tolist():
        out.append([[0 if w == end else w for w in c if w not in drop] for c in caps])
    return out


def _reward_sets(ground_truth, B):
    """the reference sets of the distinct images (by identity of their list) and, for the B sampled and then the B greedy
    captions, the index of each one's set"""
    sets, index = [], {}
    hyp_set = np.empty(2 * B, dtype=np.int32)
    for i in range(B):
        caps = ground_truth[i]
        k = id(caps)
        if k not in index:
            index[k] = len(sets)
            sets.append(caps)
        hyp_set[i] = hyp_set[B + i] = index[k]
    return sets, hyp_set


def _mix_term(scorer, weight, sampled, greedy, ground_truth, column=None):
    """weight * (score(sampled_b) - score(greedy_b)) in double: the sentence scores of a host scorer's score_token_ids (bleu.Bleu
    with column 3, its BLEU-4; rouge.RougeL with column None), rows cut after their first 0, the 0 a token — the convention of
    the CIDEr-D term"""
    B = sampled.shape[0]
    sets, hyp_set = _reward_sets(ground_truth, B)
    x = np.asarray(scorer.score_token_ids(np.concatenate([sampled, greedy], 0), hyp_set, sets)[1], dtype=np.float64)
    x = x if column is None else x[:, column]
    return weight * (x[:B] - x[B:])


def self_critical_reward(scorer, sampled, greedy, ground_truth, cider_weight=1.0, bleu_scorer=None, bleu_weight=0.0,
                         rouge_scorer=None, rouge_weight=0.0):
    """reward[b, :] = CIDEr-D(sampled_b) - CIDEr-D(greedy_b), repeated over the max_len columns
    (editnet_rl.py:611-646).  sampled/greedy: (B, max_len) integer arrays/tensors; returns float32 numpy.
    With a `bleu_scorer` (bleu.Bleu) and bleu_weight != 0 the reward of the self-critical code base:
    cider_weight * dCIDEr-D + bleu_weight * dBLEU-4, mixed in double and then cast; with a `rouge_scorer` (rouge.RougeL) and
    rouge_weight != 0: + rouge_weight * dROUGE-L, in the same sum; otherwise the scorers see the calls they saw before the
    arguments existed."""
    sampled = np.asarray(sampled.cpu() if hasattr(sampled, 'cpu') else sampled)
    greedy = np.asarray(greedy.cpu() if hasattr(greedy, 'cpu') else greedy)
    B = sampled.shape[0]
    if getattr(scorer, "_handle", None) is not None and scorer._handle() is not None:
        # integer fast path (no strings): the reference sets of the distinct images once, all 2B captions in one call
        sets, hyp_set = _reward_sets(ground_truth, B)
        s = scorer.score_token_ids(np.concatenate([sampled, greedy], 0), hyp_set, sets)
    else:
        memo = {}                # the same image's reference lists are repeated once per sample: stringify them once

        def ref_strings(caps):
            k = id(caps)
            if k not in memo:
                memo[k] = [tokens_to_str(c) for c in caps]
            return memo[k]

        refs = [ref_strings(caps) for caps in ground_truth]
        gts = {i: refs[i % B] for i in range(2 * B)}
        res = [{'image_id': i, 'caption': [tokens_to_str(sampled[i])]} for i in range(B)]
        res += [{'image_id': B + i, 'caption': [tokens_to_str(greedy[i])]} for i in range(B)]
        _, s = scorer.compute_score(gts, res)
    diff = cider_weight * (s[:B] - s[B:])
    for term, weight, column in ((bleu_scorer, bleu_weight, 3), (rouge_scorer, rouge_weight, None)):      # in this order
        if term is not None and weight != 0.0:
            diff = diff + _mix_term(term, weight, sampled, greedy, ground_truth, column)
    return np.repeat(diff[:, None], sampled.shape[1], 1).astype(np.float32)


# ---- the device route (csrc/ciderd_device.hip, include/set_hip.h set_ciderd_device_*) ---------------------------------
# The integer reward path above without the host trip: sentences, reference vectors and scores stay in device memory.
# Limits: the id and length limits of device_metric.py (shared with bleu.DeviceBleu), and only the df grams whose tokens are
# all decimal strings (the reward plumbing stringifies ids: any other gram can never match an id sequence).  Opt-in: nothing
# above calls it.


def pack_key(ids):
    """packed 64-bit key of an n-gram of 1..4 vocabulary ids: id + 1 in 16-bit fields (make_key, csrc/ngram_wave.h)"""
    ids = [int(w) for w in ids]
    if not 1 <= len(ids) <= 4:
        raise ValueError("an n-gram has 1..4 ids, got %d" % len(ids))
    key = 0
    for j, w in enumerate(ids):
        if not 0 <= w < DEVICE_PACK_LIMIT:
            raise ValueError("id %d outside [0, %d)" % (w, DEVICE_PACK_LIMIT))
        key |= (w + 1) << (16 * j)
    return key


def _gram_ids(g):
    """the ids of a df gram whose tokens are all decimal strings (or integers), else None"""
    out = []
    for w in g:
        if isinstance(w, (int, np.integer)):
            out.append(int(w))
        elif isinstance(w, str) and w.isascii() and w.isdigit():
            out.append(int(w))
        else:
            return None
    return out


def device_table_input(df):
    """The table input of set_ciderd_device_create from a df dict: (tokens (E, 4) int64 vocabulary ids, lens (E,) int32,
    counts (E,) float64, E).  Grams of other lengths than 1..4 and grams with a non-numeric token are dropped (they can
    never match a sequence of ids); arrays have at least one row so that their pointers are valid."""
    rows = []
    for g, c in df.items():
        if not 1 <= len(g) <= 4:
            continue
        ids = _gram_ids(g)
        if ids is not None:
            rows.append((ids, float(c)))
    E = len(rows)
    toks = np.zeros((max(1, E), 4), dtype=np.int64)
    lens = np.zeros(max(1, E), dtype=np.int32)
    cnt = np.zeros(max(1, E), dtype=np.float64)
    for i, (ids, c) in enumerate(rows):
        lens[i] = len(ids)
        cnt[i] = c
        toks[i, :len(ids)] = ids
    return toks, lens, cnt, E


class DeviceCiderD(DeviceSentenceScorer):
    """Owner of the device df table of one CiderD on one device (CiderD.device(dev)); every call is enqueued on the
    current stream of that device and reads nothing back."""
    METRIC = "CIDEr-D"

    def __init__(self, scorer, dev):
        import ctypes as C
        import torch
        from . import _lib
        super().__init__(dev)
        toks, lens, cnt, E = device_table_input(scorer.df)
        h = C.c_void_p()
        with torch.cuda.device(self.dev):
            rc = self._lib.set_ciderd_device_create(toks.ctypes.data, lens.ctypes.data, cnt.ctypes.data, E, float(scorer.ref_len),
                                                    int(scorer.n), float(scorer.sigma), _lib.stream_of(self.dev), C.byref(h))
        _lib.check(rc, "set_ciderd_device_create")
        self._h, self.n, self.n_entries = h, int(scorer.n), E

    @classmethod
    def from_refs(cls, dev, ref_sets, count_end=True, n=4, sigma=6.0, tokens=None, lens=None, set_off=None):
        """The scorer of cocoEval's `CIDEr` (corpus_cider) for one corpus, built on the device: (scorer, PreparedRefs).
        ref_sets: the corpus's reference sets as ground_truth_lists returns them (per image a list of id lists); df and N come
        from ALL of them (csrc/ciderd_device.hip cd_build_k: one wave per set enters its grams into the open-addressing table,
        once per set).  count_end=True cuts a reference after its first 0 (the 0 is a token), False before it
        (device_metric.strip_end, the validation convention).  One upload, one build launch and one vectorise launch on the
        current stream; nothing is read back.  Empty sets are allowed (a caption of such a set scores 0).
        The upload another metric already made of these very sets serves as well: pass tokens=, lens=, set_off= ((R, L) int64
        ids, (R,) int32 lengths, (n_sets + 1,) int64 offsets on the device; ref_sets is then only counted on the host), or pass
        as ref_sets the PreparedBleuRefs of bleu.DeviceBleu.prepare_refs, which keeps its upload and the host-side lengths
        (.tokens, .lens, .set_off, .host_lens; its count_end stands, nothing is packed again).
        The table's capacity is the power of two >= max(2, 2 * gram_bound), gram_bound = sum_r sum_{k < n} max(0, len_r - k)
        from the lengths held here: no gram can be dropped (dropped() == 0)."""
        import ctypes as C
        import torch
        from . import _lib
        self = cls.__new__(cls)
        DeviceSentenceScorer.__init__(self, dev)
        if "set_ciderd_device_create_corpus" in _lib.MISSING:
            raise _lib.SetError("the native library does not export set_ciderd_device_create_corpus")
        if isinstance(ref_sets, PreparedRefs):
            p = ref_sets
            if getattr(p, "tokens", None) is None or getattr(p, "host_lens", None) is None:
                raise ValueError("these PreparedRefs do not carry their upload (bleu.DeviceBleu.prepare_refs keeps it)")
            tokens, lens, set_off, ln, R, L, n_sets, max_set = p.tokens, p.lens, p.set_off, p.host_lens, p.n_refs, p.L, p.n_sets, p.max_set
        else:
            sets = [[cut_after_zero(c) for c in refs] for refs in ref_sets] if count_end else strip_end(ref_sets)
            tok, ln, off, R, L, max_set = pack_ref_sets(sets, self.METRIC, True)
            n_sets = len(sets)
            if tokens is None:
                tokens, lens, set_off = (torch.from_numpy(x).to(self.dev) for x in (tok, ln, off))
            elif lens is None or set_off is None:
                raise ValueError("tokens= comes with lens= and set_off= (the three device tensors of one upload)")
        if (tokens.dim() != 2 or tokens.shape[0] < R or tokens.shape[1] != L or tokens.stride(1) != 1 or lens.numel() < R
                or set_off.numel() != n_sets + 1 or tokens.dtype != torch.int64 or lens.dtype != torch.int32
                or set_off.dtype != torch.int64 or any(resolve_device(x.device) != self.dev for x in (tokens, lens, set_off))):
            raise ValueError("tokens=, lens=, set_off= are not the device upload of these reference sets")
        k = np.arange(int(n))[None, :]
        self.gram_bound = int(np.maximum(np.asarray(ln[:R], dtype=np.int64)[:, None] - k, 0).sum())
        self.capacity = 2
        while self.capacity < 2 * self.gram_bound:
            self.capacity *= 2
        h = C.c_void_p()
        with torch.cuda.device(self.dev):
            rc = self._lib.set_ciderd_device_create_corpus(tokens.data_ptr(), tokens.stride(0), lens.data_ptr(), R, L, set_off.data_ptr(),
                                                           n_sets, max_set, self.gram_bound, int(n), float(sigma),
                                                           _lib.stream_of(self.dev), C.byref(h))
        _lib.check(rc, "set_ciderd_device_create_corpus")
        self._h, self.n, self.n_entries = h, int(n), None
        recs, _ = self.vectorise(tokens[:R], lens[:R])
        return self, PreparedRefs(recs, L, R, set_off, n_sets, max_set)

    def dropped(self):
        """FOR TESTS (it waits for the stream and reads one number back): the grams the device build could not place because its
        bound was too small; 0 for a table that came from the host"""
        import ctypes as C
        import torch
        from . import _lib
        out = C.c_int64(-1)
        with torch.cuda.device(self.dev):
            rc = self._lib.set_ciderd_device_dropped(self._h, C.byref(out), _lib.stream_of(self.dev))
        _lib.check(rc, "set_ciderd_device_dropped")
        return int(out.value)

    def corpus_score(self, hyps, hyp_set, refs, hyp_lens=None):
        """The corpus value: the mean of the rows' scores, taken on the device (no row: 0; a NaN row makes it NaN).  Returns a
        0-d float64 device tensor; nothing is read back."""
        scores = self.score_token_ids(hyps, hyp_set, refs, hyp_lens=hyp_lens)
        return scores.mean() if scores.numel() else scores.new_zeros(())

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.set_ciderd_device_destroy(h)
            except Exception:
                pass

    def lookup(self, keys):
        """document count of packed keys (pack_key): a device int64 tensor holding the keys' bits, or a list of ints;
        returns a float64 device tensor, 0.0 for a key the table does not hold"""
        import torch
        from . import _lib
        if not torch.is_tensor(keys):
            keys = torch.from_numpy(np.asarray([int(k) for k in keys], dtype=np.uint64).view(np.int64))
        keys = keys.reshape(-1).to(self.dev, torch.int64).contiguous()
        out = torch.empty(keys.numel(), dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = self._lib.set_ciderd_device_lookup(self._h, keys.data_ptr(), keys.numel(), out.data_ptr(), _lib.stream_of(self.dev))
        _lib.check(rc, "set_ciderd_device_lookup")
        return out

    def vectorise(self, tokens, lens=None):
        """(S, L) ids [+ (S,) lengths; None: cut after the first 0] -> (record buffer, L): a caller-owned workspace"""
        import torch
        from . import _lib
        t = self._tokens(tokens)
        S, L = t.shape
        ln = self._i32(lens, S, "lens")
        recs = torch.empty(S * (8 + 8 * L), dtype=torch.int64, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = self._lib.set_ciderd_device_vectorise(self._h, t.data_ptr(), t.stride(0), None if ln is None else ln.data_ptr(),
                                                       S, L, recs.data_ptr(), _lib.stream_of(self.dev))
        _lib.check(rc, "set_ciderd_device_vectorise")
        return recs, L

    def prepare_refs(self, ref_sets):
        """Reference sets as ground_truth_lists returns them (per image a list of id lists) -> PreparedRefs: one upload and
        one vectorise launch, independent of the rollout (issue it first and it runs underneath).  References are cut after
        their first 0 as score_token_ids does; an empty set is allowed (it scores 0); a reference longer than 64 ids is refused."""
        import torch
        tok, ln, off, R, L, max_set = pack_ref_sets([[cut_after_zero(c) for c in refs] for refs in ref_sets], self.METRIC, True)
        recs, _ = self.vectorise(torch.from_numpy(tok[:R]), ln[:R])
        return PreparedRefs(recs, L, R, torch.from_numpy(off).to(self.dev), len(ref_sets), max_set)

    def score_token_ids(self, hyps, hyp_set, refs, return_pairs=False, hyp_lens=None):
        """Device twin of CiderD.score_token_ids: `hyps` (N, L) ids (0 = <end>, cut after the first 0; with hyp_lens the
        given lengths instead), `hyp_set` (N,) index of each caption's reference set, `refs` a PreparedRefs (or reference
        sets, prepared here).  Returns the (N,) float64 device tensor of scores; return_pairs=True: also (N, max set size)
        with the score against every single reference of the set (columns beyond a smaller set stay 0)."""
        import torch
        outputs = lambda N: (torch.empty(N, dtype=torch.float64, device=self.dev),)
        out = self._score_rows("set_ciderd_device_score", outputs, hyps, hyp_set, refs, hyp_lens, return_pairs, lead=(self._h,))
        return out if return_pairs else out[0]

    def _prepare(self, t, ln):
        """the records of these rows (pair_scores of the base: the candidates are vectorised once and serve as references)"""
        return self.vectorise(t, ln)[0]


import weakref as _weakref

_device_scorers = _weakref.WeakKeyDictionary()      # CiderD -> {device: DeviceCiderD}: not part of the scorer's pickled state


def _ciderd_device(self, dev):
    """The DeviceCiderD of this scorer on `dev`: built at the first call (table upload), cached per device."""
    dev = resolve_device(dev)
    per = _device_scorers.setdefault(self, {})
    if dev not in per:
        per[dev] = DeviceCiderD(self, dev)
    return per[dev]


CiderD.device = _ciderd_device


def self_critical_reward_device(dscorer, sampled, greedy, refs, image_of=None, cider_weight=1.0, bleu_scorer=None, bleu_refs=None,
                                bleu_weight=0.0, rouge_scorer=None, rouge_refs=None, rouge_weight=0.0):
    """Device twin of self_critical_reward: reward[b, :] = cider_weight * (CIDEr-D(sampled_b) - CIDEr-D(greedy of its image)).
    With a `bleu_scorer` (bleu.DeviceBleu), `bleu_refs` (its PreparedBleuRefs of the NI images, or their reference sets) and
    bleu_weight != 0: + bleu_weight * (BLEU-4(sampled_b) - BLEU-4(greedy of its image)), one more launch over the same rows.
    With a `rouge_scorer` (rouge.DeviceRougeL), `rouge_refs` and rouge_weight != 0: + rouge_weight * (ROUGE-L(sampled_b) -
    ROUGE-L(greedy of its image)) likewise; rouge_refs may be the very PreparedBleuRefs passed as bleu_refs (one layout).
    sampled (N, L) and greedy (NI, L) device id tensors, refs the PreparedRefs of the NI images (or their reference sets),
    image_of (N,) device index of each sample's image (None: row b belongs to image b % NI, the order of the repeated
    rollout).  The greedy captions are scored once per image; the difference is taken in double and then cast, as on the
    host.  Returns an (N, L) float32 device tensor; nothing is read back."""
    import torch
    if not isinstance(refs, PreparedRefs):
        refs = dscorer.prepare_refs(refs)
    N, NI = sampled.shape[0], greedy.shape[0]
    if sampled.shape[1] != greedy.shape[1]:
        raise ValueError("sampled and greedy captions differ in max_len: %d vs %d" % (sampled.shape[1], greedy.shape[1]))
    if NI != refs.n_sets:
        raise ValueError("%d greedy captions for %d reference sets" % (NI, refs.n_sets))
    dev = dscorer.dev
    own = torch.arange(NI, dtype=torch.int64, device=dev)
    image_of = own.repeat(-(-N // max(NI, 1)))[:N] if image_of is None else torch.as_tensor(image_of).reshape(-1).to(dev, torch.int64)
    rows, rows_set = torch.cat([sampled.to(dev), greedy.to(dev)], 0), torch.cat([image_of, own])
    s = dscorer.score_token_ids(rows, rows_set, refs)
    diff = cider_weight * (s[:N] - s[N:][image_of])
    for term, term_refs, weight, column, missing in (                                                     # in this order
            (bleu_scorer, bleu_refs, bleu_weight, 3,
             "the BLEU term needs bleu_refs: the images' reference sets or DeviceBleu.prepare_refs of them"),
            (rouge_scorer, rouge_refs, rouge_weight, None,
             "the ROUGE-L term needs rouge_refs: the images' reference sets or a device scorer's prepare_refs of them")):
        if term is not None and weight != 0.0:
            if term_refs is None:
                raise ValueError(missing)
            x = term.score_token_ids(rows, rows_set, term_refs)[1]
            x = x if column is None else x[:, column]
            diff = diff + weight * (x[:N] - x[N:][image_of])
    return diff.to(torch.float32)[:, None].expand(N, sampled.shape[1]).contiguous()
