"""Beam-search callers of the decode step: `evaluate()` of `editnet.py:595-718` / `dcnet.py:405-541` and the
EditNet+DCNet ensemble `evaluate_full()` of `eval/eval xe/eval_full.py:88-218`.

The reference searches ONE image at a time (batch = 1 image, beam k) and re-indexes ~11 tensors per step on
the host.  Here the search runs for MANY images at once, entirely on the device: per
timestep ONE fused decode step over all NI*k hypothesis rows, ONE beam epilogue kernel and ONE in-place state
re-index; the per-image entry points (`beam_search_editnet`, `beam_search_dcnet`, `beam_search_ensemble`,
the signatures a caller of the reference's loop needs) are the NI = 1 case of the same search.  One fix
relative to the reference text: parent = flat_index // vocab_size (the reference's `/` yields a float index on
torch >= 1.5).  Parity: tests/golden/beam_*.npz hold the outputs of the reference's own loops.
COCO scoring is out of scope.
"""
from __future__ import annotations

import torch


def sentence(seq, word_map):
    """editnet.py:715-716"""
    rev = {v: k for k, v in word_map.items()}
    skip = {word_map['<start>'], word_map['<end>'], word_map['<pad>']}
    return ' '.join(rev[w] for w in seq if w not in skip)


# ------------------------------------------------------------------------------------------------
# the same beam search for MANY images at once (the reference is batch 1), entirely
# on the device.  Per timestep: ONE fused decode step over all NI*k hypothesis rows (`set_editnet_step`,
# plus `set_dcnet_step` for the ensemble), ONE beam epilogue kernel (`set_beam_pick_f32`: log-softmax or
# ensemble averaging, flat top-k over k*V per image, the completed/live bookkeeping of editnet.py:666-699)
# and ONE in-place state re-index (`set_beam_gather_f32`).  The host only polls "all images finished"
# every few steps.  Semantics per image are those of editnet.py:643-713: k shrinks as hypotheses emit
# <end>; the answer is the best COMPLETED hypothesis (first maximum), or seqs[0][:18] at the step limit.
# ------------------------------------------------------------------------------------------------
class _FusedModel:
    """Prologue once per image, invariants replicated k times into a (NI*k)-row workspace.  `begin_args`: the tensors
    set_<abi>_begin takes between the dims and the workspace (one row per image); `step_args`: the per-image tensors whose
    k-fold replication set_<abi>_step takes in front of the words.  The model's `_beam_layout` gives the dims for k rows per image and the
    (name, per-row shape) table of the invariants the prologue leaves behind."""

    def __init__(self, model, begin_args, step_args, k, max_steps):
        import ctypes as C
        from . import _lib
        from ._lib import check, ptr, stream_of
        lib = _lib.load()
        begin, self._step = "set_%s_begin" % model._ABI, "set_%s_step" % model._ABI
        self.step_fn = getattr(lib, self._step)
        self.st = stream_of(model.fc.weight.device)
        dims_of, invariants = model._beam_layout(begin_args, max_steps)
        d_img = dims_of(1)
        self.w = model._weights(d_img)
        ws_img = model._new_workspace(d_img)
        check(getattr(lib, begin)(C.byref(self.w), C.byref(d_img), *(ptr(t) for t in begin_args), ptr(ws_img), ws_img.numel(),
                                  self.st), begin)
        self.dims = d_b = dims_of(k)
        NI, self.B = d_img.B, d_b.B
        self.ws = ws_b = model._new_workspace(d_b)
        for name, shp in invariants:
            model.ws_tensor(d_b, name, (self.B,) + shp, ws=ws_b).copy_(
                model.ws_tensor(d_img, name, (NI,) + shp, ws=ws_img).repeat_interleave(k, 0))
        self.step_args = [t.repeat_interleave(k, 0).contiguous() for t in step_args]      # (kept alive for step_ptrs)
        self.step_ptrs = tuple(ptr(t) for t in self.step_args)
        self.D = D = model.decoder_dim
        self.states = [model.ws_tensor(d_b, n, (self.B, D), ws=ws_b) for n in ("h1", "c1", "h2", "c2")]
        for s_ in self.states:
            s_.zero_()

    def step(self, words, logits):
        import ctypes as C
        from ._lib import check, ptr
        check(self.step_fn(C.byref(self.w), C.byref(self.dims), *self.step_ptrs, ptr(words), 1, self.B,
                           ptr(logits), logits.shape[1], ptr(self.ws), self.ws.numel(), self.st), self._step)


def _check_n_best(n_best, beam_size):
    """n_best=None: off.  Otherwise an integer in 1 .. beam_size (a search completes at most beam_size hypotheses)."""
    if n_best is None:
        return None
    m = int(n_best)
    if m != n_best or m < 1 or m > int(beam_size):
        raise ValueError("n_best must be an integer in 1 .. beam_size = %d, got %r" % (int(beam_size), n_best))
    return m


def _n_best_sorted(done, m):
    """[(tokens, score)] in completion order -> the m best: score descending, equal scores in completion order."""
    return sorted(done, key=lambda e: -e[1])[:m]


class BeamConstraints:
    """What a beam search may NOT pick (all eight beam_search_* entries, `constraints=`).  Constraints remove candidates before
    the flat top-k of every step, per hypothesis; nothing is renormalised, so scores stay sums of the model's log-probabilities.
      no_repeat_ngram=n (0: off, 1 .. 16): no n-gram of words occurs twice in a hypothesis (n = 1: no word twice)
      min_length=m (0: off): <end> only after at least m words
      length_penalty=a (0: off, finite, >= 0): completed hypotheses are RANKED by score / len^a, len = words including <end>; the
          returned scores and the n-best order are these rank scores (a = 0: the plain sums)
      banned_words: up to 64 token ids, or words looked up in the search's word_map; never <end>
    An all-default object is neutral: the search takes the unconstrained path, persistent launches included.  Otherwise the
    search runs per step with set_beam_pick_constrained_f32 (include/set_hip.h).  An image that runs out of candidates returns its
    best completed hypothesis, or ([<start>], nan) and an empty n-best list when nothing had completed."""

    def __init__(self, no_repeat_ngram=0, min_length=0, length_penalty=0.0, banned_words=()):
        import math
        for name, v, hi in (("no_repeat_ngram", no_repeat_ngram, 16), ("min_length", min_length, 2 ** 31 - 1)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= hi:
                raise ValueError("%s must be an integer in 0 .. %d, got %r" % (name, hi, v))
        a = float(length_penalty)
        if not math.isfinite(a) or a < 0.0:
            raise ValueError("length_penalty must be finite and >= 0, got %r" % (length_penalty,))
        banned = (banned_words,) if isinstance(banned_words, (str, int)) else tuple(banned_words)
        if len(banned) > 64:
            raise ValueError("at most 64 banned words, got %d" % len(banned))
        self.no_repeat_ngram, self.min_length, self.length_penalty, self.banned_words = int(no_repeat_ngram), int(min_length), a, banned

    def neutral(self):
        return self.no_repeat_ngram == 0 and self.min_length == 0 and self.length_penalty == 0.0 and not self.banned_words

    def banned_ids(self, word_map, V):
        """the banned token ids: ValueError for an unknown word, an id outside [0, V) and for <end>"""
        ids = []
        for w in self.banned_words:
            if isinstance(w, str):
                if w not in word_map:
                    raise ValueError("banned word %r is not in the word map" % w)
                w = word_map[w]
            if isinstance(w, bool) or int(w) != w or not 0 <= int(w) < V:
                raise ValueError("banned token id %r is outside [0, %d)" % (w, V))
            if int(w) == int(word_map['<end>']):
                raise ValueError("<end> cannot be banned (min_length delays it)")
            ids.append(int(w))
        return ids


def _active(constraints):
    """None for `constraints=None` and for a neutral object (today's path), the object otherwise"""
    if constraints is None:
        return None
    if not isinstance(constraints, BeamConstraints):
        raise TypeError("constraints must be an evaluate.BeamConstraints or None, got %s" % type(constraints).__name__)
    return None if constraints.neutral() else constraints


def _check_constraints(constraints, word_map, model):
    """what every beam_search_* entry does with `constraints=` before anything else: the active object (or None), its banned
    words resolved once against the model's vocabulary so that a bad one raises before any device work"""
    cons = _active(constraints)
    if cons is not None:
        cons.banned_ids(word_map, model.vocab_size)
    return cons


def _fused_models(model, inputs, k, max_steps):
    """(model or (decoder, dae), ([image_features,] previous_caption, prev_caplen)) -> (the _FusedModel list, X or None, prev, plen):
    the inputs as contiguous float / long tensors, the models in eval mode; with image features the first model is the EditNet"""
    prev = inputs[-2].long().contiguous()
    plen = inputs[-1].reshape(-1).long().contiguous()
    X = inputs[0].float().contiguous() if len(inputs) == 3 else None
    models = []
    for i, m in enumerate(model if isinstance(model, (tuple, list)) else (model,)):
        m.eval()
        models.append(_FusedModel(m, (X, None, prev, plen), (X,), k, max_steps) if i == 0 and X is not None else
                      _FusedModel(m, (prev, plen), (), k, max_steps))
    return models, X, prev, plen


def _gather(models, rows, NI, k, st):
    """one set_beam_gather_f32 per model: its four states re-indexed by the pick's rows"""
    from . import _lib
    from ._lib import check, ptr
    for m in models:
        s0, s1, s2, s3 = m.states
        check(_lib.load().set_beam_gather_f32(ptr(s0), ptr(s1), ptr(s2), ptr(s3), ptr(rows), NI, k, m.D, st), "set_beam_gather_f32")


class _BeamState:
    """What the per-step searches of NI images x k slots allocate alike.  done: the completion list (done_*, n_done).  two_launch:
    the pick is the constrained or the diverse one, which read their rows as float4 when the leading dimension allows it
    (V = 9490 is no multiple of 4): ld padded as _sbs_search pads it, the constraints struct (neutral for cons=None) and the
    candidate workspace.  The unconstrained picks keep ld = V.  scores start at -inf: the first step's live slots are the search's."""

    def __init__(self, n_models, NI, k, V, word_map, dev, max_steps, cons, done, two_launch):
        from . import _lib
        from ._lib import stream_of
        ids = cons.banned_ids(word_map, V) if cons is not None else []                           # (raises before any allocation)
        self.NI, self.k, self.V, self.max_steps, self.Lmax = NI, k, V, max_steps, max_steps + 2
        self.st = stream_of(dev)
        self.start, self.end = int(word_map['<start>']), int(word_map['<end>'])
        B, Lmax, neg = NI * k, self.Lmax, float("-inf")
        self.scores = torch.full((NI, k), neg, device=dev)
        self.k_left = torch.full((NI,), k, dtype=torch.int32, device=dev)
        self.words = torch.full((B,), self.start, dtype=torch.long, device=dev)
        self.rows = torch.empty(B, dtype=torch.int32, device=dev)
        self.seqs = [torch.full((NI, k, Lmax), self.start, dtype=torch.long, device=dev) for _ in range(2)]
        self.best_score = torch.full((NI,), neg, device=dev)
        self.best_seq = torch.zeros(NI, Lmax, dtype=torch.long, device=dev)
        self.best_len = torch.zeros(NI, dtype=torch.int32, device=dev)
        self.ld = (V + 63) // 64 * 64 if two_launch else V
        self.logits = [torch.empty(B, self.ld, dtype=torch.float32, device=dev) for _ in range(n_models)]
        if done:                                             # every counted <end> pick appends (score, tokens, length), set_hip.h
            self.done_score = torch.full((NI, k), neg, device=dev)
            self.done_seq = torch.zeros(NI, k, Lmax, dtype=torch.long, device=dev)
            self.done_len = torch.zeros(NI, k, dtype=torch.int32, device=dev)
            self.n_done = torch.zeros(NI, dtype=torch.int32, device=dev)
        if two_launch:
            self.banned = torch.tensor(ids, dtype=torch.long, device=dev) if ids else None       # (kept alive for copts)
            self.copts = _lib.BeamConstraintsC(*((cons.no_repeat_ngram, cons.min_length, cons.length_penalty) if cons is not None
                                                 else (0, 0, 0.0)), len(ids), self.banned.data_ptr() if ids else None)
            ws_bytes = int(_lib.load().set_beam_pick_constrained_workspace_bytes(NI, k))         # the diverse pick's is the same
            self.pick_ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)

    def pick_args(self, step):
        """what every set_beam_pick_* entry takes first: logits .. rows"""
        from ._lib import ptr
        lg = self.logits
        return (ptr(lg[0]), ptr(lg[1]) if len(lg) > 1 else None, self.ld, self.NI, self.k, self.V, self.end, step, self.Lmax,
                ptr(self.scores), ptr(self.k_left), ptr(self.seqs[0]), ptr(self.seqs[1]), ptr(self.best_score), ptr(self.best_seq),
                ptr(self.best_len), ptr(self.words), ptr(self.rows))

    def done_args(self):
        from ._lib import ptr
        return (ptr(self.done_score), ptr(self.done_seq), ptr(self.done_len), ptr(self.n_done))

    def ws_args(self):
        """what the constrained and the diverse pick take last: constraints, workspace, stream"""
        import ctypes as C
        from ._lib import ptr
        return (C.byref(self.copts), ptr(self.pick_ws), self.pick_ws.numel(), self.st)


def _beam_loop(models, s, pick, poll):
    """per timestep: every model steps on the same words into its own logits, pick(step), the seqs pair swaps, one state re-index
    per model; the host polls k_left every `poll` steps.  Returns the last step taken."""
    step = 1
    while True:
        for m, lg in zip(models, s.logits):
            m.step(s.words, lg)
        pick(step)
        s.seqs.reverse()
        _gather(models, s.rows, s.NI, s.k, s.st)
        if step > s.max_steps or (step % poll == 0 and int(s.k_left.max()) == 0):     # the only host synchronisation of the search
            return step
        step += 1


def _fused_beam(models, NI, k, V, word_map, dev, max_steps, poll=4, return_scores=False, n_best=None, constraints=None):
    from . import _lib
    from ._lib import check
    lib = _lib.load()
    cons = _active(constraints)
    s = _BeamState(len(models), NI, k, V, word_map, dev, max_steps, cons, n_best is not None or cons is not None, cons is not None)
    s.scores[:, 0] = 0.0                                 # step 1: all k rows are identical, only row 0 counts

    def pick(step):
        if cons is not None:
            check(lib.set_beam_pick_constrained_f32(*s.pick_args(step), *s.done_args(), *s.ws_args()), "set_beam_pick_constrained_f32")
        elif n_best is None:
            check(lib.set_beam_pick_f32(*s.pick_args(step), s.st), "set_beam_pick_f32")
        else:
            check(lib.set_beam_pick_nbest_f32(*s.pick_args(step), *s.done_args(), s.st), "set_beam_pick_nbest_f32")
    _beam_loop(models, s, pick, poll)
    start = s.start
    seqs_c, best_c, len_c, left_c, score_c = s.seqs[0].cpu(), s.best_seq.cpu(), s.best_len.cpu(), s.k_left.cpu(), s.best_score.cpu()
    out, out_scores = [], []
    for i in range(NI):
        if int(left_c[i]) > 0:                               # ran into the step limit (editnet.py:702-704,711)
            out.append(seqs_c[i, 0, :18].tolist())
            out_scores.append(float("nan"))
        elif int(len_c[i]) == 0:                             # constrained: ran out of candidates before anything completed
            out.append([start])
            out_scores.append(float("nan"))
        else:
            out.append(best_c[i, :int(len_c[i])].tolist())
            out_scores.append(float(score_c[i]))
    if n_best is None:
        return (out, out_scores) if return_scores else out
    ds_c, dq_c, dl_c, nd_c = s.done_score.cpu(), s.done_seq.cpu(), s.done_len.cpu(), s.n_done.cpu()
    nbest = [_n_best_sorted([(dq_c[i, j, :int(dl_c[i, j])].tolist(), float(ds_c[i, j])) for j in range(int(nd_c[i]))], n_best)
             for i in range(NI)]
    return (out, out_scores, nbest) if return_scores else (out, nbest)


def _with_trace(result, batched, return_scores, decoder, X, prev, plen, word_map, image_mean=None, n_best=None):
    """return_trace=True: the search's result + the EditTrace of the returned sequences (one forced decode of NI rows after
    the search; evaluate.edit_trace).  result: (tokens, score[, n-best]) of a per-image entry, the token lists (or (lists[,
    scores][, n-best])) of a batched one.  The trace is that of the PRIMARY result, with n_best too."""
    multi = return_scores or n_best is not None
    seqs = (result[0] if multi else result) if batched else [result[0]]
    tr = edit_trace(decoder, X, prev, plen, word_map, seqs, image_mean=image_mean)
    return (tuple(result) + (tr,)) if (not batched or multi) else (result, tr)


@torch.no_grad()
def beam_search_editnet_batched(decoder, image_features, previous_caption, prev_caplen, word_map, beam_size=3,
                                max_steps=50, return_scores=False, return_trace=False, n_best=None, constraints=None):
    """image_features (NI,R,F), previous_caption (NI,T), prev_caplen (NI,1) -> list of NI token lists
    (with return_scores: also the list of their scores; NaN where the step limit was hit).  The attention LSTM sees the mean
    over all R regions; adaptive features (zero-padded regions, an image mean per image): beam_search_adaptive_batched.
    n_best=m (1 <= m <= beam_size, all eight beam_search_* entries): the result gains, after the elements above, the N-BEST
    lists — per image up to m (tokens, score) pairs of its COMPLETED hypotheses, tokens with <start> and <end>, score descending
    and equal scores in completion order (by pick, within a pick by pick rank).  When the search finished, entry 0 is the
    primary result; a search that hit the step limit keeps the reference's primary answer (seqs[0][:18], NaN) and lists what
    had completed by then, possibly nothing.  The trace of an alternative is one more forced decode:
        seqs, nbest = beam_search_editnet_batched(dec, X, prev, plen, wm, 3, n_best=3)
        runner_up = nbest[i][1][0]                      # tokens of image i's second-best completed hypothesis
        tr = edit_trace(dec, X[i:i + 1], prev[i:i + 1], plen[i:i + 1], wm, [runner_up])
    constraints=BeamConstraints(...) (all eight beam_search_* entries): n-gram blocking, banned words, a minimum length and
    length-normalised ranking inside the pick; None or a neutral object: this search, unchanged.  Scores and the n-best order are
    then the rank scores; the trace is that of the constrained tokens.
    return_trace: the result gains the EditTrace of the returned (primary) sequences as its last element."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, decoder)
    ms, X, prev, plen = _fused_models(decoder, (image_features, previous_caption, prev_caplen), beam_size, max_steps)
    res = _fused_beam(ms, X.shape[0], beam_size, decoder.vocab_size, word_map, X.device, max_steps,
                      return_scores=return_scores, n_best=n_best, constraints=cons)
    return _with_trace(res, True, return_scores, decoder, X, prev, plen, word_map, n_best=n_best) if return_trace else res


@torch.no_grad()
def beam_search_dcnet_batched(dae, previous_caption, prev_caplen, word_map, beam_size=3, max_steps=50,
                              return_scores=False, n_best=None, constraints=None):
    """n_best, constraints: see beam_search_editnet_batched."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, dae)
    ms, _, prev, _ = _fused_models(dae, (previous_caption, prev_caplen), beam_size, max_steps)
    return _fused_beam(ms, prev.shape[0], beam_size, dae.vocab_size, word_map, prev.device, max_steps,
                       return_scores=return_scores, n_best=n_best, constraints=cons)


@torch.no_grad()
def beam_search_ensemble_batched(decoder, dae, image_features, previous_caption, prev_caplen, word_map, beam_size=3,
                                 max_steps=50, return_scores=False, return_trace=False, n_best=None, constraints=None):
    """eval_full.py:88-218 for NI images at once: both models step on the same words, the epilogue averages
    their softmax probabilities.  Fixed features (image mean over all R regions); adaptive features: beam_search_adaptive*.
    n_best, constraints: see beam_search_editnet_batched (the scores are those of the joint pick).
    return_trace: the result gains, as its last element, EditNet's view of the jointly chosen words (their EditTrace)."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, decoder)
    ms, X, prev, plen = _fused_models((decoder, dae), (image_features, previous_caption, prev_caplen), beam_size, max_steps)
    res = _fused_beam(ms, X.shape[0], beam_size, decoder.vocab_size, word_map, X.device, max_steps,
                      return_scores=return_scores, n_best=n_best, constraints=cons)
    return _with_trace(res, True, return_scores, decoder, X, prev, plen, word_map, n_best=n_best) if return_trace else res


# ------------------------------------------------------------------------------------------------
# The reference's calling convention: one image per call (editnet.py:601-613, dcnet.py:413-423,
# eval_full.py:96-109) -> (token list incl. <start>/<end>, score of the chosen hypothesis; NaN if the
# 50-step limit was hit).  NI = 1 case of the batched on-device search above.
# ------------------------------------------------------------------------------------------------
class _PersistentBeamOut:
    """Outputs of one persistent beam launch (set_editnet_beam_persistent / set_dcnet_beam_persistent), all in ONE device
    buffer: [hist_word (picks, 4) i64 | best_word i64 | hist_parent (picks, 4) i32 | result (4) i32 | best_score f32 | pad],
    with n_best=True followed by [hist_score (picks, 4) f32] (the *_nbest entries), read back with a single copy (the search's
    only host synchronisation)."""

    def __init__(self, picks, dev, n_best=False):
        self.picks = picks
        self.n_hw, self.n_hp = picks * 4 * 8, picks * 4 * 4
        self.o_hs = self.n_hw + 8 + self.n_hp + 16 + 8
        self.buf = torch.empty(self.o_hs + (picks * 4 * 4 if n_best else 0), dtype=torch.uint8, device=dev)
        base = self.buf.data_ptr()
        self.o_hp, self.o_res = self.n_hw + 8, self.n_hw + 8 + self.n_hp
        self.o_bs = self.o_res + 16
        self.hist_word, self.best_word, self.hist_parent = base, base + self.n_hw, base + self.o_hp
        self.result, self.best_score = base + self.o_res, base + self.o_bs
        self.hist_score = base + self.o_hs if n_best else None

    def answer(self, word_map, name, n_best=None, k=4):
        """(tokens, score): the best completed hypothesis, or the step-limit rule of the reference (editnet.py:702-704,711,
        dcnet.py:503-505,512: seqs[0][:18], score NaN).  n_best=m: (tokens, score, the m best completed hypotheses) — the
        completions of pick t are the slots s < k (the others are never written) with hist_word == <end> and hist_score > -inf, in
        slot order (set_hip.h)."""
        from . import _lib
        picks, n_hw, n_hp, o_hp, o_res, o_bs = self.picks, self.n_hw, self.n_hp, self.o_hp, self.o_res, self.o_bs
        host = self.buf.cpu().numpy()
        hw = host[:n_hw].view("int64").reshape(picks, 4)
        hp = host[o_hp:o_hp + n_hp].view("int32").reshape(picks, 4)
        best_t, best_parent, k_left, made = (int(v) for v in host[o_res:o_res + 16].view("int32"))
        best_word_h = int(host[n_hw:n_hw + 8].view("int64")[0])
        best_score_h = float(host[o_bs:o_bs + 4].view("float32")[0])
        if made < 0:
            raise _lib.SetError("%s: the persistent launch timed out (result poisoned)" % name)

        def trace(t_last, slot):
            out = []
            for t in range(t_last, -1, -1):
                out.append(int(hw[t, slot]))
                slot = int(hp[t, slot])
            return out[::-1]

        start = int(word_map['<start>'])
        if k_left > 0:                                                 # ran into the step limit
            one = ([start] + trace(made - 1, 0))[:18], float("nan")
        else:
            one = [start] + trace(best_t - 1, best_parent) + [best_word_h], best_score_h
        if n_best is None:
            return one
        hs = host[self.o_hs:self.o_hs + n_hp].view("float32").reshape(picks, 4)
        end = int(word_map['<end>'])
        done = [([start] + trace(t, s), float(hs[t, s])) for t in range(made) for s in range(k)
                if int(hw[t, s]) == end and hs[t, s] > float("-inf")]
        return one + (_n_best_sorted(done, n_best),)


def _persistent_beam(name, head, tail, word_map, k, picks, dev, n_best):
    """What the three persistent searches share once their own guards have passed: the output buffer, the C entry's argument
    list (the caller's leading arguments `head`, then <start>, <end>, picks and the five output pointers, then the caller's
    workspaces `tail` and the stream), the choice of `name` or `name`_nbest (the same launch, plus the score of every counted
    pick), and the answer.  None on SET_ERR_UNSUPPORTED: no output was touched (set_hip.h: answered before the prologue except
    on a device too small for the grid)."""
    from . import _lib
    lib = _lib.load()
    out = _PersistentBeamOut(picks, dev, n_best is not None)
    args = head + (int(word_map['<start>']), int(word_map['<end>']), picks, out.hist_parent, out.hist_word, out.best_score,
                   out.best_word, out.result) + tail + (_lib.stream_of(dev),)
    rc = getattr(lib, name)(*args) if n_best is None else getattr(lib, name + "_nbest")(*args, out.hist_score)
    if rc == 2:
        return None
    _lib.check(rc, name)
    return out.answer(word_map, name, n_best, k)


@torch.no_grad()
def _beam_search_editnet_persistent(decoder, image_features, previous_caption, prev_caplen, word_map, beam_size, max_steps=50,
                                    image_mean=None, n_best=None):
    """ONE image, k <= 4: prologue + one persistent launch for the whole search (include/set_hip.h
    set_editnet_beam_persistent; the rows of the launch are the k hypotheses).  Returns None when the library answers
    SET_ERR_UNSUPPORTED (no token table yet, k > 4, dimensions outside the persistent launch): the caller takes the
    per-step search.  image_mean (1, F): the adaptive model's image input (beam_search_adaptive); an adaptive decoder
    without one is refused here (the fixed-feature entries keep their routing)."""
    import ctypes as C
    from ._lib import ptr
    k = int(beam_size)
    if k < 1 or k > 4 or image_features.shape[0] != 1 or (getattr(decoder, "_adaptive", 0) and image_mean is None):
        return None
    decoder.eval()
    X = image_features.float().expand(k, -1, -1).contiguous()
    prev = previous_caption.long().expand(k, -1).contiguous()
    plen = prev_caplen.reshape(-1).long().expand(k).contiguous()
    mean = None if image_mean is None else image_mean.float().reshape(1, -1).expand(k, -1).contiguous()
    picks = max_steps + 1
    dims = decoder._dims(k, prev.shape[1], X.shape[1], picks)
    w = decoder._weights(dims)
    if not w.tok_table:
        return None
    ws = decoder._workspace(dims)
    return _persistent_beam("set_editnet_beam_persistent",
                            (C.byref(w), C.byref(dims), ptr(X), None if mean is None else ptr(mean), ptr(prev), ptr(plen)),
                            (ptr(ws), ws.numel()), word_map, k, picks, X.device, n_best)


def _first(res):
    """the NI = 1 batched result (lists, scores[, n-best lists]) as a per-image one"""
    return tuple(r[0] for r in res)


def beam_search_editnet(decoder, image_features, previous_caption, prev_caplen, word_map, beam_size=3, return_trace=False,
                        n_best=None, constraints=None):
    """The reference's own calling convention, ONE image per call (editnet.py:601-613).  k <= 4 with the token table
    active: one persistent launch (csrc/decode_persistent_wide.hip, beam mode); otherwise the NI = 1 case of the batched
    search.  Adaptive features (an image mean per image, zero-padded regions): beam_search_adaptive.
    n_best=m: (tokens, score, [(tokens, score)] of up to m completed hypotheses, best first) — see
    beam_search_editnet_batched; the routing is the same, and an entry's tokens go to edit_trace as they are:
        tokens, score, nbest = beam_search_editnet(dec, X, prev, plen, wm, 3, n_best=3)
        tr = edit_trace(dec, X, prev, plen, wm, [nbest[1][0]])         # the runner-up's trace
    constraints: see beam_search_editnet_batched; active constraints take the per-step search (its NI = 1 case) at every k.
    return_trace: (tokens, score[, n-best], EditTrace of the returned tokens)."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, decoder)
    one = None if cons is not None else _beam_search_editnet_persistent(decoder, image_features, previous_caption, prev_caplen,
                                                                        word_map, beam_size, n_best=n_best)
    if one is None:
        one = _first(beam_search_editnet_batched(decoder, image_features, previous_caption, prev_caplen, word_map, beam_size,
                                                 return_scores=True, n_best=n_best, constraints=cons))
    if return_trace:
        return _with_trace(one, False, True, decoder, image_features, previous_caption, prev_caplen, word_map)
    return one


@torch.no_grad()
def _beam_search_dcnet_persistent(dae, previous_caption, prev_caplen, word_map, beam_size, max_steps=50, n_best=None):
    """ONE previous caption, k <= 4: prologue + one persistent launch for the whole search (include/set_hip.h
    set_dcnet_beam_persistent; the rows of the launch are the k hypotheses).  Returns None when the library answers
    SET_ERR_UNSUPPORTED (no token table yet, k > 4, dimensions outside the persistent launch, SET_DEC_PERSISTENT=0): the
    caller takes the per-step search.  Output buffer, read-back, trace-back and step-limit rule: _PersistentBeamOut, shared
    with _beam_search_editnet_persistent."""
    import ctypes as C
    from ._lib import ptr
    k = int(beam_size)
    if k < 1 or k > 4 or previous_caption.shape[0] != 1:
        return None
    dae.eval()
    prev = previous_caption.long().expand(k, -1).contiguous()
    plen = prev_caplen.reshape(-1).long().expand(k).contiguous()
    picks = max_steps + 1
    dims = dae._dims(k, prev.shape[1], picks)
    w = dae._weights(dims)
    if not w.tok_table:
        return None
    ws = dae._workspace(dims)
    return _persistent_beam("set_dcnet_beam_persistent", (C.byref(w), C.byref(dims), ptr(prev), ptr(plen)), (ptr(ws), ws.numel()),
                            word_map, k, picks, prev.device, n_best)


def beam_search_dcnet(dae, previous_caption, prev_caplen, word_map, beam_size=3, n_best=None, constraints=None):
    """The reference's own calling convention, ONE previous caption per call (dcnet.py:413-423).  k <= 4 with the token table
    active: one persistent launch (csrc/decode_persistent.hip, beam mode); otherwise the NI = 1 case of the batched search.
    n_best=m: (tokens, score, [(tokens, score)] of up to m completed hypotheses, best first), see beam_search_editnet_batched.
    constraints: see beam_search_editnet_batched; active constraints take the per-step search at every k."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, dae)
    one = None if cons is not None else _beam_search_dcnet_persistent(dae, previous_caption, prev_caplen, word_map, beam_size,
                                                                      n_best=n_best)
    if one is not None:
        return one
    return _first(beam_search_dcnet_batched(dae, previous_caption, prev_caplen, word_map, beam_size, return_scores=True,
                                            n_best=n_best, constraints=cons))


_ens_xbuf = {}                 # exchange regions of the ensemble's persistent launch, one per (bytes, device, stream)


@torch.no_grad()
def _beam_search_ensemble_persistent(decoder, dae, image_features, previous_caption, prev_caplen, word_map, beam_size, max_steps=50,
                                     n_best=None):
    """ONE image, k <= 4, the EditNet + DCNet ensemble (eval_full.py:132-202): both prologues + one persistent launch that holds
    both models' state for the whole search (include/set_hip.h set_ensemble_beam_persistent; the rows of the launch are the k
    hypotheses).  Returns None when the library answers SET_ERR_UNSUPPORTED (a token table missing, k > 4, dimensions outside
    the launch, SET_DEC_PERSISTENT=0) and on the host-side checks (more than one image, vocabularies of different size, an
    adaptive decoder: the reference's ensemble uses fixed features): the caller takes the per-step search.  The modules' cached
    workspaces serve the prologues; the launch's exchange region is a buffer of its own.  Output buffer, read-back, trace-back
    and step-limit rule: _PersistentBeamOut, shared with the single-model searches."""
    import ctypes as C
    from . import _lib
    from ._lib import ptr
    k = int(beam_size)
    if (k < 1 or k > 4 or image_features.shape[0] != 1 or previous_caption.shape[0] != 1 or getattr(decoder, "_adaptive", 0)
            or decoder.vocab_size != dae.vocab_size):
        return None
    decoder.eval()
    dae.eval()
    dev = image_features.device
    X = image_features.float().expand(k, -1, -1).contiguous()
    prev = previous_caption.long().expand(k, -1).contiguous()
    plen = prev_caplen.reshape(-1).long().expand(k).contiguous()
    picks = max_steps + 1
    de = decoder._dims(k, prev.shape[1], X.shape[1], picks)
    dd = dae._dims(k, prev.shape[1], picks)
    we, wd = decoder._weights(de), dae._weights(dd)
    if not we.tok_table or not wd.tok_table:
        return None
    nx = _lib.load().set_ensemble_beam_xbuf_bytes(C.byref(de), C.byref(dd))
    if nx == 0:
        return None
    ws_e, ws_d = decoder._workspace(de), dae._workspace(dd)
    key = (nx, str(dev), torch.cuda.current_stream(dev).cuda_stream)
    xbuf = _ens_xbuf.get(key)
    if xbuf is None:
        if len(_ens_xbuf) >= 8:
            _ens_xbuf.clear()
        xbuf = _ens_xbuf[key] = torch.empty(nx, dtype=torch.uint8, device=dev)
    return _persistent_beam("set_ensemble_beam_persistent",
                            (C.byref(we), C.byref(de), C.byref(wd), C.byref(dd), ptr(X), ptr(prev), ptr(plen)),
                            (ptr(ws_e), ws_e.numel(), ptr(ws_d), ws_d.numel(), ptr(xbuf), xbuf.numel()), word_map, k, picks, dev, n_best)


def beam_search_ensemble(decoder, dae, image_features, previous_caption, prev_caplen, word_map, beam_size=3,
                         return_trace=False, n_best=None, constraints=None):
    """The reference's published protocol, ONE image per call (eval_full.py:88-237).  k <= 4 with both token tables active: one
    persistent launch (csrc/decode_persistent_ensemble.hip); otherwise the NI = 1 case of the batched search.
    n_best=m: (tokens, score, [(tokens, score)] of up to m completed hypotheses, best first), see beam_search_editnet_batched.
    constraints: see beam_search_editnet_batched; active constraints take the per-step search at every k.
    return_trace: (tokens, score[, n-best], EditNet's EditTrace of the jointly chosen tokens)."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, decoder)
    one = None if cons is not None else _beam_search_ensemble_persistent(decoder, dae, image_features, previous_caption, prev_caplen,
                                                                         word_map, beam_size, n_best=n_best)
    if one is None:
        one = _first(beam_search_ensemble_batched(decoder, dae, image_features, previous_caption, prev_caplen, word_map, beam_size,
                                                  return_scores=True, n_best=n_best, constraints=cons))
    if return_trace:
        return _with_trace(one, False, True, decoder, image_features, previous_caption, prev_caplen, word_map)
    return one


# ------------------------------------------------------------------------------------------------
# Adaptive features (adaptive_features/editnet_adaptive.py:614-735): the same search, with the image mean that comes with
# every image (the mean over its VALID regions) as the attention LSTM's input and the zero-padded regions masked in the
# visual attention (the region mask of the prologue, replicated with the other invariants).
# ------------------------------------------------------------------------------------------------
def _adaptive_args(decoder, image_features, image_mean):
    if not getattr(decoder, "_adaptive", 0):
        raise TypeError("beam_search_adaptive*: %s is not an adaptive-features decoder (editnet_adaptive.DecoderC); "
                        "fixed features: beam_search_editnet*" % type(decoder).__name__)
    X = image_features.float().contiguous()
    NI, _, F = X.shape
    if image_mean is None or tuple(image_mean.shape) != (NI, F):
        raise ValueError("beam_search_adaptive*: image_mean must have shape (NI, F) = (%d, %d), got %s"
                         % (NI, F, None if image_mean is None else tuple(image_mean.shape)))
    return X, image_mean.to(X.device).float().contiguous()


@torch.no_grad()
def beam_search_adaptive_batched(decoder, image_features, image_mean, previous_caption, prev_caplen, word_map, beam_size=3,
                                 max_steps=50, return_scores=False, return_trace=False, n_best=None, constraints=None):
    """image_features (NI,R,F) zero-padded regions, image_mean (NI,F), previous_caption (NI,T), prev_caplen (NI,1) ->
    list of NI token lists (with return_scores: also their scores; NaN where the step limit was hit).  NI images at once
    on the per-step fused kernels.  n_best, constraints: see beam_search_editnet_batched."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, decoder)
    X, mean = _adaptive_args(decoder, image_features, image_mean)
    decoder.eval()
    prev = previous_caption.long().contiguous()
    plen = prev_caplen.reshape(-1).long().contiguous()
    m = _FusedModel(decoder, (X, mean, prev, plen), (X,), beam_size, max_steps)
    res = _fused_beam([m], X.shape[0], beam_size, decoder.vocab_size, word_map, X.device, max_steps,
                      return_scores=return_scores, n_best=n_best, constraints=cons)
    return (_with_trace(res, True, return_scores, decoder, X, prev, plen, word_map, image_mean=mean, n_best=n_best)
            if return_trace else res)


def beam_search_adaptive(decoder, image_features, image_mean, previous_caption, prev_caplen, word_map, beam_size=3,
                         return_trace=False, n_best=None, constraints=None):
    """The reference's adaptive evaluate(), ONE image per call (editnet_adaptive.py:620-735) -> (tokens, score).  k <= 4
    with the token table active: one persistent launch (beam mode over up to 128 masked regions, even R); otherwise the
    NI = 1 case of beam_search_adaptive_batched.  n_best=m: (tokens, score, [(tokens, score)] of up to m completed hypotheses,
    best first), see beam_search_editnet_batched.  constraints: see there; active constraints take the per-step search at every k."""
    n_best = _check_n_best(n_best, beam_size)
    cons = _check_constraints(constraints, word_map, decoder)
    X, mean = _adaptive_args(decoder, image_features, image_mean)
    one = None if cons is not None else _beam_search_editnet_persistent(decoder, X, previous_caption, prev_caplen, word_map, beam_size,
                                                                        image_mean=mean, n_best=n_best)
    if one is None:
        one = _first(beam_search_adaptive_batched(decoder, X, mean, previous_caption, prev_caplen, word_map, beam_size,
                                                  return_scores=True, n_best=n_best, constraints=cons))
    if return_trace:
        return _with_trace(one, False, True, decoder, X, previous_caption, prev_caplen, word_map, image_mean=mean)
    return one


# ------------------------------------------------------------------------------------------------
# Edit trace: the per-word record behind the reference's demo figure — attention over the existing caption, the position the
# hard selection took, and whether the Copy-LSTM copied the selected memory or edited it.  The recurrent state depends on
# the token prefix only, so the trace of ANY decoder output (greedy, sampled, beam, ensemble, a ground-truth caption) is the
# teacher-forced, no-grad decode of those tokens (include/set_hip.h set_editnet_edit_trace; per-step kernels, the
# persistent launches are not tapped).  EditNet only: DCNet has neither a selection nor a copy gate.
# ------------------------------------------------------------------------------------------------
class EditTrace:
    """Record of a forced decode of `tokens` (B, S + 1; `<start>` first): step t describes how tokens[b, t + 1] was produced.
    alpha_c (B, S, T) caption-attention weights, select (B, S) int32 its arg-max position (-1 where t >= n_steps[b]),
    copy_gate (B, S) mean over D of the Copy-LSTM's gate, gate_full (B, S, D) the gate, alpha_v (B, S, R) visual attention
    weights, logp (B, S) log-probability of the forced word; everything at t >= n_steps[b] is 0."""

    def __init__(self, alpha_c, select, copy_gate, gate_full, alpha_v, logp, n_steps, tokens, previous_caption):
        self.alpha_c, self.select, self.copy_gate, self.gate_full = alpha_c, select, copy_gate, gate_full
        self.alpha_v, self.logp, self.n_steps, self.tokens = alpha_v, logp, n_steps, tokens
        self.previous_caption = previous_caption

    @property
    def copied(self):
        """(B, S) bool: the produced word IS the selected word of the previous caption (the figure's copy / edit label)."""
        sel = self.select.long()
        live = sel >= 0
        picked = self.previous_caption.long().gather(1, sel.clamp(min=0))
        return live & (self.tokens[:, 1:sel.shape[1] + 1] == picked)

    def rows(self, word_map):
        """per image: [(word, selected previous word, copy_gate, copied)] for its n_steps recorded steps"""
        rev = {v: k for k, v in word_map.items()}
        tok, prev = self.tokens.cpu().tolist(), self.previous_caption.cpu().tolist()
        sel, gate, cop = self.select.cpu().tolist(), self.copy_gate.cpu().tolist(), self.copied.cpu().tolist()
        out = []
        for b, n in enumerate(self.n_steps.cpu().tolist()):
            out.append([(rev[tok[b][t + 1]], rev[prev[b][sel[b][t]]], float(gate[b][t]), bool(cop[b][t])) for t in range(n)])
        return out


@torch.no_grad()
def sample_captions(model, *inputs_and_word_map, n_samples=5, temperature=1.0, top_k=0, top_p=1.0, sampler="cdf",
                    constraints=None):
    """n_samples sampled captions per image from ONE fused rollout:
        seq, seq_logp = sample_captions(decoder, image_features, previous_caption, prev_caplen, word_map, n_samples=5, top_p=0.9)
        seq, seq_logp = sample_captions(dae, previous_caption, prev_caplen, word_map, temperature=0.8, top_k=50)
    EditNet (editnet_rl.DecoderC) takes image_features (NI,R,F), previous_caption (NI,T), prev_caplen (NI,1); DCNet
    (dcnet_rl.DAE) the caption pair only.  Every image's rows are repeated n_samples times (row i * n_samples + j is sample j of
    image i): the rows differ in their index, hence in their Philox counters, hence in their draws.  Returns seq (NI, n_samples,
    max_len) int64 and seq_logp (NI, n_samples, max_len), the log-probs under the tempered / truncated distribution sampled
    from.  The seed comes from rng.next_seed() as in the models' own sampled path: torch.manual_seed() reproduces a call.
    sampler="gumbel": the Gumbel-max draw (temperature only) — for n_samples * NI <= 16 rows (EditNet) or <= 8 rows (DCNet) the
    whole rollout is one persistent launch; "cdf" (default) is the inverse-CDF draw with its draws unchanged.
    constraints: an evaluate.BeamConstraints applied to every sample's own words (see editnet_rl.DecoderC.forward; sampler="cdf")."""
    *inputs, word_map = inputs_and_word_map
    if len(inputs) not in (2, 3):
        raise ValueError("sample_captions(model, [image_features,] previous_caption, prev_caplen, word_map, ...)")
    n = int(n_samples)
    if n < 1:
        raise ValueError("n_samples must be >= 1, got %r" % (n_samples,))
    model.eval()
    prev = inputs[-2].long().repeat_interleave(n, 0).contiguous()
    plen = inputs[-1].reshape(-1).long().repeat_interleave(n, 0).contiguous()
    kw = dict(sample_max=False, sample_rl=True, temperature=temperature, top_k=top_k, top_p=top_p)
    if sampler != "cdf":
        kw["sampler"] = sampler
    if constraints is not None:
        kw["constraints"] = constraints
    if len(inputs) == 3:
        X = inputs[0].float().repeat_interleave(n, 0).contiguous()
        seq, logp = model(word_map, prev, plen, X, **kw)
    else:
        seq, logp = model(word_map, prev, plen, **kw)
    NI = seq.shape[0] // n
    return seq.view(NI, n, -1), logp.view(NI, n, -1)


SBS_MAX_SAMPLES = 8     # slots of set_sbs_pick_f32


def _sbs_slots(n_samples, return_threshold):
    """(n, slots of the search): return_threshold takes one slot more, so n_samples <= 7 with it"""
    k = int(n_samples)
    top = SBS_MAX_SAMPLES - (1 if return_threshold else 0)
    if k != n_samples or k < 1 or k > top:
        raise ValueError("n_samples must be an integer in 1 .. %d%s, got %r"
                         % (top, " with return_threshold (the threshold is one more slot)" if return_threshold else "", n_samples))
    return k, k + (1 if return_threshold else 0)


def _sbs_max_steps(model, max_steps):
    max_steps = int(getattr(model, "max_len", 18) if max_steps is None else max_steps)
    if max_steps < 1 or max_steps > 255:
        raise ValueError("max_steps must lie in 1 .. 255, got %r" % (max_steps,))
    return max_steps


def _sbs_search(models, NI, k, V, word_map, dev, max_steps, opts, return_steps):
    """The stochastic beam search of NI images x k slots over one _FusedModel (set_sbs_pick_opts_f32) or the EditNet + DCNet
    pair (set_sbs_pick_ensemble_opts_f32; opts: temperature, top_k, top_p, or None): per timestep every model steps on the same
    words into its own padded logits, the pick, one set_beam_gather_f32 per model with the pick's rows; the host polls "no open
    slot" every 4 steps.  Returns (per image the live slots' (tokens, logp, G, finished) in draw order, the per-step logits when
    asked for: a tensor per step for one model, a tuple of two for the pair)."""
    import ctypes as C
    from . import _lib, rng
    from ._lib import check, ptr, stream_of
    lib = _lib.load()
    st = stream_of(dev)
    start, end = int(word_map['<start>']), int(word_map['<end>'])
    B, neg = NI * k, float("-inf")
    phi = torch.zeros(NI, k, device=dev)
    G = torch.full((NI, k), neg, device=dev)
    G[:, 0] = 0.0                                        # step 0: the k rows are identical, only slot 0 is live
    fin = torch.zeros(NI, k, dtype=torch.int32, device=dev)
    length = torch.zeros(NI, k, dtype=torch.int32, device=dev)
    n_open = torch.ones(NI, dtype=torch.int32, device=dev)
    seqs = [torch.zeros(NI, k, max_steps, dtype=torch.long, device=dev) for _ in range(2)]
    words = torch.full((B,), start, dtype=torch.long, device=dev)
    rows = torch.empty(B, dtype=torch.int32, device=dev)
    # the leading dimension padded as the rollouts' workspace logits are: the pick then reads its rows as float4 (its register
    # path needs ld % 4 == 0; V = 9490 is no multiple of 4), the step writes V columns of every row
    ld = (V + 63) // 64 * 64
    logits = [torch.empty(B, ld, dtype=torch.float32, device=dev) for _ in models]
    ws = torch.empty(lib.set_sbs_workspace_bytes(NI, k), dtype=torch.uint8, device=dev)
    a = _lib.SbsArgs(logits=logits[0].data_ptr(), ld=ld, end_idx=end, seed=rng.next_seed(), offset=rng.offset(rng.SITE_ROLLOUT),
                     phi=phi.data_ptr(), G=G.data_ptr(), finished=fin.data_ptr(), len=length.data_ptr(),
                     words=words.data_ptr(), rows=rows.data_ptr(), n_open=n_open.data_ptr(), ws=ws.data_ptr(),
                     ws_bytes=ws.numel(), NI=NI, k=k, V=V, Lmax=max_steps)
    o = C.byref(opts) if opts is not None else None
    steps = []
    for t in range(max_steps):
        for m, lg in zip(models, logits):
            m.step(words, lg)
        if return_steps:
            got = tuple(lg[:, :V].clone() for lg in logits)
            steps.append(got[0] if len(models) == 1 else got)
        a.t, a.seqs_in, a.seqs_out = t, seqs[0].data_ptr(), seqs[1].data_ptr()
        if len(models) == 1:
            check(lib.set_sbs_pick_opts_f32(C.byref(a), o, st), "set_sbs_pick_opts_f32")
        else:
            check(lib.set_sbs_pick_ensemble_opts_f32(C.byref(a), ptr(logits[1]), o, st), "set_sbs_pick_ensemble_opts_f32")
        seqs.reverse()
        if t + 1 == max_steps:
            break
        _gather(models, rows, NI, k, st)
        if (t + 1) % 4 == 0 and int(n_open.max()) == 0:          # the only host synchronisation of the search
            break
    seqs_c, phi_c, G_c, fin_c, len_c = seqs[0].cpu(), phi.cpu(), G.cpu(), fin.cpu(), length.cpu()
    out = []
    for i in range(NI):
        entries = []
        for j in range(k):
            if float(G_c[i, j]) == neg:
                continue
            n = int(len_c[i, j])
            tk = [0 if w == end else w for w in seqs_c[i, j, :n].tolist()]
            entries.append((tk + [0] * (max_steps - n), float(phi_c[i, j]), float(G_c[i, j]), bool(fin_c[i, j])))
        out.append(entries)
    return out, steps


def _sbs_answer(out, steps, n, return_threshold, return_steps):
    """the public return convention: out[, kappa][, steps]; with the threshold, the search ran n + 1 slots: the first n entries
    are the sample and the G of entry n + 1 bounds everything that was not returned (-inf: there is nothing else)"""
    res = (out,)
    if return_threshold:
        res = ([e[:n] for e in out], [e[n][2] if len(e) > n else float("-inf") for e in out])
    if return_steps:
        res = res + (steps,)
    return res[0] if len(res) == 1 else res


@torch.no_grad()
def sample_captions_distinct(model, *inputs_and_word_map, n_samples=5, temperature=1.0, top_k=0, top_p=1.0, max_steps=None,
                             return_threshold=False, _return_steps=False):
    """Up to n_samples DISTINCT captions per image, an exact sample WITHOUT replacement from the model's (tempered) sequence
    distribution, by stochastic beam search (Kool, van Hoof, Welling, ICML 2019; include/set_hip.h set_sbs_pick_f32 /
    set_sbs_pick_opts_f32):
        out = sample_captions_distinct(decoder, image_features, previous_caption, prev_caplen, word_map, n_samples=5)
        out = sample_captions_distinct(decoder, image_features, previous_caption, prev_caplen, word_map, n_samples=5, top_p=0.9)
        out = sample_captions_distinct(dae, previous_caption, prev_caplen, word_map, temperature=0.8)
    EditNet (editnet_rl.DecoderC, fixed features) takes image_features (NI,R,F), previous_caption (NI,T), prev_caplen (NI,1);
    DCNet (dcnet_rl.DAE) the caption pair only.  One beam-shaped pass for all images: per timestep one decode step over the
    NI * n_samples slots, the pick, one state re-index; the host polls "no open slot" every 4 steps.  Finished sequences stay in
    the beam and compete; nothing is deterministic about the result but its seed, which comes from rng.next_seed() as in the
    sampled rollout (torch.manual_seed() reproduces a call).
    Returns, per image, a list of up to n_samples entries (tokens, logp, G, finished) in DRAW order (G descending): tokens is a
    list of max_steps words in the sampled rollouts' convention (<end> stored as 0, zeros behind it; tokens_from_greedy takes
    them), logp the sequence's log-probability under the tempered, truncated model, G its perturbed log-probability.  max_steps
    defaults to the sampled rollout's max_len; a sequence still open at the limit is returned as it is, with finished=False.
    Fewer than n_samples entries come back only when the model gives fewer sequences a non-zero probability.
    top_k / top_p (sample_captions' options; 0 / 1.0: off) cut every step's word distribution to the top_k most probable words
    and then to the smallest head holding top_p of their mass (ties kept whole), renormalised: the result is the exact sample
    without replacement from that TRUNCATED model, logp is the log-probability under it, and no returned sequence holds a word
    outside its step's kept set.  The truncated model has fewer sequences: with top_k=1 it has one, so exactly one entry comes
    back per image (the greedy words, logp = G = 0).  Neutral values return what the call without them returns.
    return_threshold=True: returns (out, kappa).  The search runs n_samples + 1 slots; out[i] holds the first n_samples entries
    and kappa[i] is the G of entry n_samples + 1 (-inf when the model, truncated if top_k / top_p say so, gives no further
    sequence a non-zero probability).  A search with m slots returns the m sequences with the largest perturbed scores, so
    kappa[i] bounds the G of everything not returned: the threshold that sbs_importance_weights needs, after
    sbs_unconditioned_threshold (the search conditions every image's largest G on being 0; see there); under top_k / top_p the
    weights estimate expectations under the truncated model.  n_samples <= 7 with the flag, and the draws differ from those of
    the same seed without it (the slot count enters the row index, hence the noise): they are those of the n_samples + 1 search.
    n_samples must be 1 .. 8.  Adaptive features are not covered, and a model pair is refused (ValueError): the EditNet + DCNet
    ensemble has its own entry, sample_captions_distinct_ensemble."""
    from . import _lib
    *inputs, word_map = inputs_and_word_map
    if isinstance(model, (tuple, list)) or getattr(model, "_adaptive", 0) or getattr(model, "_ABI", None) not in ("editnet", "dcnet"):
        raise ValueError("sample_captions_distinct supports editnet_rl.DecoderC with fixed features and dcnet_rl.DAE; adaptive "
                         "features and the EditNet + DCNet ensemble are not covered")
    if len(inputs) != (3 if model._ABI == "editnet" else 2):
        raise ValueError("sample_captions_distinct(model, [image_features,] previous_caption, prev_caplen, word_map, ...): "
                         "image_features for EditNet, none for DCNet")
    n, k = _sbs_slots(n_samples, return_threshold)
    opts = _lib.sample_opts(temperature, top_k, top_p)
    max_steps = _sbs_max_steps(model, max_steps)
    ms, _, prev, _ = _fused_models(model, inputs, k, max_steps)
    out, steps = _sbs_search(ms, prev.shape[0], k, model.vocab_size, word_map, prev.device, max_steps, opts, _return_steps)
    return _sbs_answer(out, steps, n, return_threshold, _return_steps)


@torch.no_grad()
def sample_captions_distinct_ensemble(decoder, dae, image_features, previous_caption, prev_caplen, word_map, n_samples=5,
                                      temperature=1.0, top_k=0, top_p=1.0, max_steps=None, return_threshold=False,
                                      _return_steps=False):
    """sample_captions_distinct for the EditNet + DCNet ENSEMBLE, the model of the reference's published scores
    (eval_full.py:151-153; beam_search_ensemble*): up to n_samples distinct captions per image, an exact sample without
    replacement from the sequence distribution whose every step is (softmax_e + softmax_d) / 2.  The averaged probabilities are
    a distribution over the words at every step, so the construction applies unchanged (include/set_hip.h
    set_sbs_pick_ensemble_f32).  Both models step on the same words; both states are re-indexed by the pick's rows.
    The temperature tempers EACH model before the average (softmax(x_e / T) and softmax(x_d / T) are averaged, not the average
    tempered).  top_k / top_p truncate the ENSEMBLE's word distribution (the average), not each model before it: the kept set
    is taken on log((softmax_e + softmax_d) / 2) and the average is renormalised over it (set_sbs_pick_ensemble_opts_f32).
    Return convention, max_steps, return_threshold and the seed: sample_captions_distinct; logp is the sequence's
    log-probability under the tempered, truncated ensemble (top_k=1: one entry per image; kappa = -inf when the truncated
    ensemble has no further sequence; the importance weights estimate expectations under it).  max_steps defaults to the
    decoder's max_len.
    ValueError: an adaptive-features decoder (the reference's ensemble uses fixed features), models that are not an
    editnet_rl.DecoderC and a dcnet_rl.DAE, vocabularies of different size, n_samples outside 1 .. 8 (1 .. 7 with
    return_threshold), options sample_captions refuses."""
    from . import _lib
    if getattr(decoder, "_adaptive", 0) or getattr(decoder, "_ABI", None) != "editnet" or getattr(dae, "_ABI", None) != "dcnet":
        raise ValueError("sample_captions_distinct_ensemble takes an editnet_rl.DecoderC with fixed features and a dcnet_rl.DAE; "
                         "adaptive features are not covered")
    if decoder.vocab_size != dae.vocab_size:
        raise ValueError("sample_captions_distinct_ensemble: the models' vocabularies differ (%d and %d words); the ensemble "
                         "averages their word distributions" % (decoder.vocab_size, dae.vocab_size))
    n, k = _sbs_slots(n_samples, return_threshold)
    opts = _lib.sample_opts(temperature, top_k, top_p)
    max_steps = _sbs_max_steps(decoder, max_steps)
    ms, X, _, _ = _fused_models((decoder, dae), (image_features, previous_caption, prev_caplen), k, max_steps)
    out, steps = _sbs_search(ms, X.shape[0], k, decoder.vocab_size, word_map, X.device, max_steps, opts, _return_steps)
    return _sbs_answer(out, steps, n, return_threshold, _return_steps)


# ------------------------------------------------------------------------------------------------
# Diverse (group) beam search (Vijayakumar et al., "Diverse Beam Search"): G alternative captions that differ from each other.
# The beam's k slots are G groups of k / G; every group is a beam search of its own whose picks are penalised, inside the pick
# (set_beam_pick_diverse_f32), for the words the earlier groups picked at the same step.
# ------------------------------------------------------------------------------------------------
def _check_diverse(beam_size, groups, diversity_penalty, max_steps):
    import math
    for name, v in (("beam_size", beam_size), ("groups", groups), ("max_steps", max_steps)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer, got %r" % (name, v))
    k, G, max_steps = int(beam_size), int(groups), int(max_steps)
    if not 1 <= k <= 8:
        raise ValueError("beam_size must lie in 1 .. 8, got %r" % (beam_size,))
    if G < 1 or k % G != 0:
        raise ValueError("groups must divide beam_size = %d, got %r" % (k, groups))
    pen = float(diversity_penalty)
    if not math.isfinite(pen) or pen < 0.0:
        raise ValueError("diversity_penalty must be finite and >= 0, got %r" % (diversity_penalty,))
    if not 1 <= max_steps <= 254:
        raise ValueError("max_steps must lie in 1 .. 254, got %r" % (max_steps,))
    return k, G, pen, max_steps


def _diverse_search(models, NI, k, G, penalty, V, word_map, dev, max_steps, cons, return_all, poll=4):
    """_beam_loop on set_beam_pick_diverse_f32, with the completion list and its groups"""
    from . import _lib
    from ._lib import check, ptr
    lib = _lib.load()
    g = k // G
    s = _BeamState(len(models), NI, k, V, word_map, dev, max_steps, cons, True, True)
    s.scores[:, ::g] = 0.0                                # step 1: only the first slot of every group counts
    g_left = torch.full((NI, G), g, dtype=torch.int32, device=dev)
    done_group = torch.zeros(NI, k, dtype=torch.int32, device=dev)
    step = _beam_loop(models, s, lambda step: check(lib.set_beam_pick_diverse_f32(
        *s.pick_args(step), *s.done_args(), ptr(done_group), ptr(g_left), G, penalty, *s.ws_args()), "set_beam_pick_diverse_f32"), poll)
    start = s.start
    seqs_c, left_c = s.seqs[0].cpu(), g_left.cpu()
    ds_c, dq_c, dl_c, dg_c, nd_c = s.done_score.cpu(), s.done_seq.cpu(), s.done_len.cpu(), done_group.cpu(), s.n_done.cpu()
    out, every = [], []
    for i in range(NI):
        done = [(dq_c[i, j, :int(dl_c[i, j])].tolist(), float(ds_c[i, j]), int(dg_c[i, j])) for j in range(int(nd_c[i]))]
        res = []
        for gi in range(G):
            mine = [e for e in done if e[2] == gi]
            if mine:
                best = max(range(len(mine)), key=lambda q: (mine[q][1], -q))      # first maximum
                res.append((mine[best][0], mine[best][1]))
            elif int(left_c[i, gi]) > 0:                  # ran into the step limit with nothing completed
                res.append((seqs_c[i, gi * g, :step + 1].tolist(), float("nan")))
            else:                                         # ran out of candidates with nothing completed
                res.append(([start], float("nan")))
        out.append(res)
        every.append(sorted(done, key=lambda e: -e[1]))
    return (out, every) if return_all else out


@torch.no_grad()
def beam_search_diverse(model, *inputs_and_word_map, beam_size=6, groups=3, diversity_penalty=0.5, max_steps=50, constraints=None,
                        return_all=False):
    """`groups` alternative captions per image that differ from each other, by diverse (group) beam search (Vijayakumar et al.,
    "Diverse Beam Search"; include/set_hip.h set_beam_pick_diverse_f32):
        out = beam_search_diverse(decoder, image_features, previous_caption, prev_caplen, word_map, beam_size=6, groups=3)
        out = beam_search_diverse(dae, previous_caption, prev_caplen, word_map, beam_size=8, groups=4, diversity_penalty=1.0)
    EditNet (editnet.DecoderC / editnet_rl.DecoderC, fixed features) takes image_features (NI,R,F), previous_caption (NI,T),
    prev_caplen (NI,1); DCNet (DAE) the caption pair only.  The beam's beam_size slots (1 .. 8) are `groups` groups of
    beam_size / groups slots; every group is this project's beam search over its own slots, and at every step the groups pick one
    after the other, each by log-probability sum minus diversity_penalty x (how many picks of the earlier groups at this step took
    the word).  <end> is never penalised.  The penalty only steers the picks: the returned scores are sums of the model's
    log-probabilities (rank scores under constraints.length_penalty), comparable between groups and with every beam_search_*.
    diversity_penalty = 0: every group runs the same search of beam_size / groups slots; groups = 1: the constrained search.
    constraints: an evaluate.BeamConstraints (n-gram blocking, banned words, minimum length, length penalty) applied to every
    group, or None.
    Returns, per image, a list of `groups` (tokens, score) pairs in group order: the group's best completed hypothesis (tokens
    with <start> and <end>, first maximum of the score); (its first slot's tokens so far, nan) for a group that hit the step
    limit with nothing completed; ([<start>], nan) for one that ran out of candidates with nothing completed.
    return_all=True: returns (that, every) with every[i] all completed hypotheses of image i as (tokens, score, group), score
    descending, equal scores in completion order.
    ValueError before any device work: beam_size outside 1 .. 8, groups not dividing it, a penalty that is negative or not
    finite, a bad banned word, an adaptive-features model or a model pair (the ensemble: beam_search_diverse_ensemble)."""
    *inputs, word_map = inputs_and_word_map
    k, G, pen, max_steps = _check_diverse(beam_size, groups, diversity_penalty, max_steps)
    if isinstance(model, (tuple, list)) or getattr(model, "_adaptive", 0) or getattr(model, "_ABI", None) not in ("editnet", "dcnet"):
        raise ValueError("beam_search_diverse supports EditNet's DecoderC with fixed features and DCNet's DAE; adaptive features "
                         "are not covered and the EditNet + DCNet ensemble has its own entry")
    if len(inputs) != (3 if model._ABI == "editnet" else 2):
        raise ValueError("beam_search_diverse(model, [image_features,] previous_caption, prev_caplen, word_map, ...): "
                         "image_features for EditNet, none for DCNet")
    cons = _check_constraints(constraints, word_map, model)
    ms, _, prev, _ = _fused_models(model, inputs, k, max_steps)
    return _diverse_search(ms, prev.shape[0], k, G, pen, model.vocab_size, word_map, prev.device, max_steps, cons, return_all)


@torch.no_grad()
def beam_search_diverse_ensemble(decoder, dae, image_features, previous_caption, prev_caplen, word_map, beam_size=6, groups=3,
                                 diversity_penalty=0.5, max_steps=50, constraints=None, return_all=False):
    """beam_search_diverse for the EditNet + DCNet ENSEMBLE (beam_search_ensemble*): both models step on the same words, a
    candidate's value is the running sum plus log((softmax_e + softmax_d) / 2), both states are re-indexed by the pick's rows.
    Keywords, result and errors: beam_search_diverse; also ValueError for an adaptive-features decoder, models that are not an
    EditNet DecoderC and a DCNet DAE, and vocabularies of different size."""
    k, G, pen, max_steps = _check_diverse(beam_size, groups, diversity_penalty, max_steps)
    if getattr(decoder, "_adaptive", 0) or getattr(decoder, "_ABI", None) != "editnet" or getattr(dae, "_ABI", None) != "dcnet":
        raise ValueError("beam_search_diverse_ensemble takes an EditNet DecoderC with fixed features and a DCNet DAE; adaptive "
                         "features are not covered")
    if decoder.vocab_size != dae.vocab_size:
        raise ValueError("beam_search_diverse_ensemble: the models' vocabularies differ (%d and %d words); the ensemble averages "
                         "their word distributions" % (decoder.vocab_size, dae.vocab_size))
    cons = _check_constraints(constraints, word_map, decoder)
    ms, X, _, _ = _fused_models((decoder, dae), (image_features, previous_caption, prev_caplen), k, max_steps)
    return _diverse_search(ms, X.shape[0], k, G, pen, decoder.vocab_size, word_map, X.device, max_steps, cons, return_all)


def sbs_unconditioned_threshold(kappa, e=None):
    """The threshold of return_threshold with the conditioning on "the largest perturbed score of the image is 0" taken out:
        kappa' = -log(exp(-kappa) + E - 1) = -log(expm1(-kappa) + E),   E ~ Exp(1), one draw per image
    In u = exp(-G) the top-down construction only ever ADDS to the root's u (a child's conditioned u is its parent's plus a
    difference of its siblings'), so a root at G = Z instead of 0 moves every u of the image by exp(-Z) - 1, and exp(-Z) of a
    standard Gumbel Z is a standard exponential.  The map is increasing: order and sample are unchanged; the same map takes an
    entry's G to its unconditioned value.  kappa = -inf stays -inf.
    kappa: a float or a list of floats (one per image).  e: the exponential draws (a float or a list; tests), default: drawn
    from torch's CPU generator, so torch.manual_seed() reproduces them.  Float64 on the host."""
    import numpy as np
    one = np.ndim(kappa) == 0
    k = np.atleast_1d(np.asarray(kappa, np.float64))
    if e is None:
        e = torch.empty(len(k), dtype=torch.float64).exponential_().numpy()
    e = np.broadcast_to(np.asarray(e, np.float64), k.shape)
    with np.errstate(over="ignore", divide="ignore"):
        out = -np.log(np.expm1(-k) + e)
    return float(out[0]) if one else out.tolist()


def sbs_importance_weights(entries, kappa, normalize=True):
    """Importance weights of ONE image's stochastic-beam-search sample (Kool, van Hoof, Welling, ICML 2019, section 4.2):
        out, kappa = sample_captions_distinct(model, ..., n_samples=5, return_threshold=True)
        kappa = sbs_unconditioned_threshold(kappa)
        w = sbs_importance_weights(out[i], kappa[i], normalize=False)
        estimate = sum(w_j * f(entry_j) for w_j, entry_j in zip(w, out[i]))       # unbiased for E[f(caption)]
    entries: the image's (tokens, logp, G, finished) list; kappa: its threshold.  In float64 on the host:
        q_j = P(G_j > kappa) = 1 - exp(-exp(logp_j - kappa)) = -expm1(-exp(logp_j - kappa))
        w_j = exp(logp_j) / q_j
    kappa = -inf (the sample is the model's whole support) gives q_j = 1 and w_j = p_j.  normalize=True divides the weights by
    their sum (the self-normalised estimator: biased, lower variance); normalize=False gives the unbiased estimator.
    UNBIASED ONLY WITH AN UNCONDITIONED THRESHOLD.  The search starts every image's root at G = 0, i.e. it draws the perturbed
    scores conditioned on their maximum being 0.  That leaves the sample and its order exact, but the raw kappa of
    return_threshold is the threshold of the conditioned scores, and q_j above is the inclusion probability under independent
    Gumbel scores: with the raw kappa the estimate is biased (table model of tests/sbs_fixtures.py, 2 of 40 sequences: the
    estimate of E[1] is 0.84).  Pass kappa through sbs_unconditioned_threshold first.
    Exact only for FINISHED sequences: an entry cut at max_steps stands for every continuation of its prefix, and its logp is
    the prefix's.  Returns a float64 numpy array, one weight per entry."""
    import numpy as np
    phi = np.array([e[1] for e in entries], np.float64)
    with np.errstate(over="ignore"):
        q = -np.expm1(-np.exp(phi - np.float64(kappa)))
    w = np.exp(phi) / q
    return w / w.sum() if normalize and len(w) else w


def tokens_from_greedy(seq, word_map):
    """(B, max_len) greedy / sampled output -> forced token lists: `<start>` in front and, for rows that ended before
    max_len, `<end>` behind (the decode loops store `<end>` as 0, editnet_rl.py:531)."""
    start, end = int(word_map['<start>']), int(word_map['<end>'])
    rows = seq.cpu().tolist() if torch.is_tensor(seq) else [list(map(int, r)) for r in seq]
    out = []
    for r in rows:
        n = r.index(0) if 0 in r else len(r)
        out.append([start] + [int(x) for x in r[:n]] + ([end] if n < len(r) else []))
    return out


def _forced_tokens(tokens, lengths, dev):
    """token lists | (B, L) tensor + lengths -> (tokens (B, S + 1) int64 zero-padded, n_steps (B) int32, S) with
    n_steps[b] = len(tokens[b]) - 1 and S = the largest of them (at least 1)"""
    if torch.is_tensor(tokens):
        if lengths is None:
            raise ValueError("edit_trace: a token tensor needs `lengths` (tokens per row, <start> included)")
        lens = torch.as_tensor(lengths).reshape(-1).cpu().long()
        if lens.numel() != tokens.shape[0] or int(lens.min()) < 1 or int(lens.max()) > tokens.shape[1]:
            raise ValueError("edit_trace: lengths must be B values in [1, %d]" % tokens.shape[1])
        S = max(1, int(lens.max()) - 1)
        tok = torch.zeros(tokens.shape[0], S + 1, dtype=torch.long)
        src = tokens.cpu().long()
        keep = torch.arange(S + 1)[None, :] < lens[:, None]
        w = min(S + 1, src.shape[1])
        tok[:, :w] = src[:, :w] * keep[:, :w]
    else:
        rows = [[int(x) for x in r] for r in tokens]
        if not rows or min(len(r) for r in rows) < 1:
            raise ValueError("edit_trace: every token list starts with <start>")
        lens = torch.tensor([len(r) for r in rows], dtype=torch.long)
        S = max(1, int(lens.max()) - 1)
        tok = torch.zeros(len(rows), S + 1, dtype=torch.long)
        for b, r in enumerate(rows):
            tok[b, :len(r)] = torch.tensor(r, dtype=torch.long)
    return tok.to(dev), (lens - 1).to(torch.int32).to(dev), S


@torch.no_grad()
def edit_trace(decoder, image_features, previous_caption, prev_caplen, word_map, tokens, image_mean=None, lengths=None):
    """Forced, no-grad decode of `tokens` that records every step -> EditTrace.  tokens: a list of B token lists as the beam
    searches return them (`<start>` ... `<end>`, or cut at the step limit; see tokens_from_greedy for greedy output), or a
    (B, L) tensor with `lengths` (B) tokens per row.  image_mean (B, F) selects the adaptive model's image input exactly as
    beam_search_adaptive* takes it (None: the mean over all R regions)."""
    import ctypes as C
    from . import _lib
    from ._lib import check, ptr, stream_of
    decoder.eval()
    lib = _lib.load()
    X = image_features.float().contiguous()
    dev = X.device
    prev = previous_caption.long().contiguous()
    plen = prev_caplen.reshape(-1).long().contiguous()
    if getattr(decoder, "_adaptive", 0):
        X, mean = _adaptive_args(decoder, X, image_mean)
    else:
        mean = None if image_mean is None else image_mean.to(dev).float().contiguous()
    tok, n_steps, S = _forced_tokens(tokens, lengths, dev)
    B, R = X.shape[0], X.shape[1]
    if tok.shape[0] != B or prev.shape[0] != B or plen.shape[0] != B:
        raise ValueError("edit_trace: %d token rows for %d images / %d previous captions" % (tok.shape[0], B, prev.shape[0]))
    if int(tok.min()) < 0 or int(tok.max()) >= decoder.vocab_size:
        raise ValueError("edit_trace: token outside the vocabulary")
    T, D = prev.shape[1], decoder.decoder_dim
    dims = decoder._dims(B, T, R, S)
    w = decoder._weights(dims)
    ws = decoder._workspace(dims)
    n = lib.set_editnet_edit_trace_workspace_bytes(C.byref(dims), S)
    if n == 0:
        raise _lib.SetError("edit_trace: unsupported dims")
    tws = torch.empty(n, dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    tr = EditTrace(torch.empty(B, S, T, **f32), torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, S, **f32),
                   torch.empty(B, S, D, **f32), torch.empty(B, S, R, **f32), torch.empty(B, S, **f32), n_steps, tok, prev)
    out = _lib.EditTrace(alpha_c=tr.alpha_c.data_ptr(), select=tr.select.data_ptr(), copy_gate=tr.copy_gate.data_ptr(),
                         gate_full=tr.gate_full.data_ptr(), alpha_v=tr.alpha_v.data_ptr(), logp=tr.logp.data_ptr())
    check(lib.set_editnet_edit_trace(C.byref(w), C.byref(dims), ptr(X), None if mean is None else ptr(mean), ptr(prev), ptr(plen),
                                     ptr(tok), tok.shape[1], ptr(n_steps), S, C.byref(out), ptr(ws), ws.numel(), ptr(tws),
                                     tws.numel(), stream_of(dev)), "set_editnet_edit_trace")
    return tr


# ---- consensus (minimum-Bayes-risk) reranking under CIDEr-D -------------------------------------------------------------
def consensus_rerank(scorer, candidates, n_per_image, weights=None):
    """Choose among the candidate captions of an image the one most similar to all the others:
        dsc = ciderd_scorer.device(dev)                                      # ciderd.DeviceCiderD
        seq, _ = sample_captions(decoder, X, prev, plen, word_map, n_samples=5)
        best, utility = consensus_rerank(dsc, seq.reshape(-1, seq.shape[-1]), 5)
    candidates: (NI * n, L) id tensor in the decoder's format (0 = <end>, rows i * n .. i * n + n - 1 belong to image i);
    `scorer.pair_scores(candidates, n)` gives the (NI * n, n) CIDEr-D of every candidate against each candidate of its image
    as the only reference (csrc/ciderd_device.hip: the candidates are each other's references and never leave the device).
    Any object with that method serves: bleu.DeviceBleu(dev) reranks under sentence BLEU-4 instead (csrc/bleu_device.hip),
    rouge.DeviceRougeL(dev) under ROUGE-L (csrc/rouge_device.hip),
    editdist.DeviceEditDistance(dev) under the word edit similarity (m - d) / m (csrc/editdist_device.hip).
    utility[i, j] = mean over the OTHER candidates r != j of that score (the diagonal is left out; identical candidates are
    separate votes), or with weights (NI, n) — e.g. sbs_importance_weights per image — the weighted mean
    sum_{r != j} w[i, r] s[j, r] / sum_{r != j} w[i, r] (0 where that sum is 0).  n = 1: utility 0, index 0.
    Returns (best_index (NI,) int64: the largest utility, ties to the lowest index; utility (NI, n) float64), on the
    device of the scores."""
    n = int(n_per_image)
    if n < 1:
        raise ValueError("n_per_image must be >= 1, got %r" % (n_per_image,))
    N = int(candidates.shape[0])
    if N % n:
        raise ValueError("%d candidates are not %d per image" % (N, n))
    NI = N // n
    P = scorer.pair_scores(candidates, n)
    if tuple(P.shape) != (N, n):
        raise ValueError("pair_scores returned shape %s, expected %s" % (tuple(P.shape), (N, n)))
    P = P.double().view(NI, n, n)
    dev = P.device
    w = torch.ones(NI, n, dtype=torch.float64, device=dev) if weights is None else \
        torch.as_tensor(weights, dtype=torch.float64).to(dev).reshape(NI, n)
    off = 1.0 - torch.eye(n, dtype=torch.float64, device=dev)
    wm = w[:, None, :] * off[None]                              # [i, j, r]: weight of vote r for candidate j
    den = wm.sum(-1)
    num = (torch.where(wm != 0, P, torch.zeros_like(P)) * wm).sum(-1)
    utility = torch.where(den != 0, num / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(den))
    idx = torch.arange(n, device=dev).expand(NI, n)
    best = torch.where(utility == utility.max(1, keepdim=True).values, idx, torch.full_like(idx, n)).min(1).values
    return best, utility


def consensus_rerank_lists(scorer, captions, weights=None, word_map=None):
    """consensus_rerank for what sample_captions_distinct[_ensemble], n_best= and beam_search_diverse(return_all=True) return:
    captions[i] = the id lists of image i (or entries whose first field is the id list), any number per image.  Lists are in
    the rollouts' convention (<end> stored as 0); with word_map, <start> / <pad> are dropped and <end> becomes 0 first, as
    ciderd.ground_truth_lists does.  weights[i]: one weight per candidate of image i, or None.
    Lists are zero-padded to the longest: one that holds no 0 and is shorter than that is read as ended where it stops.
    Returns (best (NI) list of indices, utility (NI) list of float lists); images with the same count share one launch."""
    drop, end = set(), None
    if word_map is not None:
        drop, end = {int(word_map['<start>']), int(word_map['<pad>'])}, int(word_map['<end>'])
    rows = [[[0 if w == end else int(w) for w in (c[0] if isinstance(c, tuple) else c) if int(w) not in drop] for c in caps]
            for caps in captions]
    L = max([1] + [len(c) for caps in rows for c in caps])
    best, util = [0] * len(rows), [[] for _ in rows]
    for n in sorted({len(caps) for caps in rows} - {0}):
        ids = [i for i, caps in enumerate(rows) if len(caps) == n]
        t = torch.zeros(len(ids) * n, L, dtype=torch.int64)
        for a, i in enumerate(ids):
            for j, c in enumerate(rows[i]):
                t[a * n + j, :len(c)] = torch.tensor(c, dtype=torch.int64)
        w = None if weights is None else [list(weights[i]) for i in ids]
        b, u = consensus_rerank(scorer, t, n, w)
        for a, i in enumerate(ids):
            best[i], util[i] = int(b[a]), u[a].tolist()
    return best, util


# ---- validation BLEU, ROUGE-L and CIDEr (the `Bleu_1..4` / `ROUGE_L` / `CIDEr` of the reference's evaluate(): editnet_rl.py:834/897, dcnet.py:541-611)
def _validation_rows(captions, hyp_set, dev, count_end, word_map):
    """The caption-normalising front of the validation scores: captions in either input form (see validation_bleu) ->
    ((N, L) id tensor on `dev`, (N,) set index on `dev`, lengths or None for the 0 rule)."""
    lens = None
    if word_map is not None:
        drop, end = {int(word_map['<start>']), int(word_map['<pad>'])}, int(word_map['<end>'])
        rows = [[0 if int(w) == end else int(w) for w in c if int(w) not in drop] for c in captions]
        rows = [c[:c.index(0) + (1 if count_end else 0)] if 0 in c else c for c in rows]
        captions = torch.zeros(len(rows), max([1] + [len(c) for c in rows]), dtype=torch.int64)
        for i, c in enumerate(rows):
            captions[i, :len(c)] = torch.tensor(c, dtype=torch.int64)
        # a list that never reached <end> (the step limit) ends where it stops: explicit lengths, not the 0 rule
        lens = torch.tensor([len(c) for c in rows], dtype=torch.int32)
    captions = torch.as_tensor(captions).to(dev)
    if captions.dim() != 2:
        raise ValueError("captions are rows of a 2-D id tensor, got shape %s" % (tuple(captions.shape),))
    N, L = captions.shape
    if hyp_set is None:
        hyp_set = torch.arange(N, dtype=torch.int32, device=dev)
    if lens is None and not count_end and L > 0:
        is0 = captions == 0
        lens = torch.where(is0.any(1), is0.int().argmax(1), torch.full((N,), L, dtype=torch.int64, device=dev))
    return captions, hyp_set, lens


def _validation_corpus(scorer, captions, hyp_set, ground_truth, count_end, word_map):
    """corpus_score of a record-based device scorer over captions in either input form, the references prepared here"""
    captions, hyp_set, lens = _validation_rows(captions, hyp_set, scorer.dev, count_end, word_map)
    return scorer.corpus_score(captions, hyp_set, scorer.prepare_refs(ground_truth, count_end=count_end), lens)


def validation_bleu(captions, hyp_set, ground_truth, dev, count_end=False, word_map=None):
    """Corpus Bleu_1..4 of decoded captions without strings:
        gt = ciderd.ground_truth_lists(allcaps, word_map)
        seq, _ = decoder(word_map, prev, plen, X, sample_max=True, sample_rl=False)     # greedy: (N, L) ids, stays on the device
        bleu = validation_bleu(seq, None, gt, X.device)                                 # bleu[3]: Bleu_4
        seqs = beam_search_editnet_batched(decoder, X, prev, plen, word_map)            # any search: lists of token lists
        bleu = validation_bleu(seqs, None, gt, X.device, word_map=word_map)
    captions: (N, L) ids in the decoder's format (0 = <end> and everything after it), L <= 64 — or, with word_map, what the
    beam searches return: N token lists in the vocabulary's ids, from which <start> / <pad> are dropped and whose <end>
    becomes 0 (ciderd.ground_truth_lists' rule), zero-padded into one upload.  hyp_set: (N,) index of each caption's reference
    set (None: caption i belongs to set i); ground_truth: the reference sets as id lists with <end> = 0.
    count_end=False (cocoEval's word strings): a caption ends BEFORE its first 0 and the references lose theirs; True: the
    SCST convention, the 0 is a token on both sides.  The statistics are summed and scored on the device (bleu.DeviceBleu,
    csrc/bleu_device.hip) and nothing is read back.  Returns a (4,) float64 device tensor."""
    from . import bleu
    return _validation_corpus(bleu.device_scorer(dev), captions, hyp_set, ground_truth, count_end, word_map)


def validation_rouge_l(captions, hyp_set, ground_truth, dev, count_end=False, word_map=None):
    """Corpus ROUGE_L of decoded captions without strings: the mean of the captions' ROUGE-L (rouge.py; beta = 1.2) on the
    device (rouge.DeviceRougeL, csrc/rouge_device.hip), nothing read back.  Input forms and conventions are validation_bleu's.
    Returns a 0-d float64 device tensor."""
    from . import rouge
    return _validation_corpus(rouge.device_scorer(dev), captions, hyp_set, ground_truth, count_end, word_map)


def validation_cider(captions, hyp_set, ground_truth, dev, count_end=False, word_map=None):
    """Corpus CIDEr of decoded captions without strings: cocoEval's `CIDEr`, the value the reference's evaluate() returns first
    and selects checkpoints by (`eval/eval rl/eval_full.py:235`).  It is the SCST reward's sentence formula (ciderd.py) with
    another table: the document frequencies and the number of documents N come from the reference sets of `ground_truth`
    itself — ALL of them, whichever sets hyp_set names; a gram counts once per image (ciderd.corpus_cider is the host
    statement).  The table is built on the device from the uploaded reference ids (ciderd.DeviceCiderD.from_refs,
    csrc/ciderd_device.hip cd_build_k); the value is the mean of the captions' scores, taken there.  Input forms and conventions
    are validation_bleu's.  Returns a 0-d float64 device tensor; nothing is read back."""
    from . import ciderd
    scorer, refs = ciderd.DeviceCiderD.from_refs(dev, ground_truth, count_end=count_end)
    captions, hyp_set, lens = _validation_rows(captions, hyp_set, scorer.dev, count_end, word_map)
    return scorer.corpus_score(captions, hyp_set, refs, lens)


def validation_scores(captions, hyp_set, ground_truth, dev, count_end=False, word_map=None, cider=False):
    """validation_bleu and validation_rouge_l in one: the references are uploaded once and prepared by one launch, whose
    records both score kernels read.  Returns {'Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L'} (the reference's key names)
    -> 0-d float64 device tensors, the very bits of the two single calls; nothing is read back.
    cider=True: the reference's whole overlap row — the key 'CIDEr' comes last, with the bits of validation_cider; its table
    and reference vectors are built from the same upload."""
    from . import bleu, rouge
    bscorer, rscorer = bleu.device_scorer(dev), rouge.device_scorer(dev)
    captions, hyp_set, lens = _validation_rows(captions, hyp_set, bscorer.dev, count_end, word_map)
    refs = bscorer.prepare_refs(ground_truth, count_end=count_end)
    b = bscorer.corpus_score(captions, hyp_set, refs, lens)
    out = {"Bleu_%d" % (k + 1): b[k] for k in range(4)}
    out["ROUGE_L"] = rscorer.corpus_score(captions, hyp_set, refs, lens)
    if cider:
        from . import ciderd
        cscorer, crefs = ciderd.DeviceCiderD.from_refs(bscorer.dev, refs)
        out["CIDEr"] = cscorer.corpus_score(captions, hyp_set, crefs, lens)
    return out


# ---- word edit distance: how far from the references, how much the model edited, which word became which (editdist.py) ----------
def validation_edit(captions, hyp_set, ground_truth, dev, count_end=False, word_map=None):
    """Word edit distance of decoded captions to their closest references without strings (editdist.py): {'similarity': the mean
    of the captions' (m - d) / m against the reference of largest similarity, 'wer': sum d / sum len of those references} on the
    device (editdist.DeviceEditDistance, csrc/editdist_device.hip), nothing read back.  Input forms and conventions are
    validation_bleu's.  Returns 0-d float64 device tensors."""
    from . import editdist
    return _validation_corpus(editdist.device_scorer(dev), captions, hyp_set, ground_truth, count_end, word_map)


def source_rows(previous_caption, prev_caplen, word_map, count_end=False):
    """The model's input captions in the outputs' convention, on the device they are on: previous_caption (B, Lp) in the
    vocabulary's ids with <start> / <end> / <pad>, prev_caplen (B[, 1]) ids per row (None: the whole row) -> ((B, Lp) int64
    with <start> / <pad> dropped, the rest moved to the front and <end> rewritten to 0 — ciderd.ground_truth_lists' rule —,
    (B,) int32 lengths: up to and, with count_end, including the first 0; no 0: every kept id)."""
    prev = torch.as_tensor(previous_caption).long()
    if prev.dim() != 2:
        raise ValueError("previous captions are rows of a 2-D id tensor, got shape %s" % (tuple(prev.shape),))
    B, Lp = prev.shape
    pos = torch.arange(Lp, device=prev.device)[None, :]
    keep = (prev != int(word_map['<start>'])) & (prev != int(word_map['<pad>']))
    if prev_caplen is not None:
        keep &= pos < torch.as_tensor(prev_caplen).to(prev.device).reshape(B, 1)
    ids = torch.where(prev == int(word_map['<end>']), torch.zeros_like(prev), prev)
    dest = torch.where(keep, keep.long().cumsum(1) - 1, torch.full_like(prev, Lp))          # dropped ids land in a spare column
    rows = torch.zeros(B, Lp + 1, dtype=torch.int64, device=prev.device).scatter_(1, dest, ids)[:, :Lp]
    kept = keep.long().sum(1)
    is0 = (rows == 0) & (pos < kept[:, None])
    lens = torch.where(is0.any(1), is0.int().argmax(1) + (1 if count_end else 0), kept)
    return rows, lens.int()


def _edit_rows(previous_caption, prev_caplen, captions, word_map, dev, count_end):
    """both sides of edit_statistics / edit_alignment on the scorer's device: (scorer, hyp rows, hyp lengths or None, source
    rows, source lengths)"""
    from . import editdist
    scorer = editdist.device_scorer(dev)
    lists = not hasattr(captions, "shape")                         # a tensor or an array: decoder ids; else token lists
    hyp, _, hyp_lens = _validation_rows(captions, None, scorer.dev, count_end, word_map if lists else None)
    src, src_lens = source_rows(torch.as_tensor(previous_caption).to(scorer.dev), prev_caplen, word_map, count_end)
    if src.shape[0] != hyp.shape[0]:
        raise ValueError("%d captions for %d previous captions" % (hyp.shape[0], src.shape[0]))
    return scorer, hyp, hyp_lens, src, src_lens


def edit_statistics(previous_caption, prev_caplen, captions, word_map, dev, count_end=False):
    """How much the model edited: the word edit script from each input caption to its output (editdist.alignment), counted.
        seq, _ = decoder(word_map, prev, plen, X, sample_max=True, sample_rl=False)     # greedy: (B, L) ids, stays on the device
        st = edit_statistics(prev, plen, seq, word_map, X.device)                        # st['unchanged_frac'], st['edit_rate']
    previous_caption (B, Lp) / prev_caplen: the model's input, brought to the outputs' convention on the device (source_rows);
    captions: (B, L) decoder ids (0 = <end> and everything after it) or, as validation_bleu accepts with word_map, B token
    lists in the vocabulary's ids.  count_end as in validation_bleu, on both sides.  Returns device tensors, nothing read back:
    per caption int32 (B,) 'dist', 'keep', 'sub', 'ins', 'del', 'unchanged'; 0-d float64 'unchanged_frac', 'mean_dist' and
    'edit_rate' = sum dist / sum source length (0 when that sum is 0)."""
    scorer, hyp, hyp_lens, src, src_lens = _edit_rows(previous_caption, prev_caplen, captions, word_map, dev, count_end)
    st = scorer.align_token_ids(hyp, src, hyp_lens, src_lens)[0]
    out = {k: st[:, c] for k, c in (("dist", 0), ("keep", 3), ("sub", 4), ("ins", 5), ("del", 6), ("unchanged", 7))}
    zero = torch.zeros((), dtype=torch.float64, device=st.device)
    words = st[:, 2].sum().double()
    some = st.shape[0] > 0
    out["unchanged_frac"] = st[:, 7].double().mean() if some else zero
    out["mean_dist"] = st[:, 0].double().mean() if some else zero
    out["edit_rate"] = torch.where(words > 0, st[:, 0].sum().double() / torch.where(words > 0, words, torch.ones_like(words)), zero)
    return out


class EditAlignment:
    """The word alignment of each input caption with its output (editdist.DeviceEditDistance.align_token_ids), device tensors:
    stats int32 (B, 8) = dist, len_h, len_s, keep, sub, ins, del, unchanged; hyp_ops int8 (B, L) 1 keep / 2 substitute /
    3 insert; hyp_src int32 (B, L) the aligned source position or -1; src_ops int8 (B, Ls) 1 kept / 2 substituted / 3 deleted;
    0 / -1 at and beyond the lengths.  hyp (B, L) and src (B, Ls) are the id rows that were aligned (<end> = 0).  This is the
    edit that happened between the two word sequences; EditTrace records the model's own soft view of it."""

    def __init__(self, stats, hyp_ops, hyp_src, src_ops, hyp, src):
        self.stats, self.hyp_ops, self.hyp_src, self.src_ops, self.hyp, self.src = stats, hyp_ops, hyp_src, src_ops, hyp, src

    def rows(self, word_map):
        """per caption: ([(output word, 'keep' / 'substitute' / 'insert', source word or None)], [deleted source words])"""
        from .editdist import DEL, OP_NAMES
        rev = {int(v): k for k, v in word_map.items()}
        rev[0] = '<end>'
        hyp, src = self.hyp.cpu().tolist(), self.src.cpu().tolist()
        ho, hs, so = self.hyp_ops.cpu().tolist(), self.hyp_src.cpu().tolist(), self.src_ops.cpu().tolist()
        out = []
        for b, st in enumerate(self.stats.cpu().tolist()):
            words = [(rev[hyp[b][j]], OP_NAMES[ho[b][j]], rev[src[b][hs[b][j]]] if hs[b][j] >= 0 else None)
                     for j in range(max(st[1], 0))]
            out.append((words, [rev[src[b][k]] for k in range(max(st[2], 0)) if so[b][k] == DEL]))
        return out


def edit_alignment(previous_caption, prev_caplen, captions, word_map, dev, count_end=False):
    """Which input word each output word corresponds to -> EditAlignment.  Arguments as edit_statistics; nothing is read back
    until `rows(word_map)` is asked for."""
    scorer, hyp, hyp_lens, src, src_lens = _edit_rows(previous_caption, prev_caplen, captions, word_map, dev, count_end)
    return EditAlignment(*scorer.align_token_ids(hyp, src, hyp_lens, src_lens), hyp, src)
