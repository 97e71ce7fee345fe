"""Restatements of the constrained greedy and sampled picks (include/set_hip.h "Constrained greedy and sampled picks") and the
fixtures of their tests.
  * removed(): rules a-c as a naive walk over a row's token list;
  * masked(): the row with its removed words at -inf (a row that has finished is left alone), after which the pick is the
    existing restatement of that mode: pick_oracle.greedy_step / trunc_sample_oracle.truncated_draw, imported and not edited.
tests/test_pick_constrained_cpu.py pins removed() to a brute-force enumeration of n-grams and asserts, on the oracle alone, that
the fixtures below keep every sampled draw and every top-p target clear of a boundary and every greedy arg-max 1e-4 clear of the
runner-up among the survivors — so tests/test_hip_pick_constrained.py compares every row."""
import numpy as np

import pick_oracle as PO
import trunc_sample_oracle as TS

GREEDY_GAP_MIN = 1e-4


class Cons:
    """the fields of SetBeamConstraints a pick reads (length_alpha is 0)"""
    def __init__(self, ngram=0, min_len=0, banned=()):
        self.ngram, self.min_len, self.banned = int(ngram), int(min_len), tuple(int(w) for w in banned)

    def neutral(self):
        return self.ngram == 0 and self.min_len == 0 and not self.banned


def removed(s, V, end, cons):
    """s = [<start>, w_1 .. w_t] (L = t + 1 tokens): the set of words removed from the row at timestep t = L - 1"""
    L, n, t = len(s), cons.ngram, len(s) - 1
    out = set(w for w in cons.banned if 0 <= w < V)                            # a
    if t < cons.min_len and 0 <= end < V:                                      # b
        out.add(int(end))
    if n >= 1 and L >= n:                                                      # c
        last = list(s[L - n + 1:L])
        for i in range(1, L - n + 1):
            if list(s[i:i + n - 1]) == last and 0 <= s[i + n - 1] < V:
                out.add(int(s[i + n - 1]))
    return out


def masked(x, hist, unf, t, end, cons, start=-1):
    """x (B, V) -> a copy with the removed words of every LIVE row (t == 0 or unf[b] != 0) at -inf; hist (B, >= t) = seq"""
    x = np.array(x, copy=True)
    V = x.shape[1]
    for b in range(x.shape[0]):
        if t > 0 and not unf[b]:
            continue
        for w in removed([start] + [int(v) for v in hist[b, :t]], V, end, cons):
            x[b, w] = -np.inf
    return x


def greedy_step(x64, t, max_len, end, st, cons, row_limit=None):
    """one constrained greedy launch on float64 logits: st as pick_oracle.new_state, updated in place"""
    return PO.greedy_step(masked(x64, st["seq"], st["unf"], t, end, cons), t, max_len, end, st, row_limit)


def sample_step(x32, opts, seed, offset, t, reg, max_len, end, st, cons):
    """one constrained sampled launch on the kernel's float32 logits x32 (B, V): the draw of trunc_sample_oracle on the masked
    rows, then the bookkeeping.  Returns (Draw, step log-prob (B,), broken).  reg: the row layout.  A MASKED row (live, constraints
    not neutral) is enumerated as the register path enumerates it on either layout — the draw does not depend on the layout; a row
    that is not masked keeps the layout's enumeration, as in the unconstrained pick."""
    m32 = masked(np.asarray(x32, np.float32), st["seq"], st["unf"], t, end, cons)
    d = TS.truncated_draw(m32, opts, seed, offset, t=t, reg=reg)
    if not reg and not cons.neutral():
        q = TS.truncated_draw(m32, opts, seed, offset, t=t, reg=True)
        is_masked = (np.asarray(st["unf"]) != 0) | (t == 0)
        d.ids, d.margin, d.alt = (np.where(is_masked, a, b) for a, b in ((q.ids, d.ids), (q.margin, d.margin), (q.alt, d.alt)))
    logp = d.logp[np.arange(len(d.ids)), d.ids]
    broken = PO.book_step(d.ids, logp, t, max_len, end, st)
    return d, logp, broken


# ------------------------------------------------------------------------------------------- fixtures of the pick-level tests
FILLER = 7
SAMPLE_OPTS = [TS.NEUTRAL, (1.0, 50, 1.0), (1.0, 0, 0.9), (0.8, 50, 0.9)]


class Case:
    """name, V, ld, n slabs, B rows, timestep t of max_len, end, Cons; slabs (n, B, V) + bias as trunc_sample_oracle.grid_case
    makes them; hist (B, max_len) = seq before the step, unf (B,)"""


def _history(t, max_len, n, w, rng, V):
    """t tokens after which rule c (n >= 1, t >= n) removes w: [FILLER^(n-1), w, FILLER ...] when the suffix clears w, w^t
    otherwise; t < n: w^t (nothing can fire).  Padded with random other words where the pattern leaves room."""
    h = np.zeros(max_len, np.int64)
    if n > 1 and t >= 2 * n - 1:
        h[:t] = FILLER
        h[n - 1] = w
    else:
        h[:t] = w
    return h


def make_case(name, V, ld, n, B, t, max_len, ngram, min_len, n_banned=3, seed=None, finished_row=None):
    c = Case()
    c.name, c.V, c.ld, c.n, c.B, c.t, c.max_len = name, V, ld, n, B, t, max_len
    slabs, bias, x32 = TS.grid_case(V, n, seed)
    c.slabs, c.bias, c.x32 = slabs[:, :B].copy(), bias, x32[:B].copy()
    rng = np.random.default_rng([V, n, t, B, 99])
    top = np.argsort(-c.x32.astype(np.float64), axis=1)
    c.end = int(top[min(1, B - 1), 0]) if min_len > t else V - 1          # rule b on: <end> is row 1's best word
    # banned: row 0's second-best word, an id beyond V, then words of the tail; never <end>
    banned = [int(top[0, 1]), V + 5]
    pool = [int(w) for w in rng.permutation(V) if int(w) != c.end and int(w) != int(top[0, 1])]
    banned += pool[:max(n_banned - 2, 0)]
    c.cons = Cons(ngram, min_len, banned[:n_banned])
    c.hist = np.zeros((B, max_len), np.int64)
    c.unf = np.ones(B, np.int32)
    for b in range(B):
        if name == "full_lists":                                           # t distinct words: n = 1 removes every one of them
            words = [w for w in pool[n_banned:] if w != 0][:t - 1]
            c.hist[b, :t] = [int(top[b, 0])] + words
        else:
            c.hist[b] = _history(t, max_len, ngram, int(top[b, 0]), rng, V)
    if finished_row is not None and t > 0 and finished_row < B:           # a row that ended one step ago: read unmasked
        c.unf[finished_row] = 0
        c.hist[finished_row, t - 1] = 0
    return c


def pick_cases():
    """the smallest shapes at which the constrained picks can go wrong (ISSUE: layouts, list sizes, the steps at which rule c
    first can and cannot fire, both min_len edges)"""
    mk = make_case
    return [
        mk("reg_last_size", 12288, 12288, 1, 5, 3, 18, 2, 4, finished_row=3),            # min_len == t + 1: <end> removed
        mk("scalar_by_V", 12289, 12289, 3, 5, 2, 18, 2, 2, finished_row=3),              # t == n: first step rule c can fire; min_len == t
        mk("v9490_scalar", 9490, 9490, 3, 5, 17, 18, 3, 0, finished_row=2),              # the last step
        mk("v9490_reg", 9490, 9492, 3, 5, 17, 18, 3, 0, finished_row=2),
        mk("full_lists", 330, 332, 1, 5, 254, 255, 1, 255, n_banned=64),
        mk("full_lists_b1", 330, 330, 1, 1, 254, 255, 1, 255, n_banned=64),
        mk("t0", 9490, 9492, 1, 1, 0, 18, 1, 1),                                         # no history; <end> removed
        mk("n1", 1028, 1028, 3, 5, 4, 18, 1, 0, finished_row=4),
        mk("n16_cannot", 1028, 1028, 1, 5, 15, 18, 16, 0),                               # t == n - 1
        mk("n16_first", 1028, 1029, 1, 5, 16, 18, 16, 17),                               # t == n, scalar by ld
        mk("n2_far", 203, 204, 3, 5, 9, 18, 2, 9),                                       # min_len == t: <end> allowed
    ]


def case_reg(c):
    return TS.is_reg(c.V, c.ld)


def x64_of(c):
    return PO.slab_logits(c.slabs, c.bias, c.V)


# ------------------------------------------------------------------------------------------- n-gram rule on a decoded sequence
def violations(seq_row, start, end_rewritten_zero, cons, V):
    """(a, b, c) counts over one decoded row `seq_row` (words, 0 after the end): a banned word, an end before min_len words,
    an n-gram of words occurring twice"""
    words = []
    for w in seq_row:
        if int(w) == 0:
            break
        words.append(int(w))
    a = sum(1 for w in words if w in cons.banned)
    b = 1 if (len(words) < cons.min_len and len(words) < len(seq_row)) else 0
    c = 0
    n = cons.ngram
    if n >= 1:
        seen = set()
        for i in range(len(words) - n + 1):
            g = tuple(words[i:i + n])
            c += g in seen
            seen.add(g)
    return a, b, c
