"""Integer / float64 restatement of the word edit distance on token lists, written from the definitions and independent of
show_edit_tell_amd/editdist.py: the yardstick of tests/test_edit_cpu.py and the tests/test_hip_edit_*.py files.

    T[i][j]    = the unit-cost Levenshtein distance of a[:i] and b[:j], the textbook (m + 1) x (n + 1) table
    sim(h, r)  = (m - d) / m, m = max(len h, len r);  1 when both are empty
    stats      = [dist, len_h, len_r, ref] of the reference with the largest sim (Fractions; of equal ones the first)
    corpus     = {'similarity': the mean of the sentence sims, 'wer': sum dist / sum len_r (0 without reference words)}
    script     = the canonical walk-back through T (keep, then substitute, then insert, else delete)
and a plain-Python restatement of the 64-bit column recurrence the kernels run, with the popcount formula of a table cell.
"""
from fractions import Fraction

KEEP, SUB, INS, DEL = 1, 2, 3, 3
W = (1 << 64) - 1


def table(a, b):
    m, n = len(a), len(b)
    T = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        T[i][0] = i
    for j in range(n + 1):
        T[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            T[i][j] = min(T[i - 1][j - 1] + (a[i - 1] != b[j - 1]), T[i - 1][j] + 1, T[i][j - 1] + 1)
    return T


def dist(a, b):
    return table(a, b)[len(a)][len(b)]


def frac(d, lh, lr):
    m = max(lh, lr)
    return Fraction(m - d, m) if m else Fraction(1, 1)


def stats(h, R):
    """[dist, len_h, len_r, ref] of hypothesis h (list) against the references R (non-empty list of lists)"""
    best = None
    for k, r in enumerate(R):
        d = dist(h, r)
        s = frac(d, len(h), len(r))
        if best is None or s > best[0]:
            best = (s, [d, len(h), len(r), k])
    return best[1]


def score(st):
    d, lh, lr = int(st[0]), int(st[1]), int(st[2])
    m = max(lh, lr)
    return (m - d) / m if m else 1.0


def sentence(h, R):
    return score(stats(h, R))


def corpus(pairs):
    sts = [stats(h, R) for h, R in pairs]
    words = sum(s[2] for s in sts)
    return {"similarity": sum(score(s) for s in sts) / len(sts) if sts else 0.0,
            "wer": sum(s[0] for s in sts) / words if words else 0.0}


def script(src, hyp):
    """canonical walk-back -> (hyp_ops, hyp_src, src_ops, [keep, sub, ins, del])"""
    T = table(src, hyp)                                            # rows: src, columns: hyp
    i, j = len(src), len(hyp)
    hyp_ops, hyp_src, src_ops, cnt = [0] * j, [-1] * j, [0] * i, [0, 0, 0, 0]
    while i or j:
        if i and j and src[i - 1] == hyp[j - 1] and T[i][j] == T[i - 1][j - 1]:
            hyp_ops[j - 1], hyp_src[j - 1], src_ops[i - 1] = KEEP, i - 1, KEEP
            cnt[0] += 1; i -= 1; j -= 1
        elif i and j and T[i][j] == T[i - 1][j - 1] + 1:
            hyp_ops[j - 1], hyp_src[j - 1], src_ops[i - 1] = SUB, i - 1, SUB
            cnt[1] += 1; i -= 1; j -= 1
        elif j and T[i][j] == T[i][j - 1] + 1:
            hyp_ops[j - 1] = INS
            cnt[2] += 1; j -= 1
        else:
            assert i > 0 and T[i][j] == T[i - 1][j] + 1
            src_ops[i - 1] = DEL
            cnt[3] += 1; i -= 1
    return hyp_ops, hyp_src, src_ops, cnt


def align_stats(src, hyp):
    """the eight integers of one aligned row: dist, len_h, len_s, keep, sub, ins, del, unchanged"""
    d = dist(src, hyp)
    return [d, len(hyp), len(src)] + script(src, hyp)[3] + [1 if d == 0 else 0]


def bit_parallel(rows, cols):
    """The 64-bit recurrence (Myers / Hyyro, global distance): `rows` (<= 64 tokens) lies along the bits, `cols` is walked.
    Returns (distance, [(Pv, Mv) after every column])."""
    m = len(rows)
    assert m <= 64
    if m == 0:
        return len(cols), [(0, 0)] * len(cols)
    mask, top = (1 << m) - 1, 1 << (m - 1)
    Pv, Mv, d, hist = mask, 0, m, []
    for c in cols:
        Eq = sum(1 << k for k, r in enumerate(rows) if r == c)
        Xv = Eq | Mv
        Xh = ((((Eq & Pv) + Pv) & W) ^ Pv) | Eq
        Ph = (Mv | ~(Xh | Pv)) & W
        Mh = Pv & Xh
        d += 1 if Ph & top else 0
        d -= 1 if Mh & top else 0
        Ph = ((Ph << 1) | 1) & W
        Mh = (Mh << 1) & W
        Pv = (Mh | (~(Xv | Ph) & W)) & mask
        Mv = Ph & Xv & mask
        hist.append((Pv, Mv))
    return d, hist


def cell(hist, i, j):
    """T[i][j] from the stored columns: column 0 is T[i][0] = i"""
    if j == 0:
        return i
    Pv, Mv = hist[j - 1]
    low = (1 << i) - 1
    return j + bin(Pv & low).count("1") - bin(Mv & low).count("1")


def cut_after_zero(row):
    """the decoder's rule: a row ends after its first 0, the 0 stays; no 0: the whole row"""
    row = [int(w) for w in row]
    return row[:row.index(0) + 1] if 0 in row else row


def grid(seed=13):
    """The fixed-seed grid of the test files: lengths {0, 1, 2, 7, 63, 64} on both sides, alphabets of 1, 2 and 30 symbols, sets
    of 1 and 5 references.  Returns a list of (h, R) with ids >= 1.  In a set of 5 the first reference has the grid length, the
    others rotate through the lengths (so empty references sit beside others, and similarities tie in small alphabets); with
    the large alphabet one reference is a mutated copy of the hypothesis, so that something matches."""
    import random
    rng = random.Random(seed)
    lengths = (0, 1, 2, 7, 63, 64)
    out = []
    for A in (1, 2, 30):
        words = lambda n: [rng.randint(1, A) for _ in range(n)]
        for lh in lengths:
            for a, lr in enumerate(lengths):
                h = words(lh)
                out.append((h, [words(lr)]))
                R = [words(lr)] + [words(lengths[(a + k) % len(lengths)]) for k in range(1, 5)]
                if A == 30 and lh > 2:
                    c = list(h)
                    c[rng.randrange(len(c))] = rng.randint(1, A)
                    del c[rng.randrange(len(c))]
                    c.insert(rng.randrange(len(c) + 1), rng.randint(1, A))
                    R[2] = c[:lengths[(a + 2) % len(lengths)]] or R[2]
                out.append((h, R))
    return out


def edge_cases():
    """(h, R) beyond the grid: the top bit at m = 64, one repeated id, a reverse, 63 / 64 mixed, an empty hypothesis, sets of 8"""
    import random
    rng = random.Random(5)
    full = list(range(1, 65))
    w = lambda n, A=6: [rng.randint(1, A) for _ in range(n)]
    return [
        (full, [list(full)]),                                      # 64 distinct ids on both sides: distance 0
        (full, [[k + 100 for k in full]]),                         # ... and nothing equal: distance 64
        ([9] * 64, [[9] * 63, [9] * 64, [9]]),
        ([9] * 64, [[9] * 63]),
        ([9] * 64, [[9]]),
        (full, [full[::-1]]),                                      # a sentence against its reverse
        (w(63), [w(64), w(63), w(64, 2)]),
        (w(64), [w(63), w(64), w(63, 2)]),
        (w(64, 2), [w(64, 2)]),
        (w(63, 2), [w(64, 2), w(63, 2)]),
        ([], [w(5), [], w(1)]),                                    # an empty hypothesis: the empty reference is chosen
        ([], [w(3), w(2)]),
        (w(20), [w(5), w(30), w(20), [], w(21), w(19), w(64), w(1)]),          # a set of 8, an empty reference inside
        ([1, 2, 3, 4], [[1, 2, 9, 4, 5, 6, 7, 8], [1, 2], [5, 2, 3, 6], [1, 2, 3, 4, 5, 6, 7, 8], [3, 4], [1, 9, 9, 4],
                        [9, 9, 9, 9, 1, 2, 3, 4], [1, 2, 3, 9, 9, 9, 9, 9]]),  # a set of 8 whose similarities tie at 1/2
    ]
