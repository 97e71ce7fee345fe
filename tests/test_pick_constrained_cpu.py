"""CPU: the restatement of the constrained picks (tests/pick_constrained_oracle.py) against a second, brute-force statement of the
rules, and the pin on the GPU tests' fixtures that lets tests/test_hip_pick_constrained.py compare every row."""
import numpy as np
import pytest

import pick_constrained_oracle as PCO
import trunc_sample_oracle as TS


def brute_removed(s, V, end, cons):
    """every word v of [0, V) tried in turn: banned, <end> too early, or appending v to s repeats an n-gram of s[1:]"""
    words, t, n = list(s[1:]), len(s) - 1, cons.ngram
    grams = set(tuple(words[i:i + n]) for i in range(len(words) - n + 1)) if n >= 1 else set()
    out = set()
    for v in range(V):
        if v in cons.banned or (v == end and t < cons.min_len):
            out.add(v)
        elif n >= 1 and len(words) >= n - 1 and tuple((words + [v])[len(words) + 1 - n:]) in grams:
            out.add(v)
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 16])
def test_removed_words_against_brute_force(n):
    """small alphabets so that n-grams repeat; L < n, L == n, L == n + 1 and longer; periodic rows for n = 16"""
    rng = np.random.default_rng(n)
    V, end, fired = 12, 11, 0
    for L in sorted(set([1, 2, max(n - 1, 1), n, n + 1, n + 2, 2 * n + 3, 40])):
        for trial in range(40):
            alpha = int(rng.integers(1, 4))
            s = [5] + [int(w) for w in rng.integers(0, alpha, size=L - 1)]
            if trial % 4 == 0:
                s = [5] + [int(w) for w in np.resize(rng.integers(0, V, size=int(rng.integers(1, 4))), L - 1)]      # periodic
            cons = PCO.Cons(n, int(rng.integers(0, L + 2)), [int(w) for w in rng.integers(-3, V + 3, size=int(rng.integers(0, 4)))])
            got, want = PCO.removed(s, V, end, cons), brute_removed(s, V, end, cons)
            assert got == want, (n, L, s, cons.__dict__, got, want)
            plain = PCO.removed(s, V, end, PCO.Cons(n))
            fired += bool(plain)
            if L < n or L == 1 and n > 1:
                assert not plain, "rule c fired with fewer than n tokens"
    assert fired > 0


def test_rule_c_edges_by_hand():
    c2 = PCO.Cons(2)
    assert PCO.removed([9, 3], 10, 0, c2) == set()                       # L == n: one bigram position would need i = 1 .. 0
    assert PCO.removed([9, 3, 4, 3], 10, 0, c2) == {4}                   # (3, 4) seen, the row ends in 3
    assert PCO.removed([3, 4, 3], 10, 0, c2) == set()                    # <start> takes no part: (3, 4) began at position 0
    assert PCO.removed([9, 3, 3], 10, 0, c2) == {3}                      # L == n + 1
    assert PCO.removed([9, 1, 2, 3], 10, 0, PCO.Cons(1)) == {1, 2, 3}
    assert PCO.removed([9, 1], 10, 4, PCO.Cons(0, 2, [-1, 10, 7])) == {4, 7}
    assert PCO.removed([9, 1, 2], 10, 4, PCO.Cons(0, 2)) == set()        # t == min_len


def test_finished_rows_are_not_masked():
    x = np.zeros((2, 6))
    hist = np.array([[1, 0], [1, 2]])
    m = PCO.masked(x, hist, np.array([0, 1]), 2, 5, PCO.Cons(1, 9, [3]))
    assert np.isfinite(m[0]).all()
    assert np.isinf(m[1]).tolist() == [False, True, True, True, False, True]


CASES = PCO.pick_cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_fixtures_keep_clear_of_boundaries(c):
    """On the float64 oracle alone: every fixture row's greedy arg-max lies 1e-4 above the runner-up among the survivors, no
    sampled draw lies within trunc_sample_oracle.MARGIN_MIN of a CDF boundary and no top-p target within BOUNDARY_MIN of a group
    boundary — and the constraints matter: some live row's arg-max is a removed word, and no finished row is touched."""
    assert c.V > len(c.cons.banned) + 1 + c.max_len
    x = PCO.x64_of(c)
    m = PCO.masked(x, c.hist, c.unf, c.t, c.end, c.cons)
    top2 = -np.sort(-m, axis=1)[:, :2]
    assert (top2[:, 0] - top2[:, 1] >= PCO.GREEDY_GAP_MIN).all(), (c.name, top2)
    live = (c.unf != 0) | (c.t == 0)
    if c.name != "n16_cannot":
        assert (np.isinf(m[live, np.argmax(x, 1)[live]])).any(), (c.name, "no live row loses its arg-max")
    else:
        assert np.array_equal(np.isinf(m), np.isinf(PCO.masked(x, c.hist, c.unf, c.t, c.end, PCO.Cons(0, c.cons.min_len, c.cons.banned))))
    assert np.isfinite(m[~live]).all()
    for opts in PCO.SAMPLE_OPTS:
        st = dict(seq=c.hist.copy(), seq_logp=np.zeros(c.hist.shape), it=np.zeros(c.B, np.int64), unf=c.unf.copy(),
                  alive=np.ones(c.max_len + 2, np.int32))
        d, logp, _ = PCO.sample_step(c.x32, opts, 2024, 5, c.t, PCO.case_reg(c), c.max_len, c.end, st, c.cons)
        assert d.margin.min() >= TS.MARGIN_MIN, (c.name, opts, d.margin.min())
        assert d.dist.min() >= TS.BOUNDARY_MIN, (c.name, opts, d.dist.min())
        assert np.isfinite(logp).all()
        assert np.isfinite(m[np.arange(c.B), d.ids]).all(), "the oracle drew a removed word"
