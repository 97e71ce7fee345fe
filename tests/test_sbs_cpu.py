"""Stochastic beam search on the float64 oracle alone (tests/sbs_oracle.py): the distribution of what it returns, the structure
of a pick, and the margins of every fixture the GPU tests compare exactly (tests/sbs_fixtures.py)."""
import itertools

import numpy as np
import pytest

import gumbel_oracle as GO
import sbs_fixtures as F
import sbs_oracle as SO


def _table_search(seed, k=F.TABLE_K):
    def logits_of(t, states):
        return np.stack([F.table_logits(tuple(states[0].toks[j])) for j in range(k)])
    states, infos = SO.search(logits_of, 1, k, F.TABLE_STEPS, seed, F.OFFSET, F.TABLE_END)
    return states[0], infos


@pytest.fixture(scope="module")
def table_draws():
    """the 4000 searches of the table model at seeds 1 .. 4000 (fixed when the test was written): (first, second) sequences"""
    out = []
    for seed in range(1, F.TABLE_DRAWS + 1):
        st, _ = _table_search(seed)
        out.append((tuple(st.toks[0]), tuple(st.toks[1])))
    return out


# ------------------------------------------------------------------------------------------- 1. distribution
def test_first_drawn_sequence_follows_the_model(table_draws):
    leaves = F.table_leaves()
    keys = sorted(leaves)
    p = np.exp([leaves[s] for s in keys])
    assert abs(p.sum() - 1.0) < 1e-12
    counts = np.array([sum(1 for a, _ in table_draws if a == s) for s in keys])
    assert counts.sum() == F.TABLE_DRAWS                 # every first sequence is a leaf
    chi2, bins, pv = GO.chi_square_pvalue(counts, p)
    print("first: chi2 %.2f over %d bins, p = %.4f" % (chi2, bins, pv))
    assert pv > 1e-3


def test_ordered_pair_follows_sampling_without_replacement(table_draws):
    leaves = F.table_leaves()
    keys = sorted(leaves)
    pairs = [(a, b) for a, b in itertools.product(keys, keys) if a != b]
    p = np.array([np.exp(leaves[a]) * np.exp(leaves[b]) / (1.0 - np.exp(leaves[a])) for a, b in pairs])
    assert abs(p.sum() - 1.0) < 1e-12
    index = {ab: i for i, ab in enumerate(pairs)}
    counts = np.zeros(len(pairs), np.int64)
    for ab in table_draws:
        counts[index[ab]] += 1                           # (KeyError: a repeated or impossible sequence)
    chi2, bins, pv = GO.chi_square_pvalue(counts, p)
    print("pair: chi2 %.2f over %d bins, p = %.4f" % (chi2, bins, pv))
    assert pv > 1e-3


# ------------------------------------------------------------------------------------------- 2. structure
@pytest.mark.parametrize("name", ["v255_k3_ni3", "v1027_k8_ni1"])
def test_structure_of_every_pick(name):
    V, _, k, NI, T, seed = F.DIRECT[name]
    L = F.direct_logits(name)
    states = [SO.Image(k) for _ in range(NI)]
    for t in range(F.STEPS):
        for i in range(NI):
            old = states[i]
            states[i], info = SO.pick(old, L[t][i * k:(i + 1) * k], i, t, seed, F.OFFSET, F.END, F.inv_t(T))
            new = states[i]
            live = [s for s in range(k) if new.G[s] > -np.inf]
            seqs = [tuple(new.toks[s]) for s in live]
            assert len(set(seqs)) == len(seqs)                               # distinct
            assert all(new.G[a] >= new.G[b] for a, b in zip(live, live[1:]))  # non-increasing over slots
            for s in live:
                assert new.G[s] <= old.G[info["parents"][s]]                 # a child never beats its parent
            # the arg-max child of every live unfinished parent carries the parent's G exactly
            for j in range(k):
                if old.G[j] == -np.inf or old.fin[j]:
                    continue
                y = GO.scaled(L[t][i * k + j], F.inv_t(T)).astype(np.float64)
                g = old.phi[j] + (y - np.log(np.exp(y - y.max()).sum()) - y.max()) + GO.noise(seed, F.OFFSET, [i * k + j], t, V)[0]
                gt = SO.conditioned(old.G[j], g)
                assert gt[int(np.argmax(g))] == old.G[j] and (gt <= old.G[j]).all()


def test_one_slot_is_the_gumbel_max_draw():
    """k = 1: the word of every step is gumbel_oracle.draw's (the arg-max of y + g; phi and the log-sum-exp shift every word alike)"""
    name = "v255_k1_ni1"
    V, _, k, NI, T, seed = F.DIRECT[name]
    L = F.direct_logits(name)
    for s2 in (seed, seed + 1, seed + 2):
        st = SO.Image(1)
        for t in range(F.STEPS):
            if st.fin[0]:
                break
            ids, _, _, logp, _ = GO.draw(L[t][:1], s2, F.OFFSET, t, F.inv_t(T))
            phi0 = st.phi[0]
            st, info = SO.pick(st, L[t][:1], 0, t, s2, F.OFFSET, F.END, F.inv_t(T))
            assert info["words"][0] == int(ids[0])
            assert st.G[0] == 0.0                        # one slot: always the arg-max child of the root
            assert abs((st.phi[0] - phi0) - logp[0]) < 1e-12


# ------------------------------------------------------------------------------------------- 3. fixture margins
def _margins(L, NI, k, seed, T):
    _, infos = SO.search(lambda t, s: L[t], NI, k, len(L), seed, F.OFFSET, F.END, F.inv_t(T))
    return min(SO.margin(i) for step in infos for i in step)


def test_tolerance_and_gap_follow_the_recipe():
    assert F.TOL == 4.0 * max(F.G_MEASURED, F.PHI_MEASURED) and F.GAP == 2.0 * F.TOL and F.MARGIN == 10.0 * F.GAP
    assert F.G_MEASURED <= 1e-4


@pytest.mark.parametrize("name", sorted(F.DIRECT))
def test_direct_fixture_margins(name):
    V, _, k, NI, T, seed = F.DIRECT[name]
    m = _margins(F.direct_logits(name), NI, k, seed, T)
    print(name, "smallest distance of adjacent candidates: %.4f (needs %.4f)" % (m, F.MARGIN))
    assert m >= F.MARGIN


def test_layout_edge_and_statistics_fixture_margins():
    for name, (V, k, NI, T, seed, _) in F.LAYOUT.items():
        assert _margins(F.layout_logits(name), NI, k, seed, T) >= F.MARGIN, name
    for fn in (F.edge_minus_inf, F.edge_one_word):
        assert _margins(fn(), 1, F.EDGE_K, F.EDGE_SEED, 1.0) >= F.MARGIN, fn.__name__
    assert _margins(F.edge_closed_and_open(), 2, F.EDGE_K, F.MIXED_SEED, 1.0) >= F.MARGIN
    # the one-launch statistics: a near tie there is counted by the GPU test, not assumed away; the oracle's own pairs pass
    lg = np.tile(GO.SEVEN_WORDS, (2 * F.STAT_NI, 1))
    pairs, near = _stat_pairs(lg)
    counts, p = F.stat_counts(pairs)
    chi2, bins, pv = GO.chi_square_pvalue(counts, p)
    print("statistics fixture: chi2 %.2f over %d bins, p = %.4f; %d near ties" % (chi2, bins, pv, near))
    assert pv > 1e-3 and near <= F.NEAR_TIE_FRACTION * F.STAT_NI


def _stat_pairs(lg):
    pairs, near = [], 0
    for i in range(F.STAT_NI):
        st, info = SO.pick(SO.Image(2), lg[2 * i:2 * i + 2], i, 0, F.STAT_SEED, F.OFFSET, 6)
        pairs.append((info["words"][0], info["words"][1]))
        near += SO.margin(info) < F.GAP
    return pairs, near
