"""The truncated stochastic beam search without a device, on the float64 oracle alone (tests/sbs_trunc_oracle.py): every fixture
the GPU tests compare exactly keeps its top-p target clear of a value-group boundary and its candidates apart (zero excluded
cases), and on the table model of tests/sbs_fixtures.py under top-p the search samples the TRUNCATED model without replacement
and the importance weights estimate expectations under it.  Fixtures: tests/sbs_trunc_fixtures.py."""
import itertools

import numpy as np
import pytest

import gumbel_oracle as GO
import sbs_fixtures as F
import sbs_trunc_fixtures as T
import sbs_trunc_oracle as TS
import trunc_sample_oracle as TO


# ------------------------------------------------------------------------------------------- 1. fixture conditions
def test_tolerance_gap_and_separation_follow_the_recipe():
    assert T.TOL == 4.0 * max(T.G_MEASURED, T.PHI_MEASURED) and T.GAP == 2.0 * T.TOL
    assert max(T.G_MEASURED, T.PHI_MEASURED) <= 1e-4
    assert T.SEPARATION >= 10.0 * T.GAP and T.BOUNDARY_MIN == 1e-4 and T.CUT_GAP_MIN >= 4.0 * T.TOL


def _conditions(Ls, NI, k, temp, seed, top_k, top_p, ens=False):
    states, infos = T.oracle_run(Ls, NI, k, temp, seed, top_k, top_p)
    m, d, g = TS.smallest_margin(infos), TS.smallest_dist(infos), TS.smallest_gap(infos)
    assert m >= T.SEPARATION and m >= 10.0 * T.GAP, m
    assert d >= T.BOUNDARY_MIN, d
    assert g > 0.0 and (not ens or g >= T.CUT_GAP_MIN), g
    return states, infos


@pytest.mark.parametrize("name", sorted(T.DIRECT))
def test_direct_fixtures_keep_their_conditions(name):
    V, ld, k, NI, temp, seed, top_k, top_p = T.DIRECT[name]
    assert T.is_reg(V, ld) == ("_sc" not in name)
    Ls = T.direct_logits(name)
    states, infos = _conditions(Ls, NI, k, temp, seed, top_k, top_p)
    finish = name != "v255_k8_ni1_k2"
    assert all(not T.good(Ls, NI, k, temp, s, top_k, top_p, finish=finish) for s in range(1, seed))      # the smallest such seed
    # every picked word lies in its parent's kept set, and something is cut at every step of an open image
    for step in infos:
        for info in step:
            for p, w in zip(info["parents"], info["words"]):
                assert w < 0 or info["kept"][p, w] or w == T.END
            assert info.get("noop") or (~info["kept"]).any()
            assert info["kept"][:, V - 1].all()          # the last word (at V % 4 != 0 in the ragged last quad) is a head word
    if name == "v255_k8_ni1_k2":                         # top_k = 2 under 8 slots: 2, 4, 8 live slots at most
        live = [sum(1 for w in step[0]["words"] if w >= 0) for step in infos]
        assert live[0] == 2 and live[1] <= 4 and all(n < 8 for n in live[:2])


def test_shapes_and_options_are_the_issues():
    shapes = {(v[0], v[1]) for v in T.DIRECT.values()}
    assert {(203, 203), (255, 256), (1027, 1028), (1027, 1027), (4099, 4100), (12289, 12292)} <= shapes
    assert {v[2] for v in T.DIRECT.values()} == {1, 3, 8} and {v[3] for v in T.DIRECT.values()} == {1, 3}
    assert {v[4] for v in T.DIRECT.values()} == {1.0, 0.5}
    assert {(5, 1.0), (0, 0.9), (5, 0.9), (2, 1.0)} == {(v[6], v[7]) for v in T.DIRECT.values()}
    assert T.DIRECT["v255_k8_ni1_k2"][2] == 8


@pytest.mark.parametrize("name", sorted(T.LAYOUT))
def test_layout_fixtures_keep_their_conditions(name):
    V, k, NI, temp, seed, ldp, top_k, top_p = T.LAYOUT[name]
    assert T.is_reg(V, ldp) and not T.is_reg(V, V)
    _conditions(T.layout_logits(name), NI, k, temp, seed, top_k, top_p)


@pytest.mark.parametrize("name", sorted(T.ENS_DIRECT))
def test_ensemble_fixtures_keep_their_conditions(name):
    V, ld, k, NI, temp, seed, top_k, top_p = T.ENS_DIRECT[name]
    assert T.is_reg(V, ld) == ("_sc" not in name)
    _conditions(T.ens_logits(name), NI, k, temp, seed, top_k, top_p, ens=True)
    lay, ld_a, ld_b = T.ENS_LAYOUT
    assert lay in T.ENS_DIRECT and not T.is_reg(T.ENS_DIRECT[lay][0], ld_a) and T.is_reg(T.ENS_DIRECT[lay][0], ld_b)


@pytest.mark.parametrize("path", ["reg", "generic"])
@pytest.mark.parametrize("name", sorted(T.SPECIAL))
def test_special_rows_keep_their_conditions_and_their_words(path, name):
    lg, V, ld, want = T.special_logits(path, name)
    _, top_k, top_p, _ = T.SPECIAL[name]
    states, infos = _conditions([lg], 1, T.SPECIAL_K, 1.0, T.SPECIAL_SEED[(path, name)], top_k, top_p)
    got = sorted(w for w in infos[0][0]["words"] if w >= 0)
    if want is not None:
        assert got == want, (got, want)                  # every kept word is a candidate, nothing else is
    if name == "one_word_over_top_p":
        assert states[0].phi[0] == 0.0 and states[0].G[0] == 0.0 and (states[0].G[1:] == -np.inf).all()


def test_minus_inf_rows_keep_their_conditions():
    _, infos = _conditions(F.edge_minus_inf(), 1, F.EDGE_K, 1.0, T.EDGE_SEED, *T.EDGE_OPTS)
    for step in infos:
        assert all(w < 0 or (w % 2 == 1 and w != F.END) for w in step[0]["words"])


# ------------------------------------------------------------------------------------------- 2. the oracle composes as stated
def test_masking_before_the_pick_is_the_renormalised_truncated_model():
    """step_logp of a picked word is y - logsumexp over the kept set; neutral options are sbs_oracle.pick itself"""
    import sbs_oracle as SO
    name = "v255_k3_ni3_kp"
    V, ld, k, NI, temp, seed, top_k, top_p = T.DIRECT[name]
    lg = T.direct_logits(name)[0][:k]
    new, info = TS.pick(SO.Image(k), lg, 0, 0, seed, T.OFFSET, T.END, F.inv_t(temp), top_k, top_p)
    y = GO.scaled(lg[0], F.inv_t(temp)).astype(np.float64)
    kept, _ = TO.kept_set(y[None], top_k, top_p)
    lse = np.log(np.exp(y[kept[0]]).sum())
    for s, w in enumerate(info["words"]):
        if w >= 0:
            assert kept[0][w] and abs(info["step_logp"][s] - (y[w] - lse)) < 1e-12
    a, ia = TS.pick(SO.Image(k), lg, 0, 0, seed, T.OFFSET, T.END, F.inv_t(temp))
    b, ib = SO.pick(SO.Image(k), lg, 0, 0, seed, T.OFFSET, T.END, F.inv_t(temp))
    assert ia["words"] == ib["words"] and np.array_equal(a.G, b.G) and np.array_equal(a.phi, b.phi)


# ------------------------------------------------------------------------------------------- 3. the table model under top-p
@pytest.fixture(scope="module")
def table_draws():
    """TABLE_DRAWS searches of the truncated table model with TABLE_K + 1 slots at seeds 1 .. TABLE_DRAWS"""
    out = []
    for seed in range(1, T.TABLE_DRAWS + 1):
        st = T.table_search(seed, F.TABLE_K + 1)
        ent = [(tuple(st.toks[s]), float(st.phi[s]), float(st.G[s])) for s in range(F.TABLE_K + 1)]
        assert all(e[2] > -np.inf for e in ent)          # the truncated table model has more than three leaves
        out.append((ent[:F.TABLE_K], ent[F.TABLE_K][2]))
    return out


def test_truncated_table_model_is_a_distribution_clear_of_boundaries():
    leaves, dist = T.table_leaves()
    full = F.table_leaves()
    assert dist >= T.BOUNDARY_MIN
    assert 3 < len(leaves) < len(full) and set(leaves) < set(full)
    assert abs(sum(np.exp(v) for v in leaves.values()) - 1.0) < 1e-12
    assert all(leaves[s] > full[s] for s in leaves)      # renormalised: every kept sequence gains


def test_inclusion_follows_the_truncated_model_and_cut_sequences_never_come_back(table_draws):
    leaves, _ = T.table_leaves()
    keys = sorted(leaves)
    pairs = [(a, b) for a, b in itertools.product(keys, keys) if a != b]
    p = np.array([np.exp(leaves[a]) * np.exp(leaves[b]) / (1.0 - np.exp(leaves[a])) for a, b in pairs])
    index = {ab: i for i, ab in enumerate(pairs)}
    counts = np.zeros(len(pairs), np.int64)
    for ent, kappa in table_draws:
        for seq, phi, _ in ent:
            assert seq in leaves and abs(phi - leaves[seq]) < 1e-5       # a word outside a step's kept set is never returned;
        counts[index[(ent[0][0], ent[1][0])]] += 1                      # phi is log q (the oracle rounds its input to float32)
        assert ent[0][2] >= ent[1][2] >= kappa
    chi2, bins, pv = GO.chi_square_pvalue(counts, p)
    print("ordered pairs under top_p = %.1f: chi2 %.2f over %d bins, p = %.4f" % (T.TABLE_TOP_P, chi2, bins, pv))
    assert pv > 1e-3


def test_importance_weights_estimate_expectations_under_the_truncated_model(table_draws):
    from show_edit_tell_amd import evaluate
    leaves, _ = T.table_leaves()
    exact_len = sum(np.exp(lp) * len(s) for s, lp in leaves.items())
    one, length = [], []
    e = np.random.RandomState(20261019).exponential(size=len(table_draws))   # the un-conditioning draws, one per search
    for (ent, kappa), ei in zip(table_draws, e):
        assert ent[0][2] == 0.0
        kappa = evaluate.sbs_unconditioned_threshold(kappa, ei)
        w = evaluate.sbs_importance_weights([(list(s), phi, G, True) for s, phi, G in ent], kappa, normalize=False)
        one.append(w.sum())
        length.append(sum(wi * len(s) for wi, (s, _, _) in zip(w, ent)))
    for what, est, exact in (("E_q[1]", np.array(one), 1.0), ("E_q[len]", np.array(length), exact_len)):
        mean, se = est.mean(), est.std(ddof=1) / np.sqrt(len(est))
        print("%s exact %.5f, estimate %.5f +- %.5f (%.2f standard errors)" % (what, exact, mean, se, (mean - exact) / se))
        assert abs(mean - exact) <= 4.0 * se
