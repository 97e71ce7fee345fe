"""The two-model stochastic beam search and the threshold without a device: the ensemble through the UNCHANGED float64 oracle
(tests/sbs_oracle.py on L = log(0.5 (softmax_e + softmax_d))), the margins of every fixture the GPU tests compare exactly, the
(k + 1)-th threshold and the importance weights on the table model, the weight arithmetic, and the C ABI.
Fixtures: tests/sbs_ensemble_fixtures.py."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import gumbel_oracle as GO
import sbs_ensemble_fixtures as E
import sbs_fixtures as F
import sbs_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1


# ------------------------------------------------------------------------------------------- 1. the oracle, reused
@pytest.mark.parametrize("name", sorted(E.DIRECT))
def test_the_ensemble_goes_through_the_oracle_unchanged(name):
    """L is normalised, so the oracle's own log-softmax is the identity: its step_logp is L at the picked word.  The oracle
    rounds what it is given to float32, which moves a word by at most 2^-24 |L[v]| and the row's log-sum-exp by at most
    2^-24 sum_v p_v |L[v]| <= 2^-24 ln V (the entropy): that is the bound here, no looser."""
    V, _, k, NI, T, seed = E.DIRECT[name]
    Ls = [E.mean_logp(e, d, T) for e, d in E.direct_logits(name)]
    for L in Ls:
        m = L.max(1)
        lse = m + np.log(np.exp(L - m[:, None]).sum(1))
        assert np.abs(lse).max() < 1e-12
    states = [SO.Image(k) for _ in range(NI)]
    seen = 0
    for t, L in enumerate(Ls):
        for i in range(NI):
            old = states[i]
            states[i], info = SO.pick(old, L[i * k:(i + 1) * k], i, t, seed, E.OFFSET, E.END, 1.0)
            for s in range(k):
                p, w = info["parents"][s], info["words"][s]
                if w < 0 or old.fin[p]:
                    continue                             # a dead slot, or a finished parent carried over (no step was taken)
                want = L[i * k + p, w]
                assert abs(info["step_logp"][s] - want) <= 2.0 ** -24 * (abs(want) + np.log(V)), (t, i, s)
                seen += 1
    assert seen >= E.STEPS * NI


def test_mean_logp_is_the_log_of_the_averaged_softmax():
    e, d = E.direct_logits("v255_k3_ni2")[0]
    for T in (1.0, 0.5):
        ye, yd = (GO.scaled(x, E.inv_t(T)).astype(np.float64) for x in (e, d))
        pe, pd = (np.exp(y - y.max(1, keepdims=True)) for y in (ye, yd))
        want = np.log(0.5 * (pe / pe.sum(1, keepdims=True) + pd / pd.sum(1, keepdims=True)))
        assert np.abs(E.mean_logp(e, d, T) - want).max() < 1e-12
    e, d = E.edge_one_sided()[0]
    L = E.mean_logp(e, d)
    both = np.isinf(e) & np.isinf(d)
    assert both.any() and np.isinf(L[both]).all() and np.isfinite(L[~both]).all()
    one = np.isinf(e) & ~np.isinf(d)
    yd = d.astype(np.float64)
    lsd = yd - np.log(np.exp(yd).sum(1, keepdims=True))
    assert np.abs(L[one] - (lsd[one] - np.log(2.0))).max() < 1e-12          # l = a - ln 2


# ------------------------------------------------------------------------------------------- 2. fixture margins
def test_tolerance_and_gap_follow_the_recipe():
    assert E.TOL == 4.0 * max(E.G_MEASURED, E.PHI_MEASURED) and E.GAP == 2.0 * E.TOL
    assert max(E.G_MEASURED, E.PHI_MEASURED) <= 1e-4
    assert E.SEPARATION == 0.01 and E.SEPARATION >= 10.0 * E.GAP


@pytest.mark.parametrize("name", sorted(E.DIRECT))
def test_direct_fixtures_keep_their_separation_and_carry_a_finished_slot(name):
    V, ld, k, NI, T, seed = E.DIRECT[name]
    assert E.REGISTER_PATH[name] == (V <= 12288 and ld % 4 == 0)
    Ls = [E.mean_logp(e, d, T) for e, d in E.direct_logits(name)]
    _, infos = E.search_with_fin(Ls, NI, k, seed)
    m = E.smallest_margin(infos)
    print(name, "smallest distance of adjacent candidates: %.4f" % m)
    assert m >= E.SEPARATION and E.finished_slot_carries(infos)
    assert all(not E.good_seed(Ls, NI, k, s) for s in range(1, seed))          # the smallest such seed


def test_shapes_are_the_issues():
    assert sorted((v[0], v[1], v[2], v[3]) for v in E.DIRECT.values()) == [
        (255, 256, 3, 2), (1027, 1027, 8, 1), (4099, 4100, 5, 3), (12289, 12292, 3, 1)]


def test_layout_degenerate_and_edge_fixture_margins():
    name, ld_a, ld_b = E.LAYOUT
    assert E.DIRECT[name][0] == 1027 and (ld_a, ld_b) == (1027, 1028)
    for name in E.DEGENERATE:                            # logits2 == logits: the one-model oracle on the same logits
        V, _, k, NI, T, seed = E.DIRECT[name]
        L1 = [e for e, _ in E.direct_logits(name)]
        _, infos = SO.search(lambda t, st: L1[t], NI, k, len(L1), seed, E.OFFSET, E.END, E.inv_t(T))
        assert E.smallest_margin(infos) >= 10.0 * E.GAP, name
        _, infos = E.oracle_search([E.mean_logp(e, e, T) for e in L1], NI, k, seed)
        assert E.smallest_margin(infos) >= 10.0 * E.GAP, name
    for key, fn in (("one_sided", E.edge_one_sided), ("few_words", E.edge_few_words)):
        Ls = [E.mean_logp(e, d) for e, d in fn()]
        _, infos = E.oracle_search(Ls, 1, E.EDGE_K, E.EDGE_SEED[key])
        assert E.smallest_margin(infos) >= E.SEPARATION, key
    # the few-words fixture does what its docstring says
    states, infos = E.oracle_search([E.mean_logp(e, d) for e, d in E.edge_few_words()], 1, E.EDGE_K, E.EDGE_SEED["few_words"])
    live = [sum(1 for w in step[0]["words"] if w >= 0) for step in infos[:3]]
    assert live == [1, 2, 2] and infos[3][0].get("noop") and states[0].n_open == 0


@pytest.mark.parametrize("n,NI", sorted(E.SEARCH_SEED))
def test_search_seeds_keep_the_numpy_models_own_search_apart(n, NI):
    """the numpy models' own ensemble search (no GPU): no margin below 0.01, a sequence finishes, entries are distinct"""
    states, infos = E.numpy_search(n, NI, E.SEARCH_SEED[(n, NI)])
    m = E.smallest_margin(infos)
    print((n, NI), "smallest margin %.4f" % m, [[st.toks[s] for s in range(n)] for st in states])
    assert m >= E.SEPARATION
    for st in states:
        seqs = [tuple(st.toks[s]) for s in range(n) if st.G[s] > -np.inf]
        assert len(set(seqs)) == len(seqs) == n
    assert any(st.fin.any() for st in states)


# ------------------------------------------------------------------------------------------- 3. threshold
@pytest.fixture(scope="module")
def table_draws():
    """TABLE_DRAWS searches of the table model with TABLE_K + 1 slots at seeds 1 .. TABLE_DRAWS: per draw the entries
    [(tokens, phi, G)] and kappa"""
    out = []
    for seed in range(1, F.TABLE_DRAWS + 1):
        st = E.table_search(seed, F.TABLE_K + 1)
        ent = [(tuple(st.toks[s]), float(st.phi[s]), float(st.G[s])) for s in range(F.TABLE_K + 1)]
        assert all(e[2] > -np.inf for e in ent)          # the table model has more than three leaves
        out.append((ent[:F.TABLE_K], ent[F.TABLE_K][2]))
    return out


def test_first_two_of_three_slots_follow_sampling_without_replacement(table_draws):
    leaves = F.table_leaves()
    keys = sorted(leaves)
    pairs = [(a, b) for a, b in itertools.product(keys, keys) if a != b]
    p = np.array([np.exp(leaves[a]) * np.exp(leaves[b]) / (1.0 - np.exp(leaves[a])) for a, b in pairs])
    index = {ab: i for i, ab in enumerate(pairs)}
    counts = np.zeros(len(pairs), np.int64)
    for ent, kappa in table_draws:
        counts[index[(ent[0][0], ent[1][0])]] += 1
        assert ent[0][2] >= ent[1][2] >= kappa
    chi2, bins, pv = GO.chi_square_pvalue(counts, p)
    print("pair of three slots: chi2 %.2f over %d bins, p = %.4f" % (chi2, bins, pv))
    assert pv > 1e-3


def test_importance_weighted_estimate_of_the_sequence_length_is_unbiased(table_draws):
    from show_edit_tell_amd import evaluate
    leaves = F.table_leaves()
    exact = sum(np.exp(lp) * len(s) for s, lp in leaves.items())
    est = []
    e = np.random.RandomState(20261019).exponential(size=len(table_draws))   # the un-conditioning draws, one per search
    for (ent, kappa), ei in zip(table_draws, e):
        assert ent[0][2] == 0.0                          # the search conditions the largest G on being 0 ...
        kappa = evaluate.sbs_unconditioned_threshold(kappa, ei)              # ... which the threshold must not be
        w = evaluate.sbs_importance_weights([(list(s), phi, G, True) for s, phi, G in ent], kappa, normalize=False)
        est.append(sum(wi * len(s) for wi, (s, _, _) in zip(w, ent)))
    est = np.array(est)
    mean, se = est.mean(), est.std(ddof=1) / np.sqrt(len(est))
    print("E[len] exact %.5f, estimate %.5f +- %.5f (%.2f standard errors)" % (exact, mean, se, (mean - exact) / se))
    assert abs(mean - exact) <= 4.0 * se


# ------------------------------------------------------------------------------------------- 4. weight arithmetic
def test_importance_weights_against_the_direct_formula():
    from show_edit_tell_amd import evaluate
    ent = lambda phis: [([1, 0], float(p), 0.0, True) for p in phis]
    phi = np.array([-0.5, -1.25, -3.0, -7.5])
    for kappa in (-2.0, -0.1, -9.0):
        q = 1.0 - np.exp(-np.exp(phi - kappa))
        w = evaluate.sbs_importance_weights(ent(phi), kappa, normalize=False)
        assert w.dtype == np.float64 and np.allclose(w, np.exp(phi) / q, rtol=1e-12, atol=0.0)
        wn = evaluate.sbs_importance_weights(ent(phi), kappa)
        assert np.allclose(wn, w / w.sum(), rtol=1e-12, atol=0.0) and abs(wn.sum() - 1.0) < 1e-12
    # kappa = -inf: q = 1, the weights are the probabilities
    w = evaluate.sbs_importance_weights(ent(phi), float("-inf"), normalize=False)
    assert np.array_equal(w, np.exp(phi))
    # phi - kappa = -40: q = exp(-40) to full precision (1 - exp(-x) would cancel to 0), so w = exp(kappa) (1 + x / 2 + ...)
    kappa = -3.0
    w = evaluate.sbs_importance_weights(ent([kappa - 40.0]), kappa, normalize=False)
    x = np.exp(-40.0)
    assert np.isfinite(w[0]) and abs(w[0] / (np.exp(kappa - 40.0) / (x - x * x / 2.0)) - 1.0) < 1e-14
    assert abs(w[0] / np.exp(kappa) - 1.0) < 1e-14
    assert len(evaluate.sbs_importance_weights([], -1.0)) == 0


def test_unconditioned_threshold_arithmetic():
    import torch
    from show_edit_tell_amd import evaluate
    f = evaluate.sbs_unconditioned_threshold
    for kappa, e in ((-0.3, 0.5), (-2.0, 1.0), (-5.0, 3.25), (-1e-9, 1e-3)):
        assert abs(f(kappa, e) - -np.log(np.exp(-kappa) + e - 1.0)) <= 1e-12 * max(1.0, abs(f(kappa, e))) + 1e-7 * (kappa > -1e-6)
    assert abs(f(-1.5, 1.0) + 1.5) < 1e-12               # E = 1 is Z = 0: nothing to take out
    assert f(float("-inf"), 0.7) == float("-inf")
    assert abs(f(0.0, 0.25) + np.log(0.25)) < 1e-12                 # the largest score itself goes to Z = -log E
    assert np.allclose(f([-1.0, -2.0], [1.0, 1.0]), [-1.0, -2.0], rtol=1e-12) and isinstance(f([-1.0], [1.0]), list)
    a, b = f(-3.0, 0.5), f(-2.0, 0.5)
    assert a < b                                         # increasing
    torch.manual_seed(5)
    x = f([-1.0, -1.0, -1.0])
    torch.manual_seed(5)
    assert x == f([-1.0, -1.0, -1.0]) and len(set(x)) == 3


# ------------------------------------------------------------------------------------------- 5. ABI
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_entry_is_declared_bound_and_exported_and_the_struct_is_untouched(lib):
    from show_edit_tell_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "set_hip.h")).read()
    name = "set_sbs_pick_ensemble_f32"
    assert re.search(r"\bint %s\s*\(const SetSbsArgs\*[^,]*,\s*const float\*[^,]*,\s*const SetSampleOpts\*[^,]*,\s*void\*" % name,
                     header)
    assert name in L.PROTOTYPES and name not in L.MISSING and hasattr(lib, name)
    # SetSbsArgs as tests/test_sbs_abi_cpu.py reads and pins it: the header's fields in order, 16 x 8 + 6 x 4 bytes
    body = re.search(r"typedef struct SetSbsArgs \{(.*?)\} SetSbsArgs;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for n in re.findall(r"\w+", body) if n not in ("float", "int32_t", "int64_t", "uint64_t", "void", "size_t", "const")]
    assert names == [f for f, _ in L.SbsArgs._fields_], names
    assert C.sizeof(L.SbsArgs) == 16 * 8 + 6 * 4
    eight = ["logits", "ld", "end_idx", "seed", "offset", "phi", "G", "finished", "len", "seqs_in", "seqs_out", "words", "rows",
             "n_open", "ws", "ws_bytes"]
    four = ["NI", "k", "V", "t", "Lmax", "pad_"]
    assert names == eight + four
    assert [getattr(L.SbsArgs, n).offset for n in names] == [8 * i for i in range(16)] + [128 + 4 * i for i in range(6)]


def test_refusals_without_a_device(lib):
    """host memory stands in for the device buffers: every refusal comes before any HIP call, with nothing written"""
    from show_edit_tell_amd._lib import SampleOpts, SbsArgs
    block = np.full(1 << 16, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 256
    NI, k, V = 2, 3, 50

    def call(logits2=base + 2048, opts=None, **over):
        a = SbsArgs(logits=base, ld=52, end_idx=3, seed=1, offset=2, phi=base + 4096, G=base + 4352, finished=base + 4608,
                    len=base + 4864, seqs_in=base + 5120, seqs_out=base + 6144, words=base + 7168, rows=base + 7424,
                    n_open=base + 7680, ws=base + 8192, ws_bytes=lib.set_sbs_workspace_bytes(NI, k), NI=NI, k=k, V=V, t=0, Lmax=4)
        for key, val in over.items():
            setattr(a, key, val)
        return lib.set_sbs_pick_ensemble_f32(C.byref(a), logits2, C.byref(opts) if opts is not None else None, None)

    assert call(logits2=None) == ARG
    assert lib.set_sbs_pick_ensemble_f32(None, base, None, None) == ARG
    for field in ("logits", "phi", "G", "finished", "len", "seqs_in", "seqs_out", "words", "rows", "n_open", "ws"):
        assert call(**{field: None}) == ARG, field
    for over in (dict(k=0), dict(k=9), dict(t=-1), dict(t=255), dict(V=0), dict(ld=V - 1), dict(NI=0), dict(Lmax=0),
                 dict(ws_bytes=8), dict(end_idx=-1), dict(end_idx=V), dict(seqs_out=base + 5120)):
        assert call(**over) == ARG, over
    for o in (SampleOpts(temperature=1.0, top_k=5, top_p=1.0), SampleOpts(temperature=1.0, top_k=0, top_p=0.9),
              SampleOpts(temperature=0.0, top_k=0, top_p=1.0)):
        assert call(opts=o) == ARG
    assert (block == 0xA5).all()


def test_python_entries_refuse_before_they_touch_a_tensor():
    from show_edit_tell_amd import evaluate

    class Edit:
        _ABI, _adaptive, vocab_size = "editnet", 0, 50

    class Adaptive(Edit):
        _adaptive = 1

    class Dc:
        _ABI, vocab_size = "dcnet", 50

    class DcOther(Dc):
        vocab_size = 51

    wm = {"<start>": 1, "<end>": 2, "<pad>": 0}
    ens = evaluate.sample_captions_distinct_ensemble
    with pytest.raises(ValueError, match="adaptive"):
        ens(Adaptive(), Dc(), None, None, None, wm)
    with pytest.raises(ValueError, match="vocabular"):
        ens(Edit(), DcOther(), None, None, None, wm)
    with pytest.raises(ValueError):
        ens(Dc(), Edit(), None, None, None, wm)          # the models in the wrong order
    for n in (0, 9, 2.5):
        with pytest.raises(ValueError, match="n_samples"):
            ens(Edit(), Dc(), None, None, None, wm, n_samples=n)
    for fn, args in ((ens, (Edit(), Dc(), None, None, None, wm)), (evaluate.sample_captions_distinct, (Edit(), None, None, None, wm))):
        with pytest.raises(ValueError, match="n_samples.*return_threshold"):
            fn(*args, n_samples=8, return_threshold=True)
        with pytest.raises(ValueError, match="max_steps"):
            fn(*args, n_samples=7, return_threshold=True, max_steps=256)          # (7 with the flag passes the slot check)
