"""CPU: the Gumbel-max sampler's definition (include/set_hip.h "Gumbel-max draw") in its float64 restatement
(tests/gumbel_oracle.py), the refusals of the new C entries and of the Python option, and the near-tie budget of the fixtures the
GPU tests (tests/test_hip_gumbel_sampling.py) use."""
import ctypes as C

import numpy as np
import pytest

import gumbel_fixtures as GF
import gumbel_oracle as GO
from oracle import philox_np

ARG, UNSUPPORTED, WORKSPACE = 1, 2, 4


# ------------------------------------------------------------------------------------------- 1. the noise
def test_noise_matches_direct_float64_evaluation():
    """g(r) = -log(-log((r + 1/2) 2^-32)) for the corner words and a few thousand random ones.  The direct evaluation needs more
    than float64 near r = 2^32 - 1 (1 - u = 2^-33 is lost in u), so it is made in extended precision where the platform has it and
    from the series -log(1 - x) = x + x^2 / 2 + ... otherwise."""
    rs = np.random.RandomState(1)
    r = np.concatenate([np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint64),
                        rs.randint(0, 2 ** 32, size=4000, dtype=np.uint64)])
    got = GO.noise_of_words(r)
    from fractions import Fraction
    import math
    want = np.empty(len(r))
    for i, ri in enumerate(r.tolist()):
        u = Fraction(2 * ri + 1, 2 ** 33)
        if ri < 2 ** 31:
            E = -math.log(u)                                        # u <= 1/2: exact rational -> one rounding, no cancellation
        else:
            x = float(1 - u)                                        # exact (a 33-bit integer over 2^33)
            E = -math.log1p(-x)
        want[i] = -math.log(E)
    assert np.abs(got - want).max() < 1e-12
    assert abs(got[0] - (-math.log(33 * math.log(2)))) < 1e-12      # r = 0: u = 2^-33
    assert abs(got[4] - 33 * math.log(2)) < 1e-9                    # r = 2^32 - 1: E = 2^-33 (1 + 2^-34 + ...)
    assert np.isfinite(got).all() and got.min() > -3.2 and got.max() < 22.9
    assert abs(got[2] - got[3]) < 1e-9                               # the two branches meet at u = 1/2


def test_counter_layout_is_pinned():
    """word v of (row, t) = output word v & 3 of counter (row, t + 256 ((v >> 2) + 1), offset_lo, offset_hi), key (seed_lo,
    seed_hi): literal Philox outputs (generated once from oracle/philox_np.py, itself pinned by the Random123 vectors)."""
    seed, offset = 0x0123456789ABCDEF, (7 << 40) | 5
    w = GO.words(seed, offset, 3, 7, 1027)
    assert w.shape == (1027,) and w.dtype == np.uint32
    for v in (0, 1, 5, 1026):
        ctr = np.array([[3, 7 + 256 * ((v >> 2) + 1), offset & 0xFFFFFFFF, offset >> 32]], np.uint64)
        assert w[v] == philox_np.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[0, v & 3]
    assert [int(x) for x in w[[0, 1, 5, 1026]]] == PINNED_WORDS
    # a different offset, row or timestep is a different stream
    assert not np.array_equal(w, GO.words(seed, offset + 1, 3, 7, 1027)) and not np.array_equal(w, GO.words(seed, offset, 3, 8, 1027))


PINNED_WORDS = [3397551084, 2682695926, 259695637, 46108679]


def test_gumbel_max_is_a_categorical_draw():
    """arg-max of y + g over the 7-word distribution for 20 000 (row, t) pairs: the chi-square test of tests/test_hip_sampling.py
    (its statistic, its level p > 1e-4) against softmax(y)"""
    row = GO.SEVEN_WORDS
    counts = np.zeros(7, np.int64)
    for t in range(20):
        ids, _, _, _, _ = GO.draw(np.repeat(row[None], 1000, 0), 777, 3, t)
        counts += np.bincount(ids, minlength=7)
    p = np.exp(row.astype(np.float64) - row.max())
    p /= p.sum()
    chi2, nb, pval = GO.chi_square_pvalue(counts, p)
    assert counts.sum() == 20000 and pval > 1e-4, (chi2, nb, pval)


# ------------------------------------------------------------------------------------------- 3. the C ABI and the Python option
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def _opts(t=1.0, k=0, p=1.0):
    from show_edit_tell_amd._lib import SampleOpts
    return SampleOpts(temperature=t, top_k=k, top_p=p)


def test_new_symbols_are_exported(lib):
    from show_edit_tell_amd import _lib as L
    for name in ("set_gumbel_pick_f32", "set_gumbel_fill_f32", "set_editnet_sample_gumbel", "set_dcnet_sample_gumbel",
                 "set_editnet_gumbel_persistent"):
        assert name not in L.MISSING and hasattr(lib, name), name


BAD = [dict(k=5), dict(p=0.9), dict(t=0.0), dict(t=float("nan")), dict(t=1e4), dict(k=-1), dict(p=0.0)]


def test_pick_and_fill_refuse_bad_arguments_without_a_device(lib):
    """SET_ERR_ARG before any HIP call and nothing written: truncation options, a bad temperature, max_len > 255, t > 255"""
    block = np.full(4096, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 64

    def pick(o, max_len=18, t=1, V=50):
        return lib.set_gumbel_pick_f32(base, 64, 2, V, t, max_len, V - 1, 1, 2, base + 512, base + 1024, base + 1536, base + 2048,
                                       base + 2560, base + 3072, base + 3328, None, C.byref(o) if o is not None else None)

    for b in BAD:
        assert pick(_opts(**b)) == ARG, b
    assert pick(None, max_len=256) == ARG and pick(_opts(0.5), max_len=256) == ARG
    assert pick(None, max_len=300, t=256) == ARG
    assert lib.set_gumbel_fill_f32(base, 2, 50, 256, 1, 2, None) == ARG
    assert lib.set_gumbel_fill_f32(base, 2, 50, -1, 1, 2, None) == ARG
    assert lib.set_gumbel_fill_f32(None, 2, 50, 0, 1, 2, None) == ARG
    assert lib.set_gumbel_fill_f32(base, 0, 50, 0, 1, 2, None) == ARG
    assert lib.set_gumbel_fill_f32(base, 1, (1 << 26) - 3, 0, 1, 2, None) == ARG
    assert (block == 0xA5).all()


def test_rollout_entries_refuse_bad_arguments_without_a_device(lib):
    """set_editnet_sample_gumbel / set_dcnet_sample_gumbel / set_editnet_gumbel_persistent with well-formed dims: the refusals
    are SET_ERR_ARG; a temperature alone passes them (the per-step entries go on to the workspace check, the persistent entry
    answers SET_ERR_UNSUPPORTED for a model without a token table) — so each refusal is the arguments'."""
    from show_edit_tell_amd import _lib as L
    block = np.full(4096, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 64
    ew, dw = L.EditNetWeights(), L.DcnetWeights()

    def dims(maxT=19, V=203):
        return (L.EditNetDims(B=2, T=9, R=7, F=128, D=64, A=32, V=V, maxT=maxT, adaptive=0),
                L.DcnetDims(B=2, T=9, D=64, A=32, C=32, E=64, V=V, maxT=maxT))

    def calls(o, max_len=18, maxT=19):
        ed, dd = dims(maxT)
        op = C.byref(o) if o is not None else None
        e = [fn(C.byref(ew), C.byref(ed), base, None, base + 512, base + 1024, 1, 2, max_len, 5, 6, base + 1536, base + 2048,
                base + 2560, 16, None, op) for fn in (lib.set_editnet_sample_gumbel, lib.set_editnet_gumbel_persistent)]
        dc = lib.set_dcnet_sample_gumbel(C.byref(dw), C.byref(dd), base + 512, base + 1024, 1, 2, max_len, 5, 6, base + 1536,
                                         base + 2048, base + 2560, 16, None, op)
        return e[0], e[1], dc

    for b in BAD:
        assert calls(_opts(**b)) == (ARG, ARG, ARG), b
    assert calls(None, max_len=256, maxT=300) == (ARG, ARG, ARG)
    assert calls(None) == (WORKSPACE, UNSUPPORTED, WORKSPACE)
    assert calls(_opts(0.5)) == (WORKSPACE, UNSUPPORTED, WORKSPACE)
    assert (block == 0xA5).all()


def test_python_sampler_option():
    from show_edit_tell_amd import _lib as L
    assert L.check_sampler("cdf", L.sample_opts(0.5, 5, 0.9), False, True, False) is False
    assert L.check_sampler("gumbel", None, False, True, False) is True
    assert L.check_sampler("gumbel", L.sample_opts(0.5), False, True, False) is True
    with pytest.raises(ValueError):
        L.check_sampler("gumbel", L.sample_opts(1.0, 5, 1.0), False, True, False)       # top_k=5
    with pytest.raises(ValueError):
        L.check_sampler("gumbel", L.sample_opts(1.0, 0, 0.9), False, True, False)
    with pytest.raises(ValueError):
        L.check_sampler("gumbel", None, False, True, True)                              # gradients flow
    with pytest.raises(ValueError):
        L.check_sampler("gumbel", None, True, False, False)                             # nothing is sampled
    with pytest.raises(ValueError):
        L.check_sampler("inverse", None, False, True, False)


def test_models_raise_for_top_k_with_gumbel():
    """sampler="gumbel", top_k=5 raises ValueError from the models and from evaluate.sample_captions before anything runs"""
    import torch
    from oracle import cases
    from show_edit_tell_amd import dcnet_rl, editnet_rl, evaluate
    d = cases.build_editnet("editnet_small")
    c, wm = d["case"], d["wm"]
    dec = editnet_rl.DecoderC(wm, c["D"], c["D"], c["D"], c["A"], c["F"]).eval()
    prev, plen, X = torch.from_numpy(d["prev"]), torch.from_numpy(d["plen"]), torch.from_numpy(d["X"])
    with torch.no_grad():
        for call in (lambda: evaluate.sample_captions(dec, X, prev, plen, wm, sampler="gumbel", top_k=5),
                     lambda: evaluate.sample_captions(dec, X, prev, plen, wm, sampler="gumbel", top_p=0.5),
                     lambda: evaluate.sample_captions(dec, X, prev, plen, wm, sampler="nope")):
            with pytest.raises(ValueError):
                call()
    dd = cases.build_dcnet("dcnet_small")
    cd = dd["case"]
    dae = dcnet_rl.DAE(dd["wm"], None, cd["D"], cd["A"], cd["C"], cd["E"]).eval()
    with torch.no_grad(), pytest.raises(ValueError):
        evaluate.sample_captions(dae, torch.from_numpy(dd["prev"]), torch.from_numpy(dd["plen"]), dd["wm"], sampler="gumbel", top_k=5)


# ------------------------------------------------------------------------------------------- 4. the GPU tests' fixtures
def test_pick_fixtures_near_ties_under_the_oracle():
    """the chosen-logits fixtures of the pick test: no row of any (V, rows, temperature) case lies below the 4e-5 gap"""
    for V in (5, 1027, 9490):
        for rows in (1, 3):
            lg = GF.pick_logits(V, rows)
            for inv in (1.0, 2.0):
                _, gap, _, _, _ = GO.draw(lg, GF.PICK_SEED, GF.OFFSET, 0, inv)
                assert (gap > 4e-5).all(), (V, rows, inv, gap.min())


@pytest.mark.parametrize("B", GF.ROWS)
def test_persistent_fixture_near_ties_under_the_oracle(B):
    """the numpy model's own Gumbel rollout of the persistent test's fixture, for the listed seed: decisions whose top-two gap of
    perturbed scores lies below the "either word" limit stay within 2 % of all decisions and never fill a row; rows finish at
    different steps, one of them at the first (B > 1)"""
    from oracle import cases
    d = cases.build_editnet(GF.CASE)
    seq, gaps = GF.oracle_rollout(d, B)
    near = [(b, t) for b, t, g in gaps if g < GF.gap_limit(B)]
    assert len(near) <= GF.NEAR_TIE_FRACTION * len(gaps), (near, len(gaps))
    for b in range(B):
        nb = sum(1 for r, _, _ in gaps if r == b)
        assert sum(1 for r, _ in near if r == b) < nb
    finish = [int((r == 0).argmax()) if (r == 0).any() else GF.MAX_LEN for r in seq]
    if B > 1:
        assert 0 in finish and len(set(finish)) >= 3, finish
