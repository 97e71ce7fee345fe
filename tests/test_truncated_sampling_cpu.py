"""CPU: the float64 restatement of truncated sampling (tests/trunc_sample_oracle.py) against brute force by sorting and on chosen
rows; the refusals of the four *_opts entry points (answered before any HIP call, nothing written: every pointer is pattern-filled
HOST memory, as in tests/test_pick_abi_cpu.py); the struct size; and the conditions under which the GPU tests may pin kept sets and
draws — asserted here on the oracle alone for every (V, seed, option) combination they use."""
import ctypes as C

import numpy as np
import pytest

import trunc_sample_oracle as TS

OK, ARG, WORKSPACE = 0, 1, 4
BAD_OPTS = [(float("nan"), 0, 1.0), (float("inf"), 0, 1.0), (5e-4, 0, 1.0), (2e3, 0, 1.0), (0.0, 0, 1.0), (-1.0, 0, 1.0),
            (1.0, -1, 1.0), (1.0, 0, float("nan")), (1.0, 0, 0.0), (1.0, 0, -0.5), (1.0, 0, 1.5), (1.0, 0, float("inf"))]
GOOD_OPTS = [(1.0, 0, 1.0), (1e-3, 0, 1.0), (1e3, 0, 1.0), (0.7, 5, 0.9), (1.0, 10 ** 6, 1e-30)]


# ------------------------------------------------------------------------------------------- the oracle itself
def brute_kept(y, top_k, top_p):
    """one row: sort descending, walk"""
    V = len(y)
    order = sorted(range(V), key=lambda v: -y[v])
    kept = set(range(V))
    if 0 < top_k < V:
        tk = y[order[top_k - 1]]
        kept = {v for v in range(V) if y[v] >= tk}
    if top_p < 1.0:
        m = {v: np.exp(y[v] - y[order[0]]) for v in kept}
        M = sum(m[v] for v in order if v in kept)
        acc, out, i = 0.0, set(), 0
        live = [v for v in order if v in kept]
        while i < len(live):
            j = i
            while j < len(live) and y[live[j]] == y[live[i]]:
                j += 1
            acc += sum(m[v] for v in live[i:j])
            out |= set(live[i:j])
            if acc >= top_p * M:
                break
            i = j
        kept = out
    return kept


@pytest.mark.parametrize("seed", range(6))
def test_kept_set_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    V = 37
    y = np.round(rng.standard_normal((5, V)) * 2.0, 1)                       # one decimal: plenty of ties
    for top_k in (0, 1, 2, 5, 36, 37, 44):
        for top_p in (1.0, 1e-6, 0.3, 0.5, 0.9):
            kept, dist = TS.kept_set(y, top_k, top_p)
            for r in range(5):
                want = brute_kept(list(y[r]), top_k, top_p)
                assert set(np.nonzero(kept[r])[0]) == want, (seed, top_k, top_p, r)
                assert int(np.argmax(y[r])) in want
            assert (dist == np.inf).all() if top_p == 1.0 else (dist >= 0).all()


def test_tie_group_at_the_k_boundary_is_kept_whole():
    y = np.array([[5.0, 3.0, 1.0, 3.0, 5.0, 3.0, 0.0, -2.0]])
    kept, _ = TS.kept_set(y, 3, 1.0)
    assert kept[0].tolist() == [True, True, False, True, True, True, False, False]           # 5 words for k = 3
    kept, _ = TS.kept_set(y, 2, 1.0)
    assert kept[0].sum() == 2
    # top-p: the group that crosses the mass comes with all its ties
    m = np.exp(y[0] - 5.0)
    p_two = 2.0 / m.sum()
    kept, dist = TS.kept_set(y, 0, p_two + 0.01)
    assert kept[0].sum() == 5 and abs(dist[0] - 0.01) < 1e-12


def test_both_zeros_are_one_value():
    y = np.array([[2.0, 0.0, -0.0, -1.0, 1.0, -3.0]])
    kept, _ = TS.kept_set(y, 3, 1.0)                                         # the third largest is a zero: both zeros stay
    assert kept[0].tolist() == [True, True, True, False, True, False]
    kept, _ = TS.kept_set(y[:, ::-1], 3, 1.0)
    assert kept[0].tolist() == [False, True, False, True, True, True]
    m = np.exp(y[0] - 2.0)
    kept, _ = TS.kept_set(y, 0, (m[0] + m[4] + 0.5 * m[1]) / m.sum())       # the mass is crossed inside the zero group
    assert kept[0].tolist() == [True, True, True, False, True, False]


def test_all_negative_row_and_a_word_that_alone_exceeds_top_p():
    y = np.array([[-7.0, -3.0, -5.0, -3.5, -9.0]])
    kept, _ = TS.kept_set(y, 2, 1.0)
    assert kept[0].tolist() == [False, True, False, True, False]
    kept, _ = TS.kept_set(y, 0, 1e-6)
    assert kept[0].tolist() == [False, True, False, False, False]
    y = np.array([[0.0, 10.0, 1.0, -2.0]])
    kept, dist = TS.kept_set(y, 0, 0.9)
    assert kept[0].tolist() == [False, True, False, False] and dist[0] > 0.09
    d = TS.truncated_draw(y.astype(np.float32), (1.0, 0, 0.9), 3, 0, row_of=np.zeros(50, int))
    assert (d.ids == 1).all() and d.lse[0] == 10.0 and d.logp[0, 1] == 0.0 and np.isinf(d.logp[0, 0])


def test_truncated_draw_with_neutral_options_is_the_categorical_draw():
    from oracle import philox_np
    rng = np.random.default_rng(1)
    for V, reg in ((203, True), (1500, True)):
        lg = rng.standard_normal((40, V)).astype(np.float32)
        ids, margin, alt = philox_np.categorical_draw(lg, 9, 4, t=2, with_alt=True)
        d = TS.truncated_draw(lg, TS.NEUTRAL, 9, 4, t=2, reg=reg)
        assert np.array_equal(d.ids, ids) and np.allclose(d.margin, margin, rtol=1e-9, atol=1e-15) and np.array_equal(d.alt, alt)
    # the generic enumeration is another order of the same words
    assert sorted(TS.enumeration(1500, False).tolist()) == list(range(1500)) and TS.enumeration(1500, False)[1] == 256


def test_temperature_is_a_float32_product():
    x = np.array([[0.1, 0.7, -3.3]], np.float32)
    assert np.array_equal(TS.scaled(x, 0.7), x * (np.float32(1.0) / np.float32(0.7)))
    assert TS.scaled(x, 0.7).dtype == np.float32


# ------------------------------------------------------------------------------------------- the GPU tests' fixtures
def _conditions(what, logits, opts, reg, B, seed=2024, offset=0, row_of=None):
    d = TS.truncated_draw(logits, opts, seed, offset, reg=reg, row_of=row_of)
    assert d.dist.min() >= TS.BOUNDARY_MIN, (what, opts, "top-p target %.2e from a group boundary" % d.dist.min())
    close = int((d.margin < TS.MARGIN_MIN).sum())
    assert close <= TS.MARGIN_SHARE * B, (what, opts, "%d of %d draws within %.0e of a CDF boundary" % (close, B, TS.MARGIN_MIN))


@pytest.mark.parametrize("n", TS.GRID_N)
@pytest.mark.parametrize("V,ld", TS.GRID_V)
def test_grid_fixtures_keep_clear_of_boundaries(V, ld, n):
    _, _, logits = TS.grid_case(V, n)
    row_of = np.arange(TS.GRID_B) % TS.GRID_R
    for T in TS.GRID_T:
        for top_k, top_p in TS.grid_options(V):
            _conditions(("grid", V, ld, n), logits, (T, top_k, top_p), TS.is_reg(V, ld), TS.GRID_B, row_of=row_of)


@pytest.mark.parametrize("path", sorted(TS.SPECIAL))
def test_special_row_fixtures(path):
    """the chosen rows do what their description says, and their top-p targets and draws keep clear of boundaries too"""
    V, ld, words = TS.SPECIAL[path]
    a, b, c, d, e = words
    x = TS.special_rows(V, words)
    row_of = np.arange(TS.SPECIAL_B) % 4
    for opts in TS.SPECIAL_OPTS:
        _conditions(("special", path), x, opts, TS.is_reg(V, ld), TS.SPECIAL_B, row_of=row_of)
    kept, _ = TS.kept_set(TS.scaled(x, 0.5), 3, 1.0)
    assert sorted(np.nonzero(kept[0])[0]) == sorted([a, b, c, d])
    assert sorted(np.nonzero(kept[1])[0]) == sorted(words) == sorted(np.nonzero(kept[2])[0]) and (x[2] < 0).all()
    for T in (1.0, 2.0):
        kept, dist = TS.kept_set(TS.scaled(x, T), 0, 0.9)
        assert np.nonzero(kept[3])[0].tolist() == [a] and dist[3] > 1e-3


@pytest.mark.parametrize("V,ld,seed", TS.CHI_CASES)
def test_chi_square_fixtures_keep_clear_of_boundaries(V, ld, seed):
    row = TS.chi_row(V, seed)
    B = 8192
    for offset in range(13):
        _conditions(("chi", V), row[None], TS.CHI_OPTS, TS.is_reg(V, ld), B, seed=777, offset=offset, row_of=np.zeros(B, int))
    kept, _ = TS.kept_set(TS.scaled(row[None], TS.CHI_OPTS[0]), TS.CHI_OPTS[1], TS.CHI_OPTS[2])
    assert 3 <= kept.sum() <= 20


# ------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_struct_size_matches_the_header(lib):
    from show_edit_tell_amd._lib import SampleOpts
    assert C.sizeof(SampleOpts) == 16
    assert (SampleOpts.temperature.offset, SampleOpts.top_k.offset, SampleOpts.top_p.offset, SampleOpts.pad_.offset) == (0, 4, 8, 12)


def _opts(o):
    from show_edit_tell_amd._lib import SampleOpts
    return SampleOpts(temperature=o[0], top_k=o[1], top_p=o[2])


def test_pick_entry_points_refuse_bad_options(lib):
    """set_sample_pick_opts_f32 and set_pick_slabs_opts_f32: SET_ERR_ARG and nothing written.  (No call here carries options
    that would be accepted: with these host pointers it would go on to a launch.)"""
    import test_pick_abi_cpu as PA
    from show_edit_tell_amd._lib import PickArgs
    bufs = PA.Bufs()
    p = bufs.p

    def slabs(mode, o):
        a = PickArgs(logits=p["logits"], ld=PA.LD, stride=PA.B * PA.LD, bias=p["bias"], end_idx=PA.V - 1, seq=p["seq"],
                     seq_logp=p["seq_logp"], it=p["it"], unfinished=p["unfinished"], alive=p["alive"], seed=1, offset=2,
                     raw_ids=p["raw_ids"], lse=p["lse"], step_logp=p["step_logp"], n=2, B=PA.B, V=PA.V, t=1, max_len=PA.MAXLEN,
                     D=PA.D, mode=mode)
        return lib.set_pick_slabs_opts_f32(C.byref(a), C.byref(_opts(o)) if o is not None else None, None)

    def pick(o):
        return lib.set_sample_pick_opts_f32(p["logits"], PA.LD, PA.B, PA.V, 1, PA.MAXLEN, PA.V - 1, 1, 2, p["seq"], p["it"],
                                            p["unfinished"], p["alive"], p["raw_ids"], p["lse"], p["step_logp"], None,
                                            C.byref(_opts(o)))

    for o in BAD_OPTS:
        assert slabs(1, o) == ARG and slabs(0, o) == ARG and pick(o) == ARG, o
        assert bufs.untouched(), o
    # greedy mode takes no options: anything but NULL / neutral is refused, in range or not
    for o in GOOD_OPTS[1:]:
        assert slabs(0, o) == ARG, o
    assert bufs.untouched()
    # the other checks of the calls still answer first
    a = PickArgs(logits=None, mode=1)
    assert lib.set_pick_slabs_opts_f32(C.byref(a), C.byref(_opts(GOOD_OPTS[3])), None) == ARG
    assert lib.set_pick_slabs_opts_f32(None, None, None) == ARG
    assert bufs.untouched()


def test_rollout_entry_points_refuse_bad_options(lib):
    """set_editnet_sample_opts / set_dcnet_sample_opts with well-formed dims and a workspace of 16 bytes: options out of range
    are SET_ERR_ARG, options in range reach the workspace check (SET_ERR_WORKSPACE) — so the refusal is the options'."""
    from show_edit_tell_amd import _lib as L
    block = np.full(4096, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 64
    ed = L.EditNetDims(B=2, T=9, R=7, F=128, D=64, A=32, V=203, maxT=19, adaptive=0)
    dd = L.DcnetDims(B=2, T=9, D=64, A=32, C=32, E=64, V=203, maxT=19)
    ew, dw = L.EditNetWeights(), L.DcnetWeights()

    def editnet(o):
        return lib.set_editnet_sample_opts(C.byref(ew), C.byref(ed), base, None, base + 512, base + 1024, 1, 2, 18, 5, 6,
                                           base + 1536, base + 2048, base + 2560, 16, None, C.byref(_opts(o)))

    def dcnet(o):
        return lib.set_dcnet_sample_opts(C.byref(dw), C.byref(dd), base + 512, base + 1024, 1, 2, 18, 5, 6, base + 1536,
                                         base + 2048, base + 2560, 16, None, C.byref(_opts(o)))

    for o in BAD_OPTS:
        assert editnet(o) == ARG and dcnet(o) == ARG, o
    for o in GOOD_OPTS:
        assert editnet(o) == WORKSPACE and dcnet(o) == WORKSPACE, o
    assert (block == 0xA5).all()


def test_python_option_checks():
    from show_edit_tell_amd import _lib as L
    assert L.sample_opts() is None and L.sample_opts(1.0, 0, 1.0) is None
    o = L.sample_opts(0.5, 7, 0.25)
    assert (o.temperature, o.top_k, o.top_p) == (0.5, 7, 0.25)
    for bad in BAD_OPTS:
        with pytest.raises(ValueError):
            L.sample_opts(*bad)
    with pytest.raises(ValueError):
        L.sample_opts(1.0, 2.5, 1.0)
    for args in ((True, True, False), (True, False, False), (False, False, False), (False, True, True)):
        with pytest.raises(ValueError):
            L.refuse_sample_opts(*args)
    L.refuse_sample_opts(False, True, False)
