"""CPU: the fixtures of DCNet's persistent Gumbel launch test (tests/dcnet_gumbel_fixtures.py) under the numpy oracle alone — the
seeds and <end> boosts are fixed here, without the device: rows finish at different steps, no decision of the oracle's own rollout
comes within ten times the "either word" gap, and the five samples of one caption differ.  Also the new C entry's refusals that
need no device."""
import ctypes as C

import numpy as np
import pytest

import dcnet_gumbel_fixtures as DF

ARG, UNSUPPORTED = 1, 2


@pytest.fixture(scope="module")
def case_data():
    from oracle import cases
    return cases.build_dcnet(DF.CASE)


@pytest.mark.parametrize("case", DF.CASES)
def test_fixture_rollout_under_the_oracle(case_data, case):
    """the numpy model's own Gumbel rollout of every case, for the listed seed and boost: every row ends inside MAX_LEN; at B > 1
    one row ends at the first step and the rows end at >= 3 different steps (2 rows: at 2); NO live decision has a top-two gap of
    y + g below 10 x gap_limit (gap_limit = 4e-4 inv_t + 4e-5, gumbel_fixtures.gap_limit: the project's 1e-4 logit parity and the
    1e-5 noise bound) — so on these seeds the reference alone never needs the GPU test's "either word" allowance; the five rows
    of the 5-row case, which share one previous caption, are pairwise different."""
    seq, gaps = DF.oracle_rollout(case_data, case)
    B = DF.ROWS[case]
    prev, plen = DF.inputs(case)
    assert prev.shape[0] == B and plen.shape == (B, 1)
    finish = DF.finish_steps(seq)
    print("case %r: finish %r, %d decisions, smallest gap %.4f" % (case, finish, len(gaps), min(g for _, _, g in gaps)))
    assert max(finish) < DF.MAX_LEN, finish
    if B > 1:
        assert 0 in finish and len(set(finish)) >= min(3, B), finish
    near = [(b, t, g) for b, t, g in gaps if g < 10 * DF.gap_limit(case)]
    assert not near, near
    if case == 5:
        assert (prev == prev[0]).all() and (plen == plen[0]).all()
        assert len({tuple(r) for r in seq.tolist()}) == 5, seq


def test_fixture_shapes():
    """1 and 4 rows at T = 18 (resident variant: B <= 4, T <= 20), 5 and 8 rows (general), 2 rows padded to T = 24 with the lengths
    unchanged; temperature 0.5 on one case"""
    T = {c: DF.inputs(c)[0].shape[1] for c in DF.CASES}
    assert T == {1: 18, 4: 18, 5: 18, 8: 18, "2pad": DF.PAD_T} and 20 < DF.PAD_T < 32
    prev, plen = DF.inputs("2pad")
    assert int(plen.max()) <= 18 and (prev[:, 18:] == 0).all()
    for b in range(2):
        assert (prev[b, :plen[b, 0]] > 0).all() and (prev[b, plen[b, 0]:] == 0).all()
    assert sorted(DF.TEMPERATURE.values()) == [0.5, 1.0, 1.0, 1.0, 1.0]


def test_persistent_entry_refuses_without_a_device():
    """set_dcnet_gumbel_persistent with well-formed dims: SET_ERR_ARG for truncation options, a bad temperature, max_len > 255,
    max_len > maxT and NULL outputs; SET_ERR_UNSUPPORTED for a model without a token table — all before any HIP call, nothing
    written"""
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib as L
    lib = L.load()
    assert "set_dcnet_gumbel_persistent" not in L.MISSING and hasattr(lib, "set_dcnet_gumbel_persistent")
    block = np.full(4096, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 64
    dw = L.DcnetWeights()

    def call(o=None, max_len=18, maxT=19, seq=base + 1536):
        dd = L.DcnetDims(B=2, T=9, D=64, A=32, C=32, E=64, V=203, maxT=maxT)
        return lib.set_dcnet_gumbel_persistent(C.byref(dw), C.byref(dd), base + 512, base + 1024, 1, 2, max_len, 5, 6, seq,
                                               base + 2048, base + 2560, 16, None, C.byref(o) if o is not None else None)

    for kw in (dict(top_k=5), dict(top_p=0.9), dict(temperature=0.0), dict(temperature=float("nan")), dict(top_k=-1)):
        o = L.SampleOpts(**dict(dict(temperature=1.0, top_k=0, top_p=1.0), **kw))
        assert call(o) == ARG, kw
    assert call(max_len=256, maxT=300) == ARG
    assert call(max_len=20) == ARG
    assert call(seq=None) == ARG
    assert call() == UNSUPPORTED
    assert call(L.SampleOpts(temperature=0.5, top_k=0, top_p=1.0)) == UNSUPPORTED
    assert (block == 0xA5).all()
