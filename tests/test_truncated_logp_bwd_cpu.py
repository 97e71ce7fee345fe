"""CPU: the two exports of the truncated log-prob's backward (include/set_hip.h set_sample_pick_opts_key_f32,
set_sample_logp_bwd_opts_f32) and their refusals — answered before any HIP call with nothing written: every pointer is
pattern-filled HOST memory, as in tests/test_truncated_sampling_cpu.py — and, on the float64 oracle alone, the margins of every
fixture row tests/test_hip_truncated_logp_bwd.py pins exact kept sets on."""
import ctypes as C

import numpy as np
import pytest

import trunc_bwd_fixtures as FX
import trunc_sample_oracle as TS
from test_truncated_sampling_cpu import ARG, BAD_OPTS, GOOD_OPTS, _opts


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_exports(lib):
    from show_edit_tell_amd import _lib
    for name in ("set_sample_pick_opts_key_f32", "set_sample_logp_bwd_opts_f32"):
        assert name not in _lib.MISSING and getattr(lib, name).restype is C.c_int, name


def test_refusals_come_before_any_hip_call(lib):
    """(No call here is one that would be accepted: with these host pointers it would go on to a launch.)"""
    import test_pick_abi_cpu as PA
    bufs = PA.Bufs()
    p = bufs.p
    key = p["emb_out"]

    def pick(o, logits=p["logits"], seq=p["seq"], ld=PA.LD, kept=key):
        return lib.set_sample_pick_opts_key_f32(logits, ld, PA.B, PA.V, 1, PA.MAXLEN, PA.V - 1, 1, 2, seq, p["it"], p["unfinished"],
                                                p["alive"], p["raw_ids"], p["lse"], p["step_logp"], None,
                                                C.byref(_opts(o)) if o is not None else None, kept)

    def bwd(o, logits=p["logits"], lse=p["lse"], raw=p["raw_ids"], kept=key, g=p["step_logp"], d=p["table"], ld=PA.LD, ldd=PA.LD,
            rows=PA.B, V=PA.V):
        return lib.set_sample_logp_bwd_opts_f32(logits, ld, lse, raw, kept, g, d, ldd, rows, V,
                                                C.byref(_opts(o)) if o is not None else None, None)

    for o in BAD_OPTS:
        assert pick(o) == ARG and pick(o, kept=None) == ARG and bwd(o) == ARG and bwd(o, kept=None) == ARG, o
        assert bufs.untouched(), o
    # the other checks of the calls answer too, with options that are in range, neutral or NULL
    for o in GOOD_OPTS + [None]:
        assert pick(o, logits=None) == ARG and pick(o, seq=None) == ARG and pick(o, ld=PA.V - 1) == ARG, o
        for kw in (dict(logits=None), dict(lse=None), dict(raw=None), dict(g=None), dict(d=None), dict(rows=0), dict(V=0),
                   dict(ld=PA.V - 1), dict(ldd=PA.V - 1)):
            assert bwd(o, **kw) == ARG, (o, kw)
    assert bufs.untouched()


def test_refuse_sample_opts_is_unchanged():
    from show_edit_tell_amd import _lib as L
    for args in ((True, True, False), (True, False, False), (False, False, False), (False, True, True)):
        with pytest.raises(ValueError):
            L.refuse_sample_opts(*args)
    L.refuse_sample_opts(False, True, False)


@pytest.mark.parametrize("V,ld", FX.SHAPES)
@pytest.mark.parametrize("R", FX.ROWS)
def test_fixture_rows_keep_clear_of_the_boundaries(V, ld, R):
    x = FX.rows(V, R)
    assert len({row.tobytes() for row in x}) == R
    for opts in FX.OPTS:
        assert np.abs(TS.scaled(x, opts[0])).max() <= FX.Y_MAX
        dist, gap = FX.margins(x, opts)
        assert dist >= TS.BOUNDARY_MIN, (V, R, opts, "top-p target %.2e from a group boundary" % dist)
        assert gap > FX.K_MARGIN, (V, R, opts, "a word %.2e from the top-k boundary value" % gap)


@pytest.mark.parametrize("path", sorted(TS.SPECIAL))
def test_special_rows_keep_clear_of_the_boundaries(path):
    V, ld, words = TS.SPECIAL[path]
    x = TS.special_rows(V, words)
    for opts in TS.SPECIAL_OPTS:
        dist, gap = FX.margins(x, opts)
        assert dist >= TS.BOUNDARY_MIN and gap > FX.K_MARGIN, (path, opts, dist, gap)


def test_order_key_orders_floats():
    v = np.array([-np.inf, -30.0, -1e-30, -0.0, 0.0, 1e-30, 2.5, 30.0, np.inf], np.float32)
    k = FX.order_key(v).astype(np.int64)
    assert k[3] == k[4] and (np.diff(k[[0, 1, 2, 3, 5, 6, 7, 8]]) > 0).all()
