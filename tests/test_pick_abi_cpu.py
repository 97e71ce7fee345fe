"""CPU: set_pick_slabs_f32 (include/set_hip.h) answers every malformed call with the library's codes before any HIP call and
writes nothing.  Every pointer handed over is HOST memory filled with a pattern (16-byte aligned numpy buffers): a call that
got as far as a launch would fail with the HIP code instead, and one that wrote through a pointer would change the pattern."""
import ctypes as C

import numpy as np
import pytest

OK, ARG, UNSUPPORTED = 0, 1, 2
B, V, LD, D, TD, MAXLEN = 3, 10, 12, 8, 8, 4


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


class Bufs:
    """every operand of a call, each a 16-byte aligned view into one pattern-filled host block"""
    SIZES = dict(logits=2 * B * LD * 4, bias=V * 4, seq=B * MAXLEN * 8, seq_logp=B * MAXLEN * 4, it=B * 8, unfinished=B * 4,
                 alive=(MAXLEN + 2) * 4, table=V * D * 4, emb_out=B * D * 4, raw_ids=B * 8, lse=B * 4, step_logp=B * 4,
                 g0=2 * B * 4 * TD * 4, pre=B * 4 * TD * 4, tab=V * 4 * TD * 4, c=B * TD * 4, h=B * TD * 4)

    def __init__(self):
        total = sum((n + 63) // 64 * 64 for n in self.SIZES.values()) + 64
        self.block = np.full(total, 0xA5, np.uint8)
        at = (-self.block.ctypes.data) % 64
        self.p = {}
        for name, n in self.SIZES.items():
            self.p[name] = self.block.ctypes.data + at
            at += (n + 63) // 64 * 64

    def untouched(self):
        return bool((self.block == 0xA5).all())


def tail_of(bufs, **over):
    from show_edit_tell_amd._lib import PickTail
    p = bufs.p
    f = dict(g0=p["g0"], g0_stride=B * 4 * TD, g0_ld=4 * TD, pre=p["pre"], ldpre=4 * TD, tab=p["tab"], ld_tab=4 * TD,
             c_in=p["c"], c_out=p["c"], h_out=p["h"], g0_n=2, col0=0, nrows=V, D=TD)
    f.update(over)
    return PickTail(**f)


def call(lib, bufs, tail=None, **over):
    from show_edit_tell_amd._lib import PickArgs
    p = bufs.p
    f = dict(logits=p["logits"], ld=LD, stride=B * LD, bias=p["bias"], end_idx=V - 1, seq=p["seq"], seq_logp=p["seq_logp"],
             it=p["it"], unfinished=p["unfinished"], alive=p["alive"], table=p["table"], emb_out=p["emb_out"], seed=1, offset=2,
             raw_ids=p["raw_ids"], lse=p["lse"], step_logp=p["step_logp"], n=2, B=B, V=V, t=0, max_len=MAXLEN, D=D, mode=0)
    f.update(over)
    a = PickArgs(**f)
    if tail is not None:
        a.tail = C.pointer(tail)
    rc = lib.set_pick_slabs_f32(C.byref(a), None)
    assert bufs.untouched(), (over, "a refused call wrote through one of its pointers")
    return rc


def test_struct_layout_matches_the_header(lib):
    """sizes the C compiler gives the two structs of the header (8-byte pointers, no implicit padding)"""
    from show_edit_tell_amd._lib import PickArgs, PickTail
    assert C.sizeof(PickTail) == 10 * 8 + 4 * 4
    assert C.sizeof(PickArgs) == 18 * 8 + 8 * 4
    assert PickTail.g0_n.offset == 80 and PickArgs.tail.offset == 136 and PickArgs.n.offset == 144 and PickArgs.mode.offset == 168


def test_null_pointers_and_mode(lib):
    bufs = Bufs()
    assert lib.set_pick_slabs_f32(None, None) == ARG
    for name in ("logits", "seq", "it", "unfinished", "alive", "seq_logp"):
        assert call(lib, bufs, **{name: None}) == ARG, name
    for name in ("logits", "seq", "it", "unfinished", "alive"):
        assert call(lib, bufs, mode=1, **{name: None}) == ARG, name
    assert call(lib, bufs, mode=2) == ARG and call(lib, bufs, mode=-1) == ARG


def test_sizes(lib):
    bufs = Bufs()
    for name in ("B", "V", "n", "max_len"):
        assert call(lib, bufs, **{name: 0}) == ARG, name
        assert call(lib, bufs, **{name: -1}) == ARG, name
    assert call(lib, bufs, t=-1) == ARG
    assert call(lib, bufs, ld=V - 1) == ARG and call(lib, bufs, mode=1, ld=V - 1) == ARG
    assert call(lib, bufs, D=6) == UNSUPPORTED and call(lib, bufs, mode=1, D=6) == UNSUPPORTED


@pytest.mark.parametrize("mode", [0, 1])
def test_tail_descriptor(lib, mode):
    """what tail_ok refuses comes back as greedy_pick / sample_pick return it"""
    bufs = Bufs()
    bad = [dict(D=0), dict(D=6), dict(g0=None), dict(g0_n=0), dict(g0_ld=4 * TD + 2), dict(g0_stride=B * 4 * TD + 1),
           dict(g0=bufs.p["g0"] + 4), dict(tab=None), dict(ld_tab=4 * TD + 3), dict(col0=2), dict(tab=bufs.p["tab"] + 8),
           dict(nrows=0), dict(c_in=None), dict(c_out=None), dict(h_out=None), dict(c_in=bufs.p["c"] + 4),
           dict(c_out=bufs.p["c"] + 4), dict(h_out=bufs.p["h"] + 12), dict(pre=bufs.p["pre"] + 4), dict(ldpre=4 * TD + 1)]
    for over in bad:
        assert call(lib, bufs, tail=tail_of(bufs, **over), mode=mode) == ARG, over
    # the checks of the call itself come first, with a well-formed tail too
    assert call(lib, bufs, tail=tail_of(bufs), mode=mode, ld=V - 1) == ARG
    assert call(lib, bufs, tail=tail_of(bufs), mode=mode, D=2) == UNSUPPORTED
