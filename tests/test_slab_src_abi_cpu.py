"""The C ABI of the split-K partial consumers without a device: the six *_src_f32 entry points and set_gemm_group_slabs_f32
are declared in include/set_hip.h, bound in _lib.py and exported, SetSlabSrc agrees field for field, and every refusal —
of the addend list (make_src_list) and of each entry point's own arguments — is answered before any HIP call.  Only calls
that are refused are made here: host memory stands in for the device buffers and is never touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ARG, UNSUPPORTED = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSUMERS = ("lstm_cell", "copy_gate", "lstm_gates", "select", "context_gate", "attention")
M, D, T, L, DV, A = 5, 8, 3, 7, 8, 4


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def mem():
    block = np.full(1 << 16, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 256
    yield base
    assert (block == 0xA5).all()


def test_symbols_and_struct(lib):
    from show_edit_tell_amd import _lib as LB
    header = open(os.path.join(ROOT, "include", "set_hip.h")).read()
    for name in ["set_%s_bwd_src_f32" % c for c in CONSUMERS] + ["set_gemm_group_slabs_f32"]:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in LB.PROTOTYPES and name not in LB.MISSING and hasattr(lib, name), name
    body = re.search(r"typedef struct SetSlabSrc \{(.*?)\} SetSlabSrc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for n in re.findall(r"\w+", body) if n not in ("float", "int32_t", "int64_t", "const")]
    assert names == [f for f, _ in LB.SlabSrc._fields_], names
    assert C.sizeof(LB.SlabSrc) == 8 + 8 + 8 + 4 + 4
    assert int(re.search(r"#define SET_MAX_SRC (\d+)", header).group(1)) == 4
    codes = dict(re.findall(r"#define (SET_ERR_\w+) (\d+)", header))
    assert int(codes["SET_ERR_ARG"]) == ARG and int(codes["SET_ERR_UNSUPPORTED"]) == UNSUPPORTED


def _call(lib, base, which, src, n, **o):
    """the entry point `which` with valid dummy arguments (every pointer non-null and 256-byte aligned) except for `o`"""
    p = lambda i: base + 4096 * (i + 1)
    g = lambda key, default: o.get(key, default)
    d = g("D", D)
    if which == "lstm_cell":
        return lib.set_lstm_cell_bwd_src_f32(src, n, p(0), p(1), p(2), p(3), p(4), p(5), M, d, None)
    if which == "copy_gate":
        return lib.set_copy_gate_bwd_src_f32(src, n, g("dh_drop", p(0)), g("ld_drop", d + 4), g("p", 0.5), 7, 9, p(1), p(2),
                                             g("ld_ogate", 4 * d), p(3), p(4), p(5), p(6), p(7), p(8), p(9), p(10), M, d, None)
    if which == "lstm_gates":
        return lib.set_lstm_gates_bwd_src_f32(g("base", p(0)), src, n, p(1), p(2), p(3), p(4), p(5), M, d, None)
    if which == "select":
        return lib.set_select_bwd_src_f32(g("base", p(0)), src, n, p(1), p(2), p(3), p(4), M, T, d, g("acc", 0), None)
    if which == "context_gate":
        return lib.set_context_gate_bwd_src_f32(g("base", None), src, n, p(1), p(2), p(3), p(4), p(5), p(6),
                                                g("ld_out", 3 * d), M, d, None)
    if which == "attention":
        a = g("A", A)
        return lib.set_attention_bwd_src_f32(g("base", None), src, n, p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8), p(9),
                                             p(10), M, g("L", L), g("Dv", g("D", DV)), a, g("tanh", 1), 0, g("ld_datt2", 2 * a), None)
    raise KeyError(which)


def _list(base, *entries):
    from show_edit_tell_amd._lib import SlabSrc
    arr = (SlabSrc * max(len(entries), 1))()
    for i, e in enumerate(entries):
        e = dict(dict(p=base + 32768, slab_stride=M * D, ld=D, nslab=2, rows=M), **e)
        arr[i] = SlabSrc(e["p"], e["slab_stride"], e["ld"], e["nslab"], e["rows"])
    return arr


@pytest.mark.parametrize("which", CONSUMERS)
def test_the_addend_list_is_validated_before_any_launch(lib, mem, which):
    call = lambda src, n, **o: _call(lib, mem, which, src, n, **o)
    ok = {}
    # the count and the list pointer
    assert call(_list(mem, ok), -1) == ARG
    assert call(_list(mem, ok, ok, ok, ok, ok), 5) == ARG
    assert call(None, 1) == ARG
    # an entry's counts
    assert call(_list(mem, dict(nslab=-1)), 1) == ARG
    assert call(_list(mem, dict(rows=-1)), 1) == ARG
    assert call(_list(mem, ok, ok, ok, dict(rows=-1)), 4) == ARG                   # (every entry is looked at, not the first)
    # an entry that has partials: pointer, alignment, row stride, slab stride
    for bad in (dict(p=None), dict(p=mem + 32768 + 4), dict(p=mem + 32768 + 8), dict(ld=D + 2), dict(ld=D + 1),
                dict(slab_stride=M * D + 2), dict(slab_stride=M * D + 1)):
        assert call(_list(mem, bad), 1) == UNSUPPORTED, bad
        assert call(_list(mem, ok, ok, bad), 3) == UNSUPPORTED, bad
    # an entry without partials is not refused for its pointer: the refusal that follows is the NEXT entry's
    empty = dict(nslab=0, p=None, ld=1, slab_stride=1)
    assert call(_list(mem, empty, dict(rows=-1)), 2) == ARG
    assert call(_list(mem, empty, dict(ld=D + 2)), 2) == UNSUPPORTED
    # ... and a refusal of the entry point's own arguments comes through a list of only such entries
    assert call(_list(mem, empty, empty, empty, empty), 4, D=6) == UNSUPPORTED


def test_each_entry_points_own_refusals(lib, mem):
    none = (None, 0)
    for which in CONSUMERS:
        assert _call(lib, mem, which, *none, D=6) == UNSUPPORTED, which                       # D % 4
        if which != "attention":                                                              # (its Dv may be anything % 4 == 0)
            assert _call(lib, mem, which, *none, D=0) == ARG, which
    cg = lambda **o: _call(lib, mem, "copy_gate", *none, **o)
    assert cg(ld_ogate=D - 4) == UNSUPPORTED and cg(ld_ogate=4 * D + 2) == UNSUPPORTED
    assert cg(dh_drop=mem + 4096 + 4) == UNSUPPORTED and cg(dh_drop=mem + 4096 + 8) == UNSUPPORTED
    assert cg(ld_drop=D - 4) == UNSUPPORTED and cg(ld_drop=D + 2) == UNSUPPORTED
    for p in (-0.25, 1.0, 1.5, float("nan"), float("inf")):
        assert cg(p=p) == ARG, p
    assert cg(dh_drop=None, p=1.0) == ARG                                                     # (also without a dropped addend)
    xg = lambda **o: _call(lib, mem, "context_gate", *none, **o)
    assert xg(ld_out=D - 4) == UNSUPPORTED and xg(ld_out=3 * D + 2) == UNSUPPORTED
    at = lambda **o: _call(lib, mem, "attention", *none, **o)
    assert at(L=257) == UNSUPPORTED and at(A=1028) == UNSUPPORTED and at(Dv=2052) == UNSUPPORTED
    assert at(A=6) == UNSUPPORTED and at(Dv=6) == UNSUPPORTED
    assert at(A=8, ld_datt2=4) == UNSUPPORTED and at(ld_datt2=2 * A + 2) == UNSUPPORTED                 # ld_datt2 < A, % 4
    for tanh in (0, 1):
        assert at(L=257, tanh=tanh) == UNSUPPORTED


def test_gemm_group_slabs_needs_its_output_array(lib, mem):
    from show_edit_tell_amd._lib import GemmDesc
    descs = (GemmDesc * 1)(GemmDesc(mem + 4096, 512, mem + 8192, 64, mem + 12288, 64, 5, 64, 512, 0))
    assert lib.set_gemm_group_slabs_f32(descs, 1, 0, 1, mem + 16384, 1 << 14, None, None) == ARG
