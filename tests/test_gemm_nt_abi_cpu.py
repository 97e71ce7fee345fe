"""CPU: set_gemm_nt_group_f32 / set_gemm_nt_group_workspace_bytes (include/set_hip.h) answer every malformed call with the
library's codes before any HIP call.  The operand pointers below are dummies (16-byte-aligned small integers) or NULL: a
call that got as far as a launch, or dereferenced one, would crash this process instead of returning a code."""
import ctypes as C

import pytest

ARG, UNSUPPORTED, WORKSPACE = 1, 2, 4
P = 4096            # a 16-byte aligned, never dereferenced "device pointer"


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def prob(M=64, N=64, Ks=(64,), ksplit=1, act=0, bias=None, A=P, W=P, Cp=P, lda=None, ldw=None, ldc=None, nseg=None):
    from show_edit_tell_amd._lib import GemmNtProb, GemmNtSeg
    d = GemmNtProb()
    for s, K in enumerate(Ks[:3]):
        d.seg[s] = GemmNtSeg(A, K if lda is None else lda, W, K if ldw is None else ldw, K, 0)
    d.C, d.ldc, d.bias = Cp, (N if ldc is None else ldc), bias
    d.nseg, d.M, d.N, d.act, d.ksplit = (len(Ks) if nseg is None else nseg), M, N, act, ksplit
    return d


def call(lib, probs, n=None, ws=None, ws_bytes=0, **launch):
    from show_edit_tell_amd._lib import GemmNtLaunch, GemmNtProb
    arr = (GemmNtProb * max(len(probs), 1))(*probs)
    l = GemmNtLaunch(**launch)
    return lib.set_gemm_nt_group_f32(arr, len(probs) if n is None else n, C.byref(l), ws, ws_bytes, None)


def test_struct_layout_matches_the_header(lib):
    """sizes the C compiler gives the three structs of the header (8-byte pointers, no implicit padding)"""
    from show_edit_tell_amd._lib import GemmNtLaunch, GemmNtProb, GemmNtSeg
    assert C.sizeof(GemmNtSeg) == 40
    assert C.sizeof(GemmNtProb) == 3 * 40 + 24 + 24
    assert C.sizeof(GemmNtLaunch) == 5 * 8 + 8
    assert GemmNtProb.C.offset == 120 and GemmNtProb.nseg.offset == 144 and GemmNtLaunch.bm_hint.offset == 40


def test_null_and_count(lib):
    assert lib.set_gemm_nt_group_f32(None, 1, None, None, 0, None) == ARG
    assert call(lib, [prob()] * 7) == ARG                                   # n > GEMM_MAX_TASKS
    assert call(lib, [prob()], n=-1) == ARG
    assert call(lib, [prob(A=None)]) == ARG
    assert call(lib, [prob(W=None)]) == ARG
    assert call(lib, [prob(Cp=None)]) == ARG
    assert call(lib, [prob(), prob(Ks=(32, 32), A=None)]) == ARG            # a later problem, a later segment
    assert call(lib, [prob(M=0)]) == ARG and call(lib, [prob(N=0)]) == ARG
    assert call(lib, [prob(act=4)]) == ARG and call(lib, [prob(ksplit=-1)]) == ARG
    assert lib.set_gemm_nt_group_f32(None, 0, None, None, 0, None) == ARG


def test_segments_and_contraction_length(lib):
    assert call(lib, [prob(Ks=(32, 32, 32), nseg=4)]) == ARG                # nseg > 3
    assert call(lib, [prob(nseg=0)]) == ARG
    assert call(lib, [prob(Ks=(48,))]) == UNSUPPORTED                       # K % 32
    assert call(lib, [prob(Ks=(64, 16))]) == UNSUPPORTED
    assert call(lib, [prob(Ks=(0,))]) == ARG


def test_alignment_and_leading_dimensions(lib):
    assert call(lib, [prob(A=P + 4)]) == ARG
    assert call(lib, [prob(W=P + 8)]) == ARG
    assert call(lib, [prob(lda=66)]) == ARG and call(lib, [prob(ldw=65)]) == ARG      # not multiples of 4 floats
    assert call(lib, [prob(lda=32)]) == ARG and call(lib, [prob(ldw=60)]) == ARG      # shorter than K
    assert call(lib, [prob(ldc=63)]) == ARG                                           # shorter than N


def test_launch_fields(lib):
    assert call(lib, [prob()], bm_hint=32) == ARG
    assert call(lib, [prob()], flags=4) == ARG
    assert call(lib, [prob()], row_list=P) == ARG                           # list without count
    assert call(lib, [prob()], row_count=P) == ARG
    assert call(lib, [prob()], row_list=P, row_count=P, alive=P) == ARG     # one gate per launch


def test_workspace(lib):
    from show_edit_tell_amd._lib import GemmNtProb
    p = prob(M=65, N=130, Ks=(96, 32), ksplit=3)
    need = lib.set_gemm_nt_group_workspace_bytes((GemmNtProb * 1)(p), 1)
    assert need >= 3 * 65 * 130 * 4
    assert lib.set_gemm_nt_group_workspace_bytes((GemmNtProb * 1)(prob(ksplit=1)), 1) == 0      # never split: none
    assert lib.set_gemm_nt_group_workspace_bytes((GemmNtProb * 1)(prob(Ks=(48,))), 1) == 0
    assert lib.set_gemm_nt_group_workspace_bytes(None, 1) == 0
    assert call(lib, [p]) == WORKSPACE                                      # no workspace at all
    assert call(lib, [p], ws=P, ws_bytes=3 * 65 * 130 * 4 - 4) == WORKSPACE
    assert call(lib, [p], ws=P + 4, ws_bytes=need) == WORKSPACE             # misaligned
    assert call(lib, [prob(), p], ws=P, ws_bytes=1024) == WORKSPACE         # mixed launch: the split problem still counts
    # the planner's own split (ksplit = 0) is bounded by the query as well
    q = prob(M=64, N=4096, Ks=(288,), ksplit=0)
    assert lib.set_gemm_nt_group_workspace_bytes((GemmNtProb * 1)(q), 1) >= 8 * 64 * 4096 * 4


def test_gates_refuse_split_problems(lib):
    big = 1 << 30
    p = prob(M=64, Ks=(96,), ksplit=2)
    assert call(lib, [p], ws=P, ws_bytes=big, row_list=P, row_count=P) == ARG
    assert call(lib, [prob(), p], ws=P, ws_bytes=big, row_list=P, row_count=P) == ARG
    assert call(lib, [p], ws=P, ws_bytes=big, alive=P) == ARG               # the reduction launch carries no gate
    # partials kept: the launcher itself refuses a split problem with an activation; a bias would be dropped
    assert call(lib, [prob(Ks=(96,), ksplit=2, act=2)], ws=P, ws_bytes=big, flags=2) == ARG
    assert call(lib, [prob(Ks=(96,), ksplit=2, bias=P)], ws=P, ws_bytes=big, flags=2) == ARG


def test_row_list_on_the_16_row_class(lib):
    assert call(lib, [prob(M=16)], row_list=P, row_count=P) == UNSUPPORTED
    assert call(lib, [prob(M=5), prob(M=16, N=130)], row_list=P, row_count=P) == UNSUPPORTED
