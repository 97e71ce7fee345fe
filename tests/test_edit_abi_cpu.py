"""CPU: the device edit-distance route (csrc/editdist_device.hip, editdist.DeviceEditDistance) as far as it goes without a GPU:
both entry points are exported and prototyped, and refuse bad arguments before any HIP call."""
import ctypes as C
import os
import re

import pytest

SET_OK, SET_ERR_ARG, SET_ERR_UNSUPPORTED = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("set_edit_device_score", "set_edit_device_align")


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_exports_and_prototypes(lib):
    from show_edit_tell_amd import _lib
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "set_hip.h")).read())
    for name in NAMES:
        assert name in _lib.PROTOTYPES and name not in _lib.MISSING and hasattr(lib, name)
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == len(_lib.PROTOTYPES[name][1])
    # the parameters of set_rouge_device_score under the same names, without beta
    params = lambda name: [p.strip() for p in re.search(r"int %s\(([^)]*)\);" % name, header).group(1).split(",")]
    assert params("set_edit_device_score") == [p for p in params("set_rouge_device_score") if p != "double beta"]
    assert lib.set_abi_version() == 1


def test_score_validation(lib):
    one = C.c_void_p(16)                                      # never dereferenced: every refusal comes first

    def score(hyp=one, ld=20, n_hyp=2, L=20, set_of=one, recs=one, ref_L=20, n_refs=5, off=one, n_sets=1, max_set=5, stats=one,
              scores=None, pairs=None, pair_ld=0):
        return lib.set_edit_device_score(hyp, ld, None, n_hyp, L, set_of, recs, ref_L, n_refs, off, n_sets, max_set, stats, scores,
                                         pairs, pair_ld, None)
    assert score(L=65, ld=65) == SET_ERR_UNSUPPORTED
    assert score(ref_L=65) == SET_ERR_UNSUPPORTED
    assert score(pairs=one, pair_ld=4) == SET_ERR_ARG                                 # pair_ld below the largest set
    for kw in (dict(hyp=None), dict(set_of=None), dict(recs=None), dict(off=None), dict(stats=None), dict(n_hyp=-1),
               dict(n_sets=-1), dict(n_refs=-1), dict(max_set=-1), dict(L=0), dict(ref_L=0), dict(ld=19)):
        assert score(**kw) == SET_ERR_ARG, kw
    # a bad argument wins over an unsupported length
    assert score(L=65, ld=65, stats=None) == SET_ERR_ARG and score(ref_L=65, set_of=None) == SET_ERR_ARG
    assert score(L=65, ld=65, off=None) == SET_ERR_ARG
    assert score(n_hyp=0, hyp=None, set_of=None, stats=None) == SET_OK                # no hypothesis: a successful no-op


def test_align_validation(lib):
    one = C.c_void_p(16)

    def align(hyp=one, hyp_ld=20, n=2, L=20, src=one, src_ld=30, src_L=30, stats=one, hyp_ops=one, ops_ld=20, hyp_src=one,
              src_ops=one, src_ops_ld=30):
        return lib.set_edit_device_align(hyp, hyp_ld, None, n, L, src, src_ld, None, src_L, stats, hyp_ops, ops_ld, hyp_src, src_ops,
                                         src_ops_ld, None)
    assert align(L=65, hyp_ld=65, ops_ld=65) == SET_ERR_UNSUPPORTED
    assert align(src_L=65, src_ld=65, src_ops_ld=65) == SET_ERR_UNSUPPORTED
    for kw in (dict(hyp=None), dict(src=None), dict(stats=None), dict(hyp_ops=None), dict(hyp_src=None), dict(src_ops=None),
               dict(n=-1), dict(L=0), dict(src_L=0), dict(hyp_ld=19), dict(src_ld=29), dict(ops_ld=19), dict(src_ops_ld=29)):
        assert align(**kw) == SET_ERR_ARG, kw
    # a bad argument wins over an unsupported length
    assert align(L=65, hyp_ld=65, ops_ld=65, stats=None) == SET_ERR_ARG
    assert align(src_L=65, src_ld=65, src_ops_ld=65, hyp_ld=19) == SET_ERR_ARG
    assert align(L=65, hyp_ld=65, ops_ld=64) == SET_ERR_ARG
    assert align(n=0, hyp=None, src=None, stats=None, hyp_ops=None, hyp_src=None, src_ops=None) == SET_OK      # a no-op


def test_device_scorer_refuses_cpu():
    from show_edit_tell_amd import editdist
    from show_edit_tell_amd._lib import SetError
    for make in (editdist.DeviceEditDistance, editdist.device_scorer):
        with pytest.raises(SetError) as e:
            make("cpu")
        assert str(e.value) == "the device edit distance scorer needs a GPU device, got cpu"
