"""The C ABI of the truncated stochastic beam search picks without a device (include/set_hip.h set_sbs_pick_opts_f32,
set_sbs_pick_ensemble_opts_f32): declared, bound and exported; every refusal is answered before any HIP call with nothing
written; the Python functions refuse the same options before anything runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("set_sbs_pick_opts_f32", "set_sbs_pick_ensemble_opts_f32")


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from show_edit_tell_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "set_hip.h")).read()
    assert re.search(r"\bint set_sbs_pick_opts_f32\s*\(const SetSbsArgs\*[^,]*,\s*const SetSampleOpts\*[^,]*,\s*void\*", header)
    assert re.search(r"\bint set_sbs_pick_ensemble_opts_f32\s*\(const SetSbsArgs\*[^,]*,\s*const float\*[^,]*,\s*const SetSampleOpts\*"
                     r"[^,]*,\s*void\*", header)
    for name in NAMES:
        assert name in L.PROTOTYPES and name not in L.MISSING and hasattr(lib, name), name
    assert C.sizeof(L.SbsArgs) == 16 * 8 + 6 * 4         # the workspace query and the argument struct are unchanged


def test_refusals_without_a_device(lib):
    """host memory stands in for the device buffers: a call that got as far as a launch would fail differently (and none does)"""
    from show_edit_tell_amd._lib import SampleOpts, SbsArgs
    block = np.full(1 << 16, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 256
    NI, k, V = 2, 3, 50

    def call(ens, opts=None, logits2=base + 2048, null_args=False, **over):
        a = SbsArgs(logits=base, ld=52, end_idx=3, seed=1, offset=2, phi=base + 4096, G=base + 4352, finished=base + 4608,
                    len=base + 4864, seqs_in=base + 5120, seqs_out=base + 6144, words=base + 7168, rows=base + 7424,
                    n_open=base + 7680, ws=base + 8192, ws_bytes=lib.set_sbs_workspace_bytes(NI, k), NI=NI, k=k, V=V, t=0, Lmax=4)
        for key, val in over.items():
            setattr(a, key, val)
        ap, op = (None if null_args else C.byref(a)), (C.byref(opts) if opts is not None else None)
        if ens:
            return lib.set_sbs_pick_ensemble_opts_f32(ap, logits2, op, None)
        return lib.set_sbs_pick_opts_f32(ap, op, None)

    good = dict(temperature=1.0, top_k=5, top_p=0.9)
    for ens in (False, True):
        for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(top_p=float("inf")),
                    dict(temperature=0.0), dict(temperature=float("nan")), dict(temperature=1e4)):
            assert call(ens, SampleOpts(**(good | bad))) == ARG, (ens, bad)
        assert call(ens, SampleOpts(**good), null_args=True) == ARG
        assert call(ens, None, null_args=True) == ARG
        assert call(ens, SampleOpts(**good), t=255) == ARG       # (good options do not lift the refusals of the untruncated entry)
        for field in ("logits", "phi", "G", "finished", "len", "seqs_in", "seqs_out", "words", "rows", "n_open", "ws"):
            assert call(ens, SampleOpts(**good), **{field: None}) == ARG, field
        for over in (dict(k=0), dict(k=9), dict(t=-1), dict(V=0), dict(ld=V - 1), dict(NI=0), dict(Lmax=0), dict(ws_bytes=8),
                     dict(ws=base + 8196), dict(end_idx=-1), dict(end_idx=V), dict(seqs_out=base + 5120),
                     dict(V=(1 << 26) - 3, ld=1 << 26)):
            assert call(ens, SampleOpts(**good), **over) == ARG, over
    assert call(True, SampleOpts(**good), logits2=None) == ARG
    assert call(True, None, logits2=None) == ARG
    assert (block == 0xA5).all()


def test_python_entries_refuse_bad_options_before_anything_runs():
    from show_edit_tell_amd import evaluate

    class Edit:
        _ABI, _adaptive, vocab_size = "editnet", 0, 50

    class Dc:
        _ABI, vocab_size = "dcnet", 50

    wm = {"<start>": 1, "<end>": 2, "<pad>": 0}
    calls = ((evaluate.sample_captions_distinct, (Edit(), None, None, None, wm)),
             (evaluate.sample_captions_distinct, (Dc(), None, None, wm)),
             (evaluate.sample_captions_distinct_ensemble, (Edit(), Dc(), None, None, None, wm)))
    for fn, args in calls:
        for bad in (dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                    dict(temperature=0.0), dict(temperature=float("nan")), dict(top_k=5, temperature=0.0)):
            with pytest.raises(ValueError, match="top_k|top_p|temperature"):
                fn(*args, **bad)
