"""No GPU: the C ABI and the Python routing of DCNet's one-launch beam search (set_dcnet_beam_persistent,
evaluate._beam_search_dcnet_persistent).  The search itself: tests/test_hip_dcnet_beam.py."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_entry_point_is_exported_and_prototyped(lib):
    from show_edit_tell_amd import _lib
    assert "set_dcnet_beam_persistent" in _lib.PROTOTYPES
    assert "set_dcnet_beam_persistent" not in _lib.MISSING
    fn = lib.set_dcnet_beam_persistent
    assert fn.restype is C.c_int and len(fn.argtypes) == 15


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """SET_ERR_ARG = 1 for null pointers, max_picks < 1 and a start token outside the vocabulary; no device is needed."""
    from show_edit_tell_amd._lib import DcnetDims, DcnetWeights
    d = DcnetDims(B=3, T=18, D=1024, A=512, C=512, E=1024, V=10000, maxT=51)
    w = DcnetWeights()
    one = C.c_void_p(16)                      # (never dereferenced: the argument checks come first)
    call = lib.set_dcnet_beam_persistent
    assert call(None, C.byref(d), None, None, 0, 1, 51, None, None, None, None, None, None, 0, None) == 1
    assert call(C.byref(w), None, one, one, 0, 1, 51, one, one, one, one, one, one, 0, None) == 1
    assert call(C.byref(w), C.byref(d), one, one, 0, 1, 51, one, one, one, one, None, one, 0, None) == 1
    assert call(C.byref(w), C.byref(d), one, one, 0, 1, 0, one, one, one, one, one, one, 0, None) == 1
    assert call(C.byref(w), C.byref(d), one, one, 10000, 1, 51, one, one, one, one, one, one, 0, None) == 1
    # no token table: SET_ERR_UNSUPPORTED = 2, again before anything is touched
    assert call(C.byref(w), C.byref(d), one, one, 0, 1, 51, one, one, one, one, one, one, 0, None) == 2


def test_workspace_covers_the_candidate_words_only_up_to_four_rows(lib):
    """The exchange region grew by B x (D / 4) x 12 words of 8 bytes for B <= 4 (the beam candidates); the size reported for
    B = 5 is what the layout without them gives: every other term of the workspace is linear in B."""
    from show_edit_tell_amd._lib import DcnetDims
    n = {B: lib.set_dcnet_workspace_bytes(C.byref(DcnetDims(B=B, T=18, D=1024, A=512, C=512, E=1024, V=10000, maxT=19)))
         for B in (3, 4, 5, 6, 7)}
    assert all(v > 0 for v in n.values())
    per_row = 256 * 12 * 8
    slack = 64 * 256                          # the carver aligns every tensor
    assert abs((n[7] - n[6]) - (n[6] - n[5])) <= slack
    assert abs((n[4] - n[3]) - (n[6] - n[5]) - per_row) <= slack
    assert abs((n[5] - n[4]) - (n[6] - n[5]) + 4 * per_row) <= slack


def test_beam_search_dcnet_tries_the_persistent_launch_first(monkeypatch):
    from show_edit_tell_amd import evaluate
    assert callable(evaluate._beam_search_dcnet_persistent)
    calls = []

    def persistent(dae, prev, plen, wm, k, *a, **kw):
        calls.append(("persistent", k))
        return persistent.answer

    def batched(dae, prev, plen, wm, k=3, *a, **kw):
        calls.append(("batched", k))
        assert kw.get("return_scores")
        return [[7, 8, 9]], [-1.5]

    monkeypatch.setattr(evaluate, "_beam_search_dcnet_persistent", persistent)
    monkeypatch.setattr(evaluate, "beam_search_dcnet_batched", batched)
    persistent.answer = ([1, 2, 3], -0.25)
    assert evaluate.beam_search_dcnet(None, None, None, {}, 3) == ([1, 2, 3], -0.25)
    assert calls == [("persistent", 3)]
    del calls[:]
    persistent.answer = None                  # SET_ERR_UNSUPPORTED: the batched per-step search answers
    assert evaluate.beam_search_dcnet(None, None, None, {}, 5) == ([7, 8, 9], -1.5)
    assert calls == [("persistent", 5), ("batched", 5)]
