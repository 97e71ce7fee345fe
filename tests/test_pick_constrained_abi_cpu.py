"""CPU: every refusal of the constrained pick and decode entries (include/set_hip.h "Constrained greedy and sampled picks") is
SET_ERR_ARG, answered before any HIP call with nothing written — no device is needed.  (No call here is well formed throughout:
with these host pointers it would go on to a launch.)"""
import ctypes as C

import numpy as np
import pytest

import test_pick_abi_cpu as PA

ARG, WORKSPACE = 1, 4


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    assert _lib.load().set_error_string(ARG) and _lib.load().set_error_string(WORKSPACE)
    return _lib.load()


def _cons(L, keep, ngram=0, min_len=0, alpha=0.0, n_banned=0, banned="auto"):
    """a BeamConstraintsC over a host array of ids (kept alive in `keep`); banned: "auto" = non-NULL iff n_banned > 0"""
    ids = np.arange(64, dtype=np.int64)
    keep.append(ids)
    p = (ids.ctypes.data if n_banned > 0 else None) if banned == "auto" else banned
    return L.BeamConstraintsC(ngram, min_len, alpha, n_banned, p)


# (keyword arguments of _cons) the struct refusals of set_beam_pick_constrained_f32, then this feature's own
BAD = [dict(ngram=-1), dict(ngram=17), dict(min_len=-1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-1.0),
       dict(n_banned=-1), dict(n_banned=65), dict(n_banned=2, banned=None), dict(n_banned=0, banned=64),
       dict(alpha=0.5), dict(alpha=1e-30)]


def test_struct_layout():
    from show_edit_tell_amd._lib import BeamConstraintsC as S
    assert C.sizeof(S) == 24 and (S.no_repeat_ngram.offset, S.min_len.offset, S.length_alpha.offset, S.n_banned.offset,
                                  S.banned.offset) == (0, 4, 8, 12, 16)


def test_pick_entry_refusals(lib):
    from show_edit_tell_amd import _lib as L
    bufs, keep = PA.Bufs(), []
    p = bufs.p

    def call(c, mode=0, t=1, max_len=PA.MAXLEN, V=PA.V, opts=None, **kw):
        a = L.PickArgs(logits=p["logits"], ld=PA.LD, stride=PA.B * PA.LD, bias=p["bias"], end_idx=V - 1, seq=p["seq"],
                       seq_logp=p["seq_logp"], it=p["it"], unfinished=p["unfinished"], alive=p["alive"], seed=1, offset=2,
                       raw_ids=p["raw_ids"], lse=p["lse"], step_logp=p["step_logp"], n=2, B=PA.B, V=V, t=t, max_len=max_len,
                       D=PA.D, mode=mode)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.set_pick_slabs_constrained_f32(C.byref(a), C.byref(opts) if opts is not None else None,
                                                  C.byref(c) if c is not None else None, None)

    good = _cons(L, keep, 2, 1, 0.0, 2)
    for mode in (0, 1):
        assert call(None, mode) == ARG                                         # c == NULL
        for bad in BAD:
            assert call(_cons(L, keep, **bad), mode) == ARG, bad
        assert call(good, mode, max_len=256, V=4000) == ARG                    # the history lives in LDS
        assert call(_cons(L, keep, n_banned=5), mode) == ARG                   # V = 10 <= 5 + 1 + 4
        assert call(good, mode, V=7) == ARG                                    # V = 7 <= 2 + 1 + 4
        assert call(good, mode, t=PA.MAXLEN + 1) == ARG                        # the history is seq[:, :t]
        # what set_pick_slabs_opts_f32 refuses still answers
        assert call(good, mode, t=-1) == ARG and call(good, mode, logits=None) == ARG and call(good, mode, n=0) == ARG
        assert call(good, mode, opts=L.SampleOpts(temperature=0.0, top_k=0, top_p=1.0)) == ARG
    assert call(good, 0, opts=L.SampleOpts(temperature=0.5, top_k=0, top_p=1.0)) == ARG      # greedy: options must be neutral
    assert call(good, 2) == ARG
    assert lib.set_pick_slabs_constrained_f32(None, None, C.byref(good), None) == ARG
    assert bufs.untouched()


def test_decode_entry_refusals(lib):
    """well-formed dims and a workspace of 16 bytes: a refused struct is SET_ERR_ARG, an accepted one reaches the workspace check
    (SET_ERR_WORKSPACE) — so the refusal is the constraints'"""
    from show_edit_tell_amd import _lib as L
    keep = []
    block = np.full(4096, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 64
    ew, dw = L.EditNetWeights(), L.DcnetWeights()

    def dims(V=203, maxT=19):
        return (L.EditNetDims(B=2, T=9, R=7, F=128, D=64, A=32, V=V, maxT=maxT, adaptive=0),
                L.DcnetDims(B=2, T=9, D=64, A=32, C=32, E=64, V=V, maxT=maxT))

    def calls(c, max_len=18, V=203, maxT=19):
        ed, dd = dims(V, maxT)
        cp = C.byref(c) if c is not None else None
        out = (base + 1536, base + 2048, base + 2560, 16, None)
        return [lib.set_editnet_greedy_constrained(C.byref(ew), C.byref(ed), base, None, base + 512, base + 1024, 1, 2, max_len, *out, cp),
                lib.set_editnet_sample_constrained(C.byref(ew), C.byref(ed), base, None, base + 512, base + 1024, 1, 2, max_len, 5, 6,
                                                   *out, None, cp),
                lib.set_dcnet_greedy_constrained(C.byref(dw), C.byref(dd), base + 512, base + 1024, 1, 2, max_len, *out, cp),
                lib.set_dcnet_sample_constrained(C.byref(dw), C.byref(dd), base + 512, base + 1024, 1, 2, max_len, 5, 6, *out, None, cp)]

    assert calls(None) == [ARG] * 4
    for bad in BAD:
        assert calls(_cons(L, keep, **bad)) == [ARG] * 4, bad
    good = _cons(L, keep, 3, 4, 0.0, 2)
    assert calls(good, max_len=256, V=4000, maxT=300) == [ARG] * 4              # max_len > 255
    assert calls(good, V=21) == [ARG] * 4                                       # V = 21 <= 2 + 1 + 18
    assert calls(good, V=22) == [WORKSPACE] * 4
    assert calls(good) == [WORKSPACE] * 4 and calls(_cons(L, keep)) == [WORKSPACE] * 4
    bad_opts = L.SampleOpts(temperature=0.0, top_k=0, top_p=1.0)
    ed, dd = dims()
    assert lib.set_editnet_sample_constrained(C.byref(ew), C.byref(ed), base, None, base + 512, base + 1024, 1, 2, 18, 5, 6, base + 1536,
                                              base + 2048, base + 2560, 16, None, C.byref(bad_opts), C.byref(good)) == ARG
    assert (block == 0xA5).all()


def test_python_constraint_checks():
    from show_edit_tell_amd import _lib as L
    from show_edit_tell_amd.evaluate import BeamConstraints
    wm = {"<start>": 1, "<end>": 2, "<unk>": 3, "a": 4}
    assert L.decode_constraints(None, wm, 10, True, False, False, False) is None
    assert L.decode_constraints(BeamConstraints(), wm, 10, True, False, False, False) is None
    cons, ids = L.decode_constraints(BeamConstraints(no_repeat_ngram=3, min_length=4, banned_words=["<unk>", 7]), wm, 10, True, False,
                                     False, False)
    assert ids == [3, 7] and cons.no_repeat_ngram == 3
    active = BeamConstraints(no_repeat_ngram=2)
    for kw in (dict(grad_path=True), dict(gumbel=True), dict(sample_max=False, sample_rl=False)):
        args = dict(sample_max=True, sample_rl=False, grad_path=False, gumbel=False)
        args.update(kw)
        with pytest.raises(ValueError):
            L.decode_constraints(active, wm, 10, **args)
    for bad in (BeamConstraints(length_penalty=0.5), BeamConstraints(banned_words=["nope"]), BeamConstraints(banned_words=[10]),
                BeamConstraints(banned_words=["<end>"])):
        with pytest.raises(ValueError):
            L.decode_constraints(bad, wm, 10, True, False, False, False)
    with pytest.raises(TypeError):
        L.decode_constraints({"no_repeat_ngram": 2}, wm, 10, True, False, False, False)
    with pytest.raises(ValueError):
        L.refuse_constraints(active, "sample_rollout")
    L.refuse_constraints(None, "x")
    L.refuse_constraints(BeamConstraints(), "x")
