"""GPU: beam search over ADAPTIVE features (zero-padded regions, an image mean per image) against the reference's own
adaptive evaluate() loop (tests/golden/beam_adaptive_*.npz, `adaptive_features/editnet_adaptive.py:614-735`, written by
tools/make_adaptive_beam_golden.py):
  * beam_search_adaptive_batched: many images at once on the per-step fused kernels;
  * beam_search_adaptive: one image per call, the persistent launch in beam mode over up to 128 masked regions (k <= 4),
    otherwise the NI = 1 case of the batched search."""
import numpy as np
import pytest

import beam_parity
from hip_adapter import load_numpy_state, to_dev
from oracle import cases

pytestmark = pytest.mark.gpu

GOLDENS = {"beam_adaptive_small": "editnet_adaptive_small", "beam_adaptive_full_b4": "editnet_adaptive_full_b4"}


def _model_name(boost):
    return "adaptive_e%d" % int(round(float(boost) * 10))


def _decoder(d, boost):
    from show_edit_tell_amd import editnet_adaptive
    c, wm = d["case"], d["wm"]
    sd = {k: v.copy() for k, v in d["sd"].items()}
    sd["fc.bias"][wm["<end>"]] += np.float32(boost)
    return load_numpy_state(editnet_adaptive.DecoderC(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), sd)


def _inputs(d):
    return to_dev(d["X"]), to_dev(d["image_mean"]), to_dev(d["prev"]), to_dev(d["plen"])


def _persistent_tags(fn):
    import torch
    from show_edit_tell_amd import _lib
    lib = _lib.load()
    lib.set_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        tags = [r["tag"] for r in _lib.profile_report()]
    finally:
        lib.set_profile_enable(0)
    return out, tags


def _same_search(seq, sc, bseq, bsc, margin=np.inf):
    """One-image result against the batched search of the same image: same tokens (but for a near-tie between the two
    best completed hypotheses), score within SCORE_TOL; a step-limit run: length 18 and the same first 4 tokens."""
    if np.isnan(bsc):
        assert np.isnan(sc) and len(seq) == 18 and seq[:4] == bseq[:4], (seq, bseq)
        return
    assert abs(sc - bsc) < beam_parity.SCORE_TOL, (sc, bsc)
    assert seq == bseq or margin <= beam_parity.MARGIN_MIN, (seq, bseq)


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_batched_adaptive_beam_vs_reference_beam(name):
    """All images of the case at once, every beam size and boost of the golden == the reference's adaptive loop."""
    from show_edit_tell_amd import evaluate
    d = cases.build_editnet(GOLDENS[name])
    g = beam_parity.load(name)
    wm, B = d["wm"], d["case"]["B"]
    X, mean, prev, plen = _inputs(d)
    firm = want = 0
    for boost in g["boosts"]:
        dec, model = _decoder(d, boost), _model_name(boost)
        for k in g["beams"]:
            k = int(k)
            seqs, scores = evaluate.beam_search_adaptive_batched(dec, X, mean, prev, plen, wm, k, return_scores=True)
            assert len(seqs) == B
            for b in range(B):
                firm += beam_parity.check_one(g, k, model, b, seqs[b], scores[b])
            pre = "k%d.%s." % (k, model)
            want += int(((~g[pre + "infinite"]) & (g[pre + "margin"] > beam_parity.MARGIN_MIN)).sum())
    assert want >= 1 and firm >= want, (firm, want)


def test_per_image_persistent_adaptive_beam_vs_reference_beam():
    """The reference's calling convention at full dimensions, R = 100 with 10 / 37 / 100 valid regions forced, k = 1 .. 4:
    one persistent launch per search (profile tag), tokens as the reference's loop and the batched search, scores within
    SCORE_TOL."""
    from show_edit_tell_amd import evaluate
    name = "beam_adaptive_full_b4"
    d = cases.build_editnet(GOLDENS[name])
    g = beam_parity.load(name)
    wm, B = d["wm"], d["case"]["B"]
    assert {10, 37, 100} <= set(int(n) for n in d["nvalid"])
    X, mean, prev, plen = _inputs(d)
    firm = used = want = 0
    for boost in g["boosts"]:
        dec, model = _decoder(d, boost), _model_name(boost)
        for k in (1, 2, 3, 4):
            bseqs, bscores = evaluate.beam_search_adaptive_batched(dec, X, mean, prev, plen, wm, k, return_scores=True)
            for b in range(B):
                one = (X[b:b + 1], mean[b:b + 1], prev[b:b + 1], plen[b:b + 1])
                evaluate.beam_search_adaptive(dec, *one, wm, k)              # (the token table is built on the second call)
                (seq, sc), tags = _persistent_tags(lambda: evaluate.beam_search_adaptive(dec, *one, wm, k))
                assert "persistent_beam" in tags, tags
                used += 1
                firm += beam_parity.check_one(g, k, model, b, seq, sc)
                _same_search(seq, sc, bseqs[b], bscores[b], float(g["k%d.%s.margin" % (k, model)][b]))
            pre = "k%d.%s." % (k, model)
            want += int(((~g[pre + "infinite"]) & (g[pre + "margin"] > beam_parity.MARGIN_MIN)).sum())
    assert used == 2 * 4 * B and want >= 1 and firm >= want, (used, firm, want)


@pytest.mark.parametrize("boost", [1.0, 2.5])
def test_per_image_persistent_adaptive_beam_vs_batched_long_searches(boost):
    """Smaller <end> boosts: searches of many picks in which k shrinks inside the launch, or that run into the 50-step
    limit — the persistent launch against the batched per-step search (itself pinned to the reference above)."""
    from show_edit_tell_amd import evaluate
    d = cases.build_editnet("editnet_adaptive_full_b4")
    wm, B = d["wm"], d["case"]["B"]
    dec = _decoder(d, boost)
    X, mean, prev, plen = _inputs(d)
    same = total = 0
    lens = []
    for k in (3, 4):
        bseqs, bscores = evaluate.beam_search_adaptive_batched(dec, X, mean, prev, plen, wm, k, return_scores=True)
        for b in range(B):
            one = (X[b:b + 1], prev[b:b + 1], plen[b:b + 1])
            evaluate.beam_search_adaptive(dec, X[b:b + 1], mean[b:b + 1], prev[b:b + 1], plen[b:b + 1], wm, k)
            got = evaluate._beam_search_editnet_persistent(dec, *one, wm, k, image_mean=mean[b:b + 1])
            assert got is not None, "the persistent beam launch must be taken at k <= 4 with the token table active"
            seq, sc = got
            lens.append(len(seq))
            total += 1
            if np.isnan(bscores[b]):
                _same_search(seq, sc, bseqs[b], bscores[b])
                same += 1
            else:
                assert abs(sc - bscores[b]) < beam_parity.SCORE_TOL, (k, b, sc, bscores[b])
                same += int(seq == bseqs[b])
    print("boost", boost, "caption lengths", lens)
    assert same >= total - 1, (same, total)          # (one near-tie between two completed hypotheses may swap)


def test_per_image_adaptive_fallbacks_match_batched_search():
    """Where the persistent launch answers UNSUPPORTED — k = 5, an odd region count — beam_search_adaptive is the NI = 1
    case of the batched search."""
    from show_edit_tell_amd import evaluate
    d = cases.build_editnet("editnet_adaptive_full_b4")
    wm = d["wm"]
    dec = _decoder(d, 3.5)
    X, mean, prev, plen = _inputs(d)
    # k = 5: more hypotheses than rows of the beam launch
    bseqs, bscores = evaluate.beam_search_adaptive_batched(dec, X, mean, prev, plen, wm, 5, return_scores=True)
    for b in range(d["case"]["B"]):
        one = (X[b:b + 1], mean[b:b + 1], prev[b:b + 1], plen[b:b + 1])
        assert evaluate._beam_search_editnet_persistent(dec, one[0], one[2], one[3], wm, 5, image_mean=one[1]) is None
        seq, sc = evaluate.beam_search_adaptive(dec, *one, wm, 5)
        _same_search(seq, sc, bseqs[b], bscores[b])
    # odd R: 99 slots (the dropped one is padding on the 10- and 37-region images)
    sel = [b for b in range(d["case"]["B"]) if int(d["nvalid"][b]) in (10, 37)]
    assert len(sel) == 2
    X99 = X[sel, :99].contiguous()
    for k in (3, 4):
        bseqs, bscores = evaluate.beam_search_adaptive_batched(dec, X99, mean[sel], prev[sel], plen[sel], wm, k, return_scores=True)
        for i, b in enumerate(sel):
            one = (X99[i:i + 1], mean[b:b + 1], prev[b:b + 1], plen[b:b + 1])
            evaluate.beam_search_adaptive(dec, *one, wm, k)
            assert evaluate._beam_search_editnet_persistent(dec, one[0], one[2], one[3], wm, k, image_mean=one[1]) is None
            seq, sc = evaluate.beam_search_adaptive(dec, *one, wm, k)
            _same_search(seq, sc, bseqs[i], bscores[i])


def test_adaptive_entry_points_refuse_bad_arguments():
    """A fixed-feature decoder is a TypeError (its entries are beam_search_editnet*); image_mean must be (NI, F)."""
    from show_edit_tell_amd import editnet, evaluate
    d = cases.build_editnet("editnet_adaptive_small")
    c, wm = d["case"], d["wm"]
    X, mean, prev, plen = _inputs(d)
    fixed = load_numpy_state(editnet.DecoderC(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), d["sd"])
    with pytest.raises(TypeError):
        evaluate.beam_search_adaptive_batched(fixed, X, mean, prev, plen, wm, 3)
    with pytest.raises(TypeError):
        evaluate.beam_search_adaptive(fixed, X[:1], mean[:1], prev[:1], plen[:1], wm, 3)
    dec = _decoder(d, 2.5)
    for bad in (mean[:, :-1], mean[:1], mean[0], None):
        with pytest.raises(ValueError):
            evaluate.beam_search_adaptive_batched(dec, X, bad, prev, plen, wm, 3)
    with pytest.raises(ValueError):
        evaluate.beam_search_adaptive(dec, X[:1], mean[:2], prev[:1], plen[:1], wm, 3)
