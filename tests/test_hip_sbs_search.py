"""GPU: evaluate.sample_captions_distinct — stochastic beam search through the fused per-step route — on the gumbel_fixtures
models (`editnet_full_b4`, `dcnet_full_b4`, <end> boosted, max_steps 6): the float64 oracle's search (tests/sbs_oracle.py) on the
route's own per-step logits returns the same sequences in the same order; reproducibility; no trace left on the other entry
points; the refusals.  Tolerance and gap: tests/sbs_fixtures.py."""
import numpy as np
import pytest
import torch

import dcnet_gumbel_fixtures as DF
import gumbel_fixtures as GF
import gumbel_oracle as GO
import sbs_fixtures as F
import sbs_oracle as SO
from hip_adapter import adaptive_module, dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
_CACHE = {}


def _model(kind):
    """(word_map, model, inputs of two images): built once per kind, <end> boosted, the token table settled"""
    if kind not in _CACHE:
        if kind == "editnet":
            d, _, rl = editnet_modules(GF.CASE)
            prev, plen, X = (to_dev(a[:2]) for a in GF.inputs(5))
            inputs = (X, prev, plen)
        else:
            d, _, rl = dcnet_modules(DF.CASE)
            inputs = tuple(to_dev(a[:2]) for a in DF.inputs(4))
        with torch.no_grad():
            for _ in range(3):
                rl(d["wm"], inputs[-2], inputs[-1], *inputs[:-2], True, False)
        _CACHE[kind] = (d["wm"], rl, inputs)
        _CACHE[kind, "bias"] = rl.fc.bias.detach().clone()
    return _CACHE[kind]


def _boost(kind, temperature):
    """fc.bias[<end>] = its own value + SEARCH_END_BOOST[temperature]"""
    wm, rl, _ = _model(kind)
    with torch.no_grad():
        rl.fc.bias.copy_(_CACHE[kind, "bias"])
        rl.fc.bias[int(wm["<end>"])] += F.SEARCH_END_BOOST[temperature]


def _call(kind, NI, n, seed, temperature=1.0, **kw):
    from show_edit_tell_amd import evaluate
    wm, rl, inputs = _model(kind)
    _boost(kind, temperature)
    torch.manual_seed(seed)
    return evaluate.sample_captions_distinct(rl, *(a[:NI] for a in inputs), wm, n_samples=n, temperature=temperature,
                                             max_steps=F.SEARCH_MAX_STEPS, **kw)


def _seed_of(seed):
    from show_edit_tell_amd import rng
    torch.manual_seed(seed)
    return rng.next_seed()


def _path_logp(infos, i, s):
    """the sum of the oracle's per-step log-probs along the ancestry of final slot s of image i"""
    total = 0.0
    for step in reversed(infos):
        total += step[i]["step_logp"][s]
        s = step[i]["parents"][s]
    return total


# ------------------------------------------------------------------------------------------- 1, 2. against the oracle's search
@pytest.mark.parametrize("kind,n,NI", sorted(F.SEARCH_SEED))
def test_search_matches_the_oracle_on_the_routes_own_logits(kind, n, NI):
    wm, _, _ = _model(kind)
    end, T, seed = int(wm["<end>"]), F.SEARCH_TEMPERATURE[(kind, n, NI)], F.SEARCH_SEED[(kind, n, NI)]
    out, steps = _call(kind, NI, n, seed, T, _return_steps=True)
    L = [s.cpu().numpy() for s in steps]
    states, infos = SO.search(lambda t, st: L[t], NI, n, len(L), _seed_of(seed), F.OFFSET, end, F.inv_t(T))
    want = SO.results(states, end, F.SEARCH_MAX_STEPS)
    picks = either = 0
    for i in range(NI):
        margins = [SO.margin(step[i]) for step in infos if not step[i].get("noop")]
        picks += n * len(margins)
        print(kind, n, "image", i, "smallest margin %.4f" % min(margins), [(e[0], round(e[1], 3), e[3]) for e in out[i]])
        got_seqs = [e[0] for e in out[i]]
        assert len(set(map(tuple, got_seqs))) == len(got_seqs) == n                   # pairwise distinct, a full beam
        assert all(a[2] >= b[2] for a, b in zip(out[i], out[i][1:]))                  # draw order: G non-increasing
        if got_seqs != [e[0] for e in want[i]]:
            near = sum(1 for m in margins if m < F.GAP)
            assert near > 0, (i, got_seqs, [e[0] for e in want[i]])                   # only a near tie may go either way
            either += n * near
            continue
        for s, (g, w) in enumerate(zip(out[i], want[i])):
            assert g[3] == w[3] and abs(g[1] - w[1]) <= F.TOL and abs(g[2] - w[2]) <= F.TOL, (i, s, g, w)
            assert abs(g[1] - _path_logp(infos, i, s)) <= F.TOL
            assert not g[3] or 0 in g[0]                                              # a finished sequence ends in the stored 0
    assert either <= F.NEAR_TIE_FRACTION * picks, (either, picks)
    assert any(e[3] for img in out for e in img)                                      # the boost finishes sequences inside 6 steps


# ------------------------------------------------------------------------------------------- the route at V % 4 != 0
@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_a_vocabulary_that_is_no_multiple_of_4_takes_the_register_path(kind):
    """`editnet_small_end` / `dcnet_small_end` (V = 203, as 9490 no multiple of 4): the search pads the leading dimension of its
    step logits, so every pick launches the float4 kernel (profile scope sbs_rows, never sbs_rows_scalar), and the result is
    the oracle's search on the route's own logits"""
    from show_edit_tell_amd import _lib as L, evaluate
    if kind == "editnet":
        d, _, rl = editnet_modules("editnet_small_end")
        inputs = (to_dev(d["X"][:2]), to_dev(d["prev"][:2]), to_dev(d["plen"][:2]))
    else:
        d, _, rl = dcnet_modules("dcnet_small_end")
        inputs = (to_dev(d["prev"][:2]), to_dev(d["plen"][:2]))
    wm, end = d["wm"], int(d["wm"]["<end>"])
    assert rl.vocab_size % 4 != 0
    lib = L.load()
    torch.manual_seed(31)
    lib.set_profile_enable(1)
    out, steps = evaluate.sample_captions_distinct(rl, *inputs, wm, n_samples=3, max_steps=F.SEARCH_MAX_STEPS, _return_steps=True)
    torch.cuda.synchronize()
    tags = [r["tag"] for r in L.profile_report()]
    lib.set_profile_enable(0)
    assert "sbs_rows" in tags and "sbs_merge" in tags and "sbs_rows_scalar" not in tags, tags
    Ls = [s.cpu().numpy() for s in steps]
    assert Ls[0].shape == (6, rl.vocab_size)
    states, infos = SO.search(lambda t, st: Ls[t], 2, 3, len(Ls), _seed_of(31), F.OFFSET, end)
    want = SO.results(states, end, F.SEARCH_MAX_STEPS)
    margin = min(SO.margin(step[i]) for step in infos for i in range(2) if not step[i].get("noop"))
    print(kind, "V =", rl.vocab_size, "smallest margin %.4f" % margin, out)
    picks = either = 0
    for i in range(2):
        margins = [SO.margin(step[i]) for step in infos if not step[i].get("noop")]
        picks += 3 * len(margins)
        if [e[0] for e in out[i]] != [e[0] for e in want[i]]:
            near = sum(1 for m in margins if m < F.GAP)
            assert near > 0, (i, out[i], want[i])         # only a near tie may go either way
            either += 3 * near
            continue
        for g, w in zip(out[i], want[i]):
            assert g[3] == w[3] and abs(g[1] - w[1]) <= F.TOL and abs(g[2] - w[2]) <= F.TOL, (i, g, w)
    assert either <= F.NEAR_TIE_FRACTION * picks, (either, picks)


# ------------------------------------------------------------------------------------------- 3. one slot: the Gumbel-max rollout
def test_one_sample_is_the_gumbel_rollout():
    from show_edit_tell_amd import evaluate
    wm, rl, (X, prev, plen) = _model("editnet")
    end = int(wm["<end>"])
    out, steps = _call("editnet", 2, 1, 7, _return_steps=True)
    torch.manual_seed(7)
    seq, _ = evaluate.sample_captions(rl, X, prev, plen, wm, n_samples=1, sampler="gumbel")
    seq = seq.cpu().numpy()[:, 0]
    L = [s.cpu().numpy() for s in steps]
    seed, safe = _seed_of(7), 0
    assert evaluate.tokens_from_greedy([e[0][0] for e in out], wm)                     # the rollouts' convention
    for i in range(2):
        tk = out[i][0][0]
        n = tk.index(0) + 1 if 0 in tk else len(tk)
        gaps = [GO.draw(L[t][i:i + 1], seed, F.OFFSET, t, 1.0, rows=[i])[1][0] for t in range(min(n, len(L)))]
        if min(gaps) < GF.gap_limit(1):                   # the two routes' logits differ by up to 1e-4: not a margin-safe row
            continue
        safe += 1
        assert seq[i, :n].tolist() == tk[:n], (i, seq[i], tk)
        assert out[i][0][2] == 0.0                        # one slot: G stays the root's
    assert safe >= 1


# ------------------------------------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_manual_seed_reproduces_a_call(kind):
    a, b, c = _call(kind, 2, 3, 11, 0.8), _call(kind, 2, 3, 11, 0.8), _call(kind, 2, 3, 12, 0.8)
    assert a == b                                         # tokens, and the floats bit for bit
    assert a != c


# ------------------------------------------------------------------------------------------- 5. no trace on the other entry points
def test_other_entry_points_are_unchanged_by_a_call():
    from show_edit_tell_amd import evaluate
    wm, rl, (X, prev, plen) = _model("editnet")

    def probe():
        with torch.no_grad():
            g = rl(wm, prev, plen, X, True, False)
        b = evaluate.beam_search_editnet_batched(rl, X, prev, plen, wm, 3, max_steps=8, return_scores=True)
        torch.manual_seed(3)
        s = evaluate.sample_captions(rl, X, prev, plen, wm, n_samples=2, sampler="gumbel")
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (*g, *s)], repr(b)

    _boost("editnet", 1.0)
    probe()
    before = probe()
    _call("editnet", 2, 5, 21)
    assert probe() == before


# ------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    from show_edit_tell_amd import evaluate
    wm, rl, (X, prev, plen) = _model("editnet")
    _, dae, _ = _model("dcnet")
    d, ad = adaptive_module("editnet_adaptive_small")
    with pytest.raises(ValueError, match="editnet_rl.DecoderC.*dcnet_rl.DAE"):
        evaluate.sample_captions_distinct(ad, X, prev, plen, d["wm"])
    with pytest.raises(ValueError, match="editnet_rl.DecoderC.*dcnet_rl.DAE"):
        evaluate.sample_captions_distinct((rl, dae), X, prev, plen, wm)
    for n in (0, 9):
        with pytest.raises(ValueError, match="n_samples"):
            evaluate.sample_captions_distinct(rl, X, prev, plen, wm, n_samples=n)
    with pytest.raises(ValueError):
        evaluate.sample_captions_distinct(rl, prev, plen, wm)          # EditNet without its image features
