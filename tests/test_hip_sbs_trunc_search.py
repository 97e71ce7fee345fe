"""GPU: evaluate.sample_captions_distinct / sample_captions_distinct_ensemble under top_p and top_k on `editnet_small`,
`dcnet_small` and their pair (tests/golden/editnet_small.npz, dcnet_small.npz; V = 203, max_steps 6): the whole search equals
the float64 oracle's search (tests/sbs_trunc_oracle.py) replayed on the route's own per-step logits; top_k = 1 returns the one
greedy sequence; neutral keywords change nothing; the padded register route is taken.  Fixtures: tests/sbs_trunc_fixtures.py."""
import numpy as np
import pytest
import torch

import sbs_ensemble_fixtures as E
import sbs_fixtures as F
import sbs_oracle as SO
import sbs_trunc_fixtures as T
import sbs_trunc_oracle as TS
from hip_adapter import dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
_CACHE = {}


def _models():
    """(word_map, EditNet, DCNet, (X, prev, plen) of two images): built once; both models take EditNet's caption pair"""
    if not _CACHE:
        de, _, dec = editnet_modules("editnet_small")
        _, _, dae = dcnet_modules("dcnet_small")
        _CACHE["m"] = (de["wm"], dec, dae, (to_dev(de["X"][:2]), to_dev(de["prev"][:2]), to_dev(de["plen"][:2])))
    return _CACHE["m"]


def _call(kind, NI, n, seed, **kw):
    from show_edit_tell_amd import evaluate
    wm, dec, dae, (X, prev, plen) = _models()
    torch.manual_seed(seed)
    kw = dict(n_samples=n, max_steps=T.SEARCH_MAX_STEPS, **kw)
    if kind == "ensemble":
        return evaluate.sample_captions_distinct_ensemble(dec, dae, X[:NI], prev[:NI], plen[:NI], wm, **kw)
    if kind == "editnet":
        return evaluate.sample_captions_distinct(dec, X[:NI], prev[:NI], plen[:NI], wm, **kw)
    return evaluate.sample_captions_distinct(dae, prev[:NI], plen[:NI], wm, **kw)


def _steps_np(kind, steps):
    if kind == "ensemble":
        return [(e.cpu().numpy(), d.cpu().numpy()) for e, d in steps]
    return [s.cpu().numpy() for s in steps]


def _replay(kind, n, NI, seed, temperature):
    """the call under top_p, and the oracle's search replayed on the route's own per-step logits: (out, states, infos, smallest
    margin, smallest boundary distance, smallest cut gap)"""
    end = int(_models()[0]["<end>"])
    out, steps = _call(kind, NI, n, seed, top_p=T.SEARCH_TOP_P, temperature=temperature, _return_steps=True)
    Ls = _steps_np(kind, steps)
    states, infos = TS.search(lambda t, st: Ls[t], NI, n, len(Ls), E.seed_of(seed), T.OFFSET, end, F.inv_t(temperature), 0,
                              T.SEARCH_TOP_P, temperature=temperature)
    return out, states, infos, TS.smallest_margin(infos), TS.smallest_dist(infos), TS.smallest_gap(infos)


@pytest.mark.parametrize("kind,n,NI", sorted(T.SEARCH))
def test_search_matches_the_oracle_on_the_routes_own_logits(kind, n, NI):
    """ONE recorded seed per case (tests/sbs_trunc_fixtures.py SEARCH).  The replay's margins are asserted, not assumed: the
    route's logits are deterministic for the golden weights, and with them clear nothing below rests on an "either" decision."""
    end = int(_models()[0]["<end>"])
    seed, temperature = T.SEARCH[(kind, n, NI)]
    out, states, infos, m, d, g = _replay(kind, n, NI, seed, temperature)
    print(kind, n, NI, "seed", seed, "smallest margin %.4g, boundary distance %.4g, cut gap %.4g" % (m, d, g), out)
    assert m >= 10.0 * T.GAP and d >= T.BOUNDARY_MIN and (kind != "ensemble" or g >= T.CUT_GAP_MIN)
    want = SO.results(states, end, T.SEARCH_MAX_STEPS)
    for i in range(NI):
        assert [e[0] for e in out[i]] == [e[0] for e in want[i]], i                   # tokens and order
        assert len(out[i]) == len(want[i])
        for g_, w in zip(out[i], want[i]):
            assert g_[3] == w[3] and abs(g_[1] - w[1]) <= T.TOL and abs(g_[2] - w[2]) <= T.TOL, (i, g_, w)
        assert all(a[2] >= b[2] for a, b in zip(out[i], out[i][1:]))
    # every returned word lies in its step's kept set: walk the ancestry of every final slot; a finished parent's carried
    # <end> (no step taken: the oracle's step_logp is exactly 0) is the only entry that is not a pick
    checked = 0
    for i in range(NI):
        for s in range(len(want[i])):
            slot = s
            for t in range(len(infos) - 1, -1, -1):
                info = infos[t][i]
                if info.get("noop"):
                    continue
                p, w = info["parents"][slot], info["words"][slot]
                carried = w == end and info["step_logp"][slot] == 0.0
                if not carried:
                    assert w >= 0 and info["kept"][p, w], (i, s, t, w)
                    checked += 1
                slot = p
    assert checked >= NI * n


@pytest.mark.parametrize("kind", ["editnet", "dcnet", "ensemble"])
def test_top_k_1_returns_the_one_greedy_sequence(kind):
    wm = _models()[0]
    end = int(wm["<end>"])
    out, kappa, steps = _call(kind, 2, 3, 411, top_k=1, return_threshold=True, _return_steps=True)
    Ls = _steps_np(kind, steps)
    for i in range(2):
        assert len(out[i]) == 1 and kappa[i] == float("-inf")
        tokens, logp, G, fin = out[i][0]
        assert logp == 0.0 and G == 0.0
        # slot 0 of the image is the only live one at every step: its row's arg-max is the word
        for t, L in enumerate(Ls):
            z = E.mean_logp(L[0], L[1])[i * 4] if kind == "ensemble" else L[i * 4]
            w = int(np.argmax(z))
            assert tokens[t] == (0 if w == end else w), (i, t)
            if w == end:
                assert fin
                break


@pytest.mark.parametrize("kind", ["editnet", "dcnet", "ensemble"])
def test_neutral_keywords_return_what_the_call_without_them_returns(kind):
    assert _call(kind, 2, 3, 421) == _call(kind, 2, 3, 421, top_k=0, top_p=1.0)
    assert _call(kind, 2, 3, 421) == _call(kind, 2, 3, 421, top_k=203)                # top_k >= V is off


def test_the_padded_register_route_is_taken():
    from show_edit_tell_amd import _lib as L
    lib = L.load()
    for kind, tag in (("editnet", "sbs_rows_trunc"), ("ensemble", "sbs_rows_ens_trunc")):
        lib.set_profile_enable(1)
        _call(kind, 2, 3, 431, top_p=T.SEARCH_TOP_P)
        torch.cuda.synchronize()
        tags = [r["tag"] for r in L.profile_report()]
        lib.set_profile_enable(0)
        assert tag in tags and "sbs_merge" in tags and tag + "_scalar" not in tags, tags
        assert "sbs_rows" not in tags and "sbs_rows_ens" not in tags, tags
