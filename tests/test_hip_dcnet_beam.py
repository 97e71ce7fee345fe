"""GPU: DCNet's beam search of one previous caption as prologue + ONE persistent launch (csrc/decode_persistent.hip, beam
mode; include/set_hip.h set_dcnet_beam_persistent; evaluate.beam_search_dcnet) — against the reference's own loop
(tests/golden/beam_full_b4.npz, dcnet.py:413-514) and against the batched per-step search, which tests/test_hip_beam.py pins
to the reference.  All at dcnet_full_b4 dimensions: the small cases' dimensions are outside the persistent launch."""
import numpy as np
import pytest
import torch

import beam_parity
from hip_adapter import dcnet_modules, load_numpy_state, to_dev
from oracle import cases

pytestmark = pytest.mark.gpu


def _dae(d, sd=None):
    from show_edit_tell_amd import dcnet
    dc = d["dcase"]
    return load_numpy_state(dcnet.DAE(d["wm"], None, dc["D"], dc["A"], dc["C"], dc["E"]), d["sd_d"] if sd is None else sd)


def _boosted(d, boost):
    """The golden's weights with the <end> boost changed from 4.0 to `boost` (float32 arithmetic)."""
    sd = {k: v.copy() for k, v in d["sd_d"].items()}
    end = d["wm"]["<end>"]
    sd["fc.bias"][end] = sd["fc.bias"][end] - np.float32(4.0) + np.float32(boost)
    return sd


def _tags(fn):
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


def test_per_image_persistent_dcnet_beam_vs_reference_beam():
    """The reference's evaluate() shape — one previous caption, beam 3 — on the persistent launch: all four searches of the
    golden finished with margins 6.39 - 7.30, so all four compare strictly (tokens identical, score within SCORE_TOL).  They end
    at the first pick: this pins the pick, the score and the output format, not the parent map (next test)."""
    from show_edit_tell_amd import evaluate
    d = cases.build_beam("beam_full_b4")
    g = beam_parity.load("beam_full_b4")
    wm, B = d["wm"], d["case"]["B"]
    dae = _dae(d)
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    firm = 0
    for b in range(B):
        one = (prev[b:b + 1], plen[b:b + 1])
        evaluate.beam_search_dcnet(dae, *one, wm, 3)                  # (the token table is built on the second call)
        (seq, sc), tags = _tags(lambda: evaluate.beam_search_dcnet(dae, *one, wm, 3))
        assert "persistent_beam" in tags, tags
        print("image", b, "tokens", seq, "score", sc, "reference", float(g["k3.dcnet.score"][b]), "margin", float(g["k3.dcnet.margin"][b]))
        firm += beam_parity.check_one(g, 3, "dcnet", b, seq, sc)
    assert firm == B, firm


def test_per_image_persistent_dcnet_beam_searches_that_run():
    """<end> boosts 2.6 / 3.0 / 3.4, k = 2 / 3 / 4, four prompts: 36 searches that end after 2 or 5 tokens with hypotheses
    finishing at different picks (k shrinks inside the launch), or run all 50 picks of parent permutation into the step limit.
    The persistent launch against beam_search_dcnet_batched on the same weights.  Finished: identical tokens, scores within
    SCORE_TOL.  Step limit: both NaN, length 18, the first 4 tokens equal.  The numpy oracle (oracle/beam_np.beam_dcnet) gives
    20 finished searches (3 of them with 5 tokens, every margin above 5) and 16 at the step limit; the counts asked for here
    (14 / 2 / 12) leave room for a device search that differs from numpy at a near-tie pick, nothing else."""
    from show_edit_tell_amd import evaluate
    d = cases.build_beam("beam_full_b4")
    wm, B = d["wm"], d["case"]["B"]
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    strict = long_strict = limit = total = 0
    for boost in (2.6, 3.0, 3.4):
        dae = _dae(d, _boosted(d, boost))
        for k in (2, 3, 4):
            batched, bscores = evaluate.beam_search_dcnet_batched(dae, prev, plen, wm, k, return_scores=True)
            for b in range(B):
                one = (prev[b:b + 1], plen[b:b + 1])
                evaluate.beam_search_dcnet(dae, *one, wm, k)          # (the token table is built on the second call)
                got = evaluate._beam_search_dcnet_persistent(dae, *one, wm, k)
                assert got is not None, "the persistent beam launch must be taken at k <= 4 with the token table active"
                seq, sc = got
                total += 1
                if np.isnan(bscores[b]):
                    agree = sum(int(x == y) for x, y in zip(seq, batched[b]))
                    print("boost", boost, "k", k, "row", b, "step limit:", agree, "of 18 tokens agree")
                    assert np.isnan(sc) and len(seq) == 18 and len(batched[b]) == 18 and seq[:4] == batched[b][:4], (boost, k, b, seq, batched[b])
                    limit += 1
                else:
                    print("boost", boost, "k", k, "row", b, "finished:", len(seq), "tokens, score", sc, "batched", bscores[b])
                    assert not np.isnan(sc), (boost, k, b, seq, batched[b])
                    assert abs(sc - bscores[b]) < beam_parity.SCORE_TOL, (boost, k, b, sc, bscores[b])
                    assert seq == batched[b], (boost, k, b, seq, batched[b])
                    strict += 1
                    long_strict += int(len(seq) >= 5)
    print("strict", strict, "of them with >= 5 tokens", long_strict, "step limit", limit, "of", total)
    assert total == 36 and strict + limit == total
    assert strict >= 14 and long_strict >= 2 and limit >= 12, (strict, long_strict, limit)


def test_routing_falls_back_to_the_batched_search(monkeypatch):
    """k = 5 and SET_DEC_PERSISTENT=0 (read per call): no persistent launch, beam_search_dcnet is the NI = 1 case of the
    batched search.  A module without a token table yet: None on its first call."""
    from show_edit_tell_amd import evaluate
    d = cases.build_beam("beam_full_b4")
    wm, B = d["wm"], d["case"]["B"]
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    fresh = _dae(d)
    assert evaluate._beam_search_dcnet_persistent(fresh, prev[:1], plen[:1], wm, 3) is None
    dae = _dae(d, _boosted(d, 3.4))

    def same(one, k):
        bseqs, bscores = evaluate.beam_search_dcnet_batched(dae, *one, wm, k, return_scores=True)
        seq, sc = evaluate.beam_search_dcnet(dae, *one, wm, k)
        if np.isnan(bscores[0]):
            assert np.isnan(sc) and len(seq) == 18 and seq[:4] == bseqs[0][:4], (seq, bseqs[0])
        else:
            assert seq == bseqs[0] and abs(sc - bscores[0]) < beam_parity.SCORE_TOL, (seq, sc, bseqs[0], bscores[0])

    for b in range(B):
        one = (prev[b:b + 1], plen[b:b + 1])
        evaluate.beam_search_dcnet(dae, *one, wm, 3)
        assert evaluate._beam_search_dcnet_persistent(dae, *one, wm, 3) is not None
        assert evaluate._beam_search_dcnet_persistent(dae, *one, wm, 5) is None
        same(one, 5)
    monkeypatch.setenv("SET_DEC_PERSISTENT", "0")
    for b in range(B):
        one = (prev[b:b + 1], plen[b:b + 1])
        assert evaluate._beam_search_dcnet_persistent(dae, *one, wm, 3) is None
        (_, tags) = _tags(lambda: same(one, 3))
        assert "persistent_beam" not in tags, tags


def test_beam_launch_leaves_the_other_modes_bit_identical():
    """Greedy at B = 4 and the teacher-forced forward with last_hidden, before and after a beam launch on the SAME module and
    the SAME workspace (k = 4 and 19 picks give the dims of both: B = 4, T = 18, maxT = 19): bit-identical outputs — the beam
    launch leaves nothing behind in the workspace that another mode reads."""
    from show_edit_tell_amd import evaluate
    from test_hip_dcnet_mse import _inputs, mse_module
    d, _, rl = dcnet_modules("dcnet_full_b4")
    wm = d["wm"]
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    _, ar = mse_module("dcnet_full_b4")

    def beam(module):
        before = set(module._ws_cache)
        for b in (1, 2):
            got = evaluate._beam_search_dcnet_persistent(module, prev[b:b + 1], plen[b:b + 1], wm, 4, max_steps=18)
            assert got is not None
        assert set(module._ws_cache) == before, "the beam launch must run in a workspace the other modes use"

    with torch.no_grad():
        for _ in range(2):
            rl(wm, prev, plen, True, False)
            ar(*_inputs(d))
        seq0, logp0 = rl(wm, prev, plen, True, False)
        out0 = ar(*_inputs(d))
        torch.cuda.synchronize()
        beam(rl)
        beam(ar.dae)
        (seq1, logp1), tags = _tags(lambda: rl(wm, prev, plen, True, False))
        assert "persistent_decode" in tags, tags
        out1, tags = _tags(lambda: ar(*_inputs(d)))
        assert "persistent_decode" in tags, tags
    assert torch.equal(seq0, seq1) and torch.equal(logp0, logp1)
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[5], out1[5]) and torch.equal(out0[4], out1[4])
