"""CPU: the device BLEU route (csrc/bleu_device.hip, bleu.DeviceBleu) as far as it goes without a GPU: the entry points are
exported and refuse bad arguments before any HIP call, the SCST steps take bleu_weight, and the reward mix on stub scorers."""
import ctypes as C

import numpy as np
import pytest
import torch

SET_OK, SET_ERR_ARG, SET_ERR_UNSUPPORTED = 0, 1, 2
NAMES = ("set_bleu_device_ref_bytes", "set_bleu_device_prepare", "set_bleu_device_score")


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_exports(lib):
    from show_edit_tell_amd import _lib
    for name in NAMES:
        assert name in _lib.PROTOTYPES and name not in _lib.MISSING and hasattr(lib, name), name


def test_ref_bytes(lib):
    assert lib.set_bleu_device_ref_bytes(3, 20) == 3 * (8 + 4 * 20) * 8
    assert lib.set_bleu_device_ref_bytes(1, 64) == (8 + 256) * 8 and lib.set_bleu_device_ref_bytes(1, 1) == 12 * 8
    assert lib.set_bleu_device_ref_bytes(0, 64) == 0
    assert lib.set_bleu_device_ref_bytes(-1, 20) == 0
    assert lib.set_bleu_device_ref_bytes(1, 0) == 0 and lib.set_bleu_device_ref_bytes(1, 65) == 0
    assert lib.set_bleu_device_ref_bytes(1, -3) == 0


def test_prepare_validation(lib):
    one = C.c_void_p(16)                                      # never dereferenced: every refusal comes first
    prep = lib.set_bleu_device_prepare
    assert prep(one, 65, None, 2, 65, one, None) == SET_ERR_UNSUPPORTED              # L = 65
    assert prep(None, 20, None, 2, 20, one, None) == SET_ERR_ARG
    assert prep(one, 20, None, 2, 20, None, None) == SET_ERR_ARG
    assert prep(one, 19, None, 2, 20, one, None) == SET_ERR_ARG                      # ld < L
    assert prep(one, 20, None, -1, 20, one, None) == SET_ERR_ARG
    assert prep(one, 20, None, 2, 0, one, None) == SET_ERR_ARG
    assert prep(None, 20, None, 0, 20, None, None) == SET_OK                         # no reference: nothing to do


def test_score_validation(lib):
    one = C.c_void_p(16)

    def score(hyp=one, ld=20, n_hyp=2, L=20, set_of=one, recs=one, ref_L=20, n_refs=5, off=one, n_sets=1, max_set=5, stats=one,
              scores=None, pairs=None, pair_ld=0):
        return lib.set_bleu_device_score(hyp, ld, None, n_hyp, L, set_of, recs, ref_L, n_refs, off, n_sets, max_set, stats,
                                         scores, pairs, pair_ld, None)
    assert score(L=65, ld=65) == SET_ERR_UNSUPPORTED
    assert score(ref_L=65) == SET_ERR_UNSUPPORTED
    assert score(pairs=one, pair_ld=4) == SET_ERR_ARG                                 # pair_ld below the largest set
    for kw in (dict(hyp=None), dict(set_of=None), dict(recs=None), dict(off=None), dict(stats=None), dict(n_hyp=-1),
               dict(n_sets=-1), dict(n_refs=-1), dict(max_set=-1), dict(L=0), dict(ref_L=0), dict(ld=19)):
        assert score(**kw) == SET_ERR_ARG, kw
    assert score(n_hyp=0, hyp=None, set_of=None, stats=None) == SET_OK                # no hypothesis: a successful no-op


def test_device_scorer_refuses_cpu():
    from show_edit_tell_amd import bleu
    from show_edit_tell_amd._lib import SetError
    with pytest.raises(SetError):
        bleu.DeviceBleu("cpu")
    with pytest.raises(SetError):
        bleu.device_scorer("cpu")


def test_scst_steps_take_bleu_weight_and_check_the_route():
    from show_edit_tell_amd import train
    x = torch.zeros(2, 3)
    for w in (0.0, 0.5):
        with pytest.raises(ValueError, match="reward"):
            train.scst_train_step(None, None, {}, x, x, x, [], None, reward="bogus", bleu_weight=w)
        with pytest.raises(ValueError, match="reward"):
            train.dcnet_scst_train_step(None, None, {}, x, x, [], None, reward="bogus", bleu_weight=w)
    assert train.REWARD_ROUTES == ("host", "device")


class _Cider:
    """a CIDEr-D scorer without the native handle: the string route of self_critical_reward; scores from a table"""
    def __init__(self, scores):
        self.scores, self.calls = np.asarray(scores, dtype=np.float64), []

    def compute_score(self, gts, res):
        self.calls.append((gts, res))
        return float(self.scores.mean()), self.scores


class _Bleu:
    def __init__(self, b4):
        self.b4, self.calls = np.asarray(b4, dtype=np.float64), []

    def score_token_ids(self, hyps, hyp_set, ref_sets, hyp_lens=None):
        self.calls.append((np.asarray(hyps).copy(), np.asarray(hyp_set).copy(), ref_sets, hyp_lens))
        sc = np.zeros((len(self.b4), 4))
        sc[:, 3] = self.b4
        return np.zeros((len(self.b4), 10), dtype=np.int64), sc


SAMPLED = np.array([[5, 6, 0, 0], [7, 0, 0, 0], [5, 5, 6, 0], [8, 9, 1, 2]])
GREEDY = np.array([[5, 0, 0, 0], [7, 8, 0, 0], [5, 0, 0, 0], [7, 8, 0, 0]])
GT2 = [[[5, 6, 0], [6, 0]], [[7, 8, 0]]]


def test_bleu_weight_zero_makes_the_calls_made_before():
    """B = 4 rows over 2 images (the repeated rollout: row b, image b % 2): the CIDEr-D scorer gets one compute_score call with
    the dictionaries the function built before it knew of BLEU, the BLEU scorer none"""
    from show_edit_tell_amd import ciderd
    gt = GT2 * 2
    want_gts = {i: (["5 6 0", "6 0"], ["7 8 0"])[i % 2] for i in range(8)}
    want_res = [{'image_id': i, 'caption': [c]} for i, c in
                enumerate(["5 6 0", "7 0", "5 5 6 0", "8 9 1 2", "5 0", "7 8 0", "5 0", "7 8 0"])]
    cs = np.array([1.0, 2.0, 0.5, 0.25, 0.75, 1.5, 0.75, 1.5])
    out = []
    for extra in ((), (None, 0.0), (_Bleu(np.zeros(8)), 0.0), (None, 0.5)):
        sc = _Cider(cs)
        out.append(ciderd.self_critical_reward(sc, SAMPLED, GREEDY, gt, 0.5, *extra))
        assert sc.calls == [(want_gts, want_res)]
        if extra and extra[0] is not None:
            assert extra[0].calls == []
    want = np.repeat((0.5 * (cs[:4] - cs[4:]))[:, None], 4, 1).astype(np.float32)
    for o in out:
        assert o.dtype == np.float32 and np.array_equal(o, want)


def test_host_reward_mix_on_stubs():
    from show_edit_tell_amd import ciderd
    gt = GT2 * 2
    cs = np.array([1.0, 2.0, 0.5, 0.25, 0.75, 1.5, 0.75, 1.5]) / 3.0
    bs = np.array([0.9, 0.1, 0.3, 1e-6, 0.2, 0.7, 0.2, 0.7]) / 7.0
    sc, bl = _Cider(cs), _Bleu(bs)
    got = ciderd.self_critical_reward(sc, SAMPLED, GREEDY, gt, 0.7, bl, 0.3)
    want = (0.7 * (cs[:4] - cs[4:]) + 0.3 * (bs[:4] - bs[4:])).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (4, 4)
    assert np.array_equal(got, np.repeat(want[:, None], 4, 1))
    assert len(sc.calls) == 1 and len(bl.calls) == 1
    hyps, hyp_set, sets, lens = bl.calls[0]
    assert np.array_equal(hyps, np.concatenate([SAMPLED, GREEDY])) and lens is None
    assert hyp_set.tolist() == [0, 1, 0, 1, 0, 1, 0, 1] and sets == GT2          # the distinct images' sets, once each


def test_host_reward_mix_with_the_real_bleu():
    """the BLEU term alone (cider weight 0) equals the oracle's sentence BLEU-4 difference under the rows' 0 rule"""
    import bleu_oracle
    from show_edit_tell_amd import bleu, ciderd
    gt = GT2 * 2
    got = ciderd.self_critical_reward(_Cider(np.zeros(8)), SAMPLED, GREEDY, gt, 0.0, bleu.Bleu(), 2.0)
    b = lambda row, R: bleu_oracle.sentence(bleu_oracle.cut_after_zero(row), R)[3]
    want = np.array([2.0 * (b(SAMPLED[i], gt[i]) - b(GREEDY[i], gt[i])) for i in range(4)])
    assert np.abs(want).min() > 1e-4                                    # short sentences: BLEU-4 is small, but no term is zero
    assert np.array_equal(got[:, 0], want.astype(np.float32)) and np.array_equal(got[:, 0], got[:, 3])
