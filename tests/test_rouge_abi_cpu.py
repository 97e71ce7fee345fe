"""CPU: the device ROUGE-L route (csrc/rouge_device.hip, rouge.DeviceRougeL) as far as it goes without a GPU: the entry point is
exported and refuses bad arguments before any HIP call, the SCST steps take rouge_weight, and the reward mix on stub scorers."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import rouge_oracle

SET_OK, SET_ERR_ARG, SET_ERR_UNSUPPORTED = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_export(lib):
    from show_edit_tell_amd import _lib
    name = "set_rouge_device_score"
    assert name in _lib.PROTOTYPES and name not in _lib.MISSING and hasattr(lib, name)
    assert lib.set_abi_version() == 1


def test_score_validation(lib):
    one = C.c_void_p(16)                                      # never dereferenced: every refusal comes first

    def score(hyp=one, ld=20, n_hyp=2, L=20, set_of=one, recs=one, ref_L=20, n_refs=5, off=one, n_sets=1, max_set=5, beta=1.2,
              stats=one, scores=None, pairs=None, pair_ld=0):
        return lib.set_rouge_device_score(hyp, ld, None, n_hyp, L, set_of, recs, ref_L, n_refs, off, n_sets, max_set, beta, stats,
                                          scores, pairs, pair_ld, None)
    assert score(L=65, ld=65) == SET_ERR_UNSUPPORTED
    assert score(ref_L=65) == SET_ERR_UNSUPPORTED
    assert score(pairs=one, pair_ld=4) == SET_ERR_ARG                                 # pair_ld below the largest set
    for kw in (dict(hyp=None), dict(set_of=None), dict(recs=None), dict(off=None), dict(stats=None), dict(n_hyp=-1),
               dict(n_sets=-1), dict(n_refs=-1), dict(max_set=-1), dict(L=0), dict(ref_L=0), dict(ld=19),
               dict(beta=0.0), dict(beta=-1.2), dict(beta=float("nan")), dict(beta=float("inf")), dict(beta=float("-inf"))):
        assert score(**kw) == SET_ERR_ARG, kw
    # a bad argument wins over an unsupported length
    assert score(L=65, ld=65, stats=None) == SET_ERR_ARG and score(ref_L=65, beta=0.0) == SET_ERR_ARG
    assert score(L=65, ld=65, off=None) == SET_ERR_ARG
    assert score(n_hyp=0, hyp=None, set_of=None, stats=None) == SET_OK                # no hypothesis: a successful no-op


def test_device_scorer_refuses_cpu():
    from show_edit_tell_amd import rouge
    from show_edit_tell_amd._lib import SetError
    for make in (rouge.DeviceRougeL, rouge.device_scorer):
        with pytest.raises(SetError) as e:
            make("cpu")
        assert str(e.value) == "the device ROUGE-L scorer needs a GPU device, got cpu"


def test_scst_steps_take_rouge_weight_and_check_the_route():
    from show_edit_tell_amd import train
    x = torch.zeros(2, 3)
    for w in (0.0, 0.5):
        with pytest.raises(ValueError, match="reward"):
            train.scst_train_step(None, None, {}, x, x, x, [], None, reward="bogus", rouge_weight=w)
        with pytest.raises(ValueError, match="reward"):
            train.dcnet_scst_train_step(None, None, {}, x, x, [], None, reward="bogus", bleu_weight=w, rouge_weight=w)


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


class _Rouge:
    def __init__(self, r):
        self.r, self.calls = np.asarray(r, dtype=np.float64), []

    def score_token_ids(self, hyps, hyp_set, ref_sets, hyp_lens=None):
        self.calls.append((np.asarray(hyps).copy(), np.asarray(hyp_set).copy(), ref_sets, hyp_lens))
        return np.zeros((len(self.r), 4), dtype=np.int64), self.r.copy()


SAMPLED = np.array([[5, 6, 0, 0], [7, 0, 0, 0], [5, 5, 6, 0], [8, 9, 1, 2]])
GREEDY = np.array([[5, 0, 0, 0], [7, 8, 0, 0], [5, 0, 0, 0], [7, 8, 0, 0]])
GT2 = [[[5, 6, 0], [6, 0]], [[7, 8, 0]]]
CS = np.array([1.0, 2.0, 0.5, 0.25, 0.75, 1.5, 0.75, 1.5]) / 3.0
BS = np.array([0.9, 0.1, 0.3, 1e-6, 0.2, 0.7, 0.2, 0.7]) / 7.0
RS = np.array([0.8, 0.3, 0.6, 0.0, 0.5, 1.0, 0.5, 1.0]) / 11.0


def test_rouge_weight_zero_makes_the_calls_made_before():
    """the CIDEr-D and BLEU stubs record exactly what they record without the argument; the ROUGE stub sees no call"""
    from show_edit_tell_amd import ciderd
    gt = GT2 * 2

    def run(*extra):
        sc, bl = _Cider(CS), _Bleu(BS)
        out = ciderd.self_critical_reward(sc, SAMPLED, GREEDY, gt, 0.7, bl, 0.3, *extra)
        return out, sc.calls, bl.calls
    base, c_calls, b_calls = run()
    assert len(c_calls) == 1 and len(b_calls) == 1
    for extra in ((None, 0.0), (_Rouge(RS), 0.0), (None, 0.2)):
        out, c2, b2 = run(*extra)
        assert np.array_equal(out, base) and out.dtype == np.float32
        assert c2 == c_calls
        assert len(b2) == 1 and all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(b2[0], b_calls[0]))
        if extra[0] is not None:
            assert extra[0].calls == []


def test_rouge_weight_zero_imports_nothing_of_rouge():
    """a fresh interpreter: the host reward with rouge_weight = 0 and the steps' argument check leave rouge.py unimported"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from test_rouge_abi_cpu import _Cider, SAMPLED, GREEDY, GT2, CS\n"
            "from show_edit_tell_amd import ciderd, train\n"
            "ciderd.self_critical_reward(_Cider(CS), SAMPLED, GREEDY, GT2 * 2, 1.0, None, 0.0, None, 0.0)\n"
            "assert 'show_edit_tell_amd.rouge' not in sys.modules\n"
            "print('ok')\n" % (root, os.path.join(root, "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr


def test_host_reward_mix_on_stubs():
    from show_edit_tell_amd import ciderd
    gt = GT2 * 2
    sc, bl, rg = _Cider(CS), _Bleu(BS), _Rouge(RS)
    got = ciderd.self_critical_reward(sc, SAMPLED, GREEDY, gt, 0.7, bl, 0.3, rg, 0.2)
    want = (0.7 * (CS[:4] - CS[4:]) + 0.3 * (BS[:4] - BS[4:]) + 0.2 * (RS[:4] - RS[4:])).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (4, 4)
    assert np.array_equal(got, np.repeat(want[:, None], 4, 1))
    assert len(sc.calls) == 1 and len(bl.calls) == 1 and len(rg.calls) == 1
    hyps, hyp_set, sets, lens = rg.calls[0]
    assert np.array_equal(hyps, np.concatenate([SAMPLED, GREEDY])) and lens is None
    assert hyp_set.tolist() == [0, 1, 0, 1, 0, 1, 0, 1] and sets == GT2          # the distinct images' sets, once each
    # the ROUGE term without a BLEU scorer
    got = ciderd.self_critical_reward(_Cider(CS), SAMPLED, GREEDY, gt, 0.7, rouge_scorer=_Rouge(RS), rouge_weight=0.2)
    want = (0.7 * (CS[:4] - CS[4:]) + 0.2 * (RS[:4] - RS[4:])).astype(np.float32)
    assert np.array_equal(got[:, 0], want)


def test_host_reward_mix_with_the_real_rouge():
    """the ROUGE-L term alone (cider weight 0) equals the oracle's score difference under the rows' 0 rule"""
    from show_edit_tell_amd import ciderd, rouge
    gt = GT2 * 2
    got = ciderd.self_critical_reward(_Cider(np.zeros(8)), SAMPLED, GREEDY, gt, 0.0, None, 0.0, rouge.RougeL(), 2.0)
    r = lambda row, R: rouge_oracle.sentence(rouge_oracle.cut_after_zero(row), R)
    want = np.array([2.0 * (r(SAMPLED[i], gt[i]) - r(GREEDY[i], gt[i])) for i in range(4)])
    assert (np.abs(want) > 1e-2).sum() >= 3                              # the term is there
    assert np.array_equal(got[:, 0], want.astype(np.float32)) and np.array_equal(got[:, 0], got[:, 3])
