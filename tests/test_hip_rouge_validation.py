"""GPU: evaluate.validation_rouge_l and evaluate.validation_scores against tests/rouge_oracle.py: a greedy-format id tensor and
token lists with word_map= (one of them never reached <end>), both values of count_end; validation_scores returns the bits of
validation_bleu and validation_rouge_l.  Tolerance: the mean of N scores in [0, 1], each within a few 1e-16 of the oracle's, in
another summation order: N * 2^-53 at the most, far inside the 1e-12 asserted."""
import numpy as np
import pytest
import torch

import rouge_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
V = 60


@pytest.fixture(scope="module")
def world():
    return _world()


def _world():
    """37 captions of 0..18 words over w1..w40, each with its own 1..5 references (near-copies and random ones), in the
    decoder's format (0 = <end>, junk behind it) and as token lists in the vocabulary's ids; list 3 never reached <end>, row 5
    of the tensor is full (no 0)"""
    from show_edit_tell_amd import synth
    wm = synth.word_map(V)
    start, end, pad = wm["<start>"], wm["<end>"], wm["<pad>"]
    rng = np.random.default_rng(21)
    N, L = 37, 19
    words, gt = [], []
    for i in range(N):
        n = L if i == 5 else int(rng.integers(0, 19))
        c = [int(x) for x in rng.integers(1, 41, n)]
        words.append(c)
        refs = []
        for j in range(1 + i % 5):
            if j % 2 == 0 and n > 1:
                r = list(c)
                r[int(rng.integers(0, n))] = int(rng.integers(1, 41))
                r = r[:max(1, n - j)]
            else:
                r = [int(x) for x in rng.integers(1, 41, int(rng.integers(1, 15)))]
            refs.append(r + [0])
        gt.append(refs)
    T = np.zeros((N, L), dtype=np.int64)
    for i, c in enumerate(words):
        T[i, :len(c)] = c
        T[i, len(c) + 1:] = rng.integers(0, 41, max(0, L - len(c) - 1))       # behind the first 0: junk
    assert 0 not in T[5] and any(len(c) == 0 for c in words)
    lists = [[start] + c + ([] if i == 3 else [end]) + [pad] * (i % 3) for i, c in enumerate(words)]
    assert len(words[3]) > 0
    return dict(wm=wm, words=words, gt=gt, T=T, lists=lists, N=N)


def _want(world, count_end, lists):
    """the oracle's corpus mean; count_end: the 0 is a token on both sides — for a caption that holds one"""
    pairs = []
    for i, c in enumerate(world["words"]):
        ended = (i != 3) if lists else (i != 5)
        h = c + [0] if (count_end and ended) else c
        R = [r if count_end else r[:-1] for r in world["gt"][i]]
        pairs.append((h, R))
    return rouge_oracle.corpus(pairs)


@pytest.mark.parametrize("count_end", [False, True])
def test_validation_rouge_l_against_oracle(world, count_end):
    from show_edit_tell_amd import evaluate
    got = evaluate.validation_rouge_l(torch.from_numpy(world["T"]).to(DEV), None, world["gt"], DEV, count_end=count_end)
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
    want = _want(world, count_end, lists=False)
    print("ROUGE_L %.6f (tensor), abs err %.3e" % (want, abs(float(got) - want)))
    assert 0.3 < want < 0.95 and abs(float(got) - want) <= TOL
    got = evaluate.validation_rouge_l(world["lists"], None, world["gt"], DEV, count_end=count_end, word_map=world["wm"])
    want_l = _want(world, count_end, lists=True)
    assert abs(float(got) - want_l) <= TOL
    assert count_end == (want_l != want)          # the list without <end> and the full row differ only where the 0 counts
    # an explicit set index: the captions in reverse order against the same sets
    idx = np.arange(world["N"])[::-1].copy()
    got = evaluate.validation_rouge_l(torch.from_numpy(world["T"][idx]).to(DEV), torch.from_numpy(idx).to(DEV), world["gt"], DEV,
                                      count_end=count_end)
    assert abs(float(got) - want) <= TOL


@pytest.mark.parametrize("count_end", [False, True])
def test_validation_scores_is_both_single_calls(world, count_end):
    from show_edit_tell_amd import evaluate
    for caps, kw in ((torch.from_numpy(world["T"]).to(DEV), {}), (world["lists"], dict(word_map=world["wm"]))):
        out = evaluate.validation_scores(caps, None, world["gt"], DEV, count_end=count_end, **kw)
        assert list(out) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L"]
        b = evaluate.validation_bleu(caps, None, world["gt"], DEV, count_end=count_end, **kw)
        r = evaluate.validation_rouge_l(caps, None, world["gt"], DEV, count_end=count_end, **kw)
        for k in range(4):
            v = out["Bleu_%d" % (k + 1)]
            assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 0
            assert torch.equal(v.view(torch.int64), b[k].view(torch.int64))
        assert out["ROUGE_L"].is_cuda and out["ROUGE_L"].dim() == 0
        assert torch.equal(out["ROUGE_L"].view(torch.int64), r.view(torch.int64))
        assert float(out["Bleu_1"]) > 0.3 and float(out["ROUGE_L"]) > 0.3
