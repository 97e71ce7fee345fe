"""GPU: one reader serves both device metrics (csrc/ngram_wave.h wave_read, used by csrc/bleu_device.hip and
csrc/ciderd_device.hip).  The same 8 rows go through set_bleu_device_prepare and set_ciderd_device_vectorise under both length
conventions; the keys of both records are compared with ciderd.pack_key of the row's slices computed here.  Integers only:
every comparison is exact."""
import numpy as np
import pytest
import torch

from hip_adapter import to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 64
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64)


def _rows():
    """row r: LENGTHS[r] ids of 1..3 (so grams repeat), then a 0 and junk of 1..3 behind it"""
    rng = np.random.default_rng(5)
    H = rng.integers(1, 4, (len(LENGTHS), L)).astype(np.int64)
    for r, n in enumerate(LENGTHS):
        if n < L:
            H[r, n] = 0
    return H


def _expected(sent):
    """(every occurrence (L, 4), first occurrences only (4, L)) packed keys of one sentence, uint64"""
    from show_edit_tell_amd import ciderd
    every = np.zeros((L, 4), dtype=np.uint64)
    first = np.zeros((4, L), dtype=np.uint64)
    for k in range(4):
        seen = set()
        for i in range(len(sent) - k):
            key = ciderd.pack_key(sent[i:i + k + 1])
            every[i, k] = key
            if key not in seen:
                first[k, i] = key
                seen.add(key)
    return every, first


@pytest.mark.parametrize("explicit", (False, True), ids=("zero_rule", "explicit_lengths"))
def test_one_reader_serves_both_metrics(explicit):
    from show_edit_tell_amd import _lib, bleu, ciderd
    H = _rows()
    if explicit:                                       # the row is exactly that long; the 0 and the junk behind it do not count
        sents = [H[r, :n].tolist() for r, n in enumerate(LENGTHS)]
        lens = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    else:                                              # cut after the first 0, the 0 stays; no 0: the whole row
        sents = [H[r, :min(n + 1, L)].tolist() for r, n in enumerate(LENGTHS)]
        lens = None
    assert [len(s) for s in sents] == (list(LENGTHS) if explicit else [1, 2, 3, 4, 5, 6, 64, 64])
    want = [_expected(s) for s in sents]
    R = len(LENGTHS)
    Hd = to_dev(H)

    bsc = bleu.device_scorer(DEV)
    brec = torch.full((R * (8 + 4 * L),), -1, dtype=torch.int64, device=DEV)
    _lib.check(bsc._lib.set_bleu_device_prepare(Hd.data_ptr(), L, None if lens is None else lens.data_ptr(), R, L, brec.data_ptr(),
                                                _lib.stream_of(bsc.dev)), "set_bleu_device_prepare")
    brec = brec.cpu().numpy().view(np.uint64).reshape(R, 8 + 4 * L)

    dsc = ciderd.CiderD({("1",): 1, ("1", "2"): 1}, 2, n=4).device(DEV)
    crec, got_L = dsc.vectorise(Hd, lens)
    assert got_L == L
    crec = crec.cpu().numpy().view(np.uint64).reshape(R, 8 + 8 * L)

    for r, s in enumerate(sents):
        every, first = want[r]
        assert brec[r, 0] == len(s) == crec[r, 5], r                      # the lengths in both headers agree
        assert brec[r, 1] == 0 and crec[r, 6] == 0, r                     # no id that cannot be packed
        assert np.array_equal(brec[r, 8:].reshape(L, 4), every), r        # BLEU: every occurrence, [position][order]
        assert np.array_equal(crec[r, 8:8 + 4 * L].reshape(4, L), first), r   # CIDEr-D: first occurrences, [order][position]
        assert len(s) < 63 or (first != 0).sum() < (every != 0).sum() // 2, r   # ids 1..3: most grams of a long row are repeats
