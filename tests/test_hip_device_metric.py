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


def test_one_preparation_serves_the_three_record_scorers():
    """prepare_refs of DeviceBleu, DeviceRougeL and DeviceEditDistance is one function: the same sets give three PreparedRefs
    that every one of the three scorers reads to the same bits, and each carries the upload DeviceCiderD.from_refs builds from."""
    from show_edit_tell_amd import bleu, ciderd, editdist, rouge
    rng = np.random.default_rng(11)
    long63, long64 = rng.integers(1, 4, 63).tolist(), rng.integers(1, 4, 64).tolist()
    sets = [[[7, 65534, 3, 0]],                                            # an id the packing refuses: the rows of this set
            [[], [2], long63, long64, [1, 2, 3, 0]]]                       # lengths 0, 1, 63, 64 and 4
    scorers = [bleu.device_scorer(DEV), rouge.device_scorer(DEV), editdist.device_scorer(DEV)]
    prepared = [sc.prepare_refs(sets) for sc in scorers]
    for p in prepared:
        assert (p.L, p.n_refs, p.n_sets, p.max_set) == (64, 6, 2, 5) and p.host_lens.tolist() == [4, 0, 1, 63, 64, 4]
        assert torch.equal(p.recs, prepared[0].recs) and torch.equal(p.tokens, prepared[0].tokens)
    hyps = np.zeros((4, L), dtype=np.int64)
    hyps[1, 0], hyps[2], hyps[3, :5] = 2, long64[1:] + [3], (1, 2, 3, 3, 1)
    hyp_lens, hyp_set = [0, 1, 64, 5], [1, 0, 1, 2]                        # set 2 does not exist: that row is refused
    bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t
    for sc in scorers:
        outs = [sc.score_token_ids(hyps, hyp_set, p, hyp_lens=hyp_lens, return_pairs=True) for p in prepared]
        stats = outs[0][0].cpu().numpy()
        # row 1: a reference that cannot be packed (BLEU marks its four counts, the others all four integers); row 3: refused
        assert stats[1, 0] == -1 and (stats[3] == -1).all() and (stats[0] >= 0).all() and (stats[2] >= 0).all(), sc.METRIC
        assert torch.isnan(outs[0][1][1]).all() and torch.isnan(outs[0][1][3]).all() and not torch.isnan(outs[0][1][2]).any()
        assert outs[0][2].shape == (4, 5) and not torch.isnan(outs[0][2][2]).any() and (outs[0][2][3] == 0).all()
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                assert torch.equal(bits(a), bits(b)), sc.METRIC
    cider = [ciderd.DeviceCiderD.from_refs(DEV, p) for p in prepared]
    want = bits(cider[0][0].score_token_ids(hyps, hyp_set, cider[0][1], hyp_lens=hyp_lens))
    for csc, crefs in cider[1:]:
        assert torch.equal(crefs.recs, cider[0][1].recs)
        assert torch.equal(bits(csc.score_token_ids(hyps, hyp_set, crefs, hyp_lens=hyp_lens)), want)
