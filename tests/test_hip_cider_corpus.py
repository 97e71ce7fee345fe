"""GPU: the corpus CIDEr table built on the device (csrc/ciderd_device.hip cd_build_k, set_ciderd_device_create_corpus) and what
stands on it — ciderd.DeviceCiderD.from_refs, evaluate.validation_cider, evaluate.validation_scores(cider=True) — against
tests/cider_oracle.py.

Counts are asserted EXACTLY (they are integers).  Scores: within 1e-9 of the float64 oracle, the bound
tests/test_hip_ciderd_device.py asserts for this score kernel (measured: profiles/cider_corpus_errors.json), and bit for bit
against the same kernel on a table that the host built from the oracle's counts: the two tables hold the same map."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cider_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-9


@pytest.fixture(scope="module")
def world():
    return cider_oracle.world()


def _bits(t):
    return t.contiguous().view(torch.int64)


def _lookup(scorer, grams):
    from show_edit_tell_amd import ciderd
    return scorer.lookup([ciderd.pack_key(g) for g in grams]).cpu().tolist()


def _check_table(scorer, df, absent):
    grams = sorted(df)
    assert _lookup(scorer, grams) == [float(df[g]) for g in grams]
    assert all(g not in df for g in absent) and _lookup(scorer, absent) == [0.0] * len(absent)
    assert scorer.dropped() == 0


def _host_scorer(df, n_docs, n=4):
    """the same score kernel on a table that the host built: the oracle's counts under decimal-string grams"""
    from show_edit_tell_amd import ciderd
    return ciderd.CiderD({tuple(str(w) for w in g): c for g, c in df.items()}, n_docs, n).device(DEV)


def _rows(hyps, L=None):
    L = max([1] + [len(h) for h in hyps]) if L is None else L
    T = np.zeros((len(hyps), L), dtype=np.int64)
    for i, h in enumerate(hyps):
        T[i, :len(h)] = h
    return torch.from_numpy(T).to(DEV), torch.tensor([len(h) for h in hyps], dtype=torch.int32, device=DEV)


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_end", [False, True])
def test_table_of_the_world(world, count_end):
    from show_edit_tell_amd import ciderd
    _, sets = cider_oracle.world_sides(world, count_end)
    df = cider_oracle.document_frequency(sets)
    sc, refs = ciderd.DeviceCiderD.from_refs(DEV, world["gt"], count_end=count_end)
    _check_table(sc, df, [(41,), (59,), (1, 41), (41, 1, 2), (50, 51, 52, 53), (65533,)])
    bound = sum(max(0, len(r) - k) for rs in sets for r in rs for k in range(4))
    assert sc.gram_bound == bound and sc.capacity >= 2 * bound > sc.capacity // 2 and sc.capacity & (sc.capacity - 1) == 0
    assert refs.n_sets == 37 and refs.n_refs == sum(len(rs) for rs in sets) and refs.max_set == 5


def _edge_sets():
    rng = np.random.default_rng(5)
    long64 = [int(x) for x in rng.integers(31, 60, 64)]
    five = [11, 12, 13, 12, 11]
    return [[[5, 6, 7]],                                                        # a set of one reference
            [[], [8], [8, 9], [5, 6, 7], [1, 2, 3, 4], long64, [9, 8, 9, 8, 9]],   # max_set = 7; 0, 1, 2, 3, 4 and 64 ids
            [],                                                                 # an empty set
            [[21] * 64, [21, 21]],                                              # one word 64 times
            [list(five) for _ in range(5)],                                     # the same sentence five times
            [[5, 6, 7], [7, 6, 5]]]


def test_table_edges():
    from show_edit_tell_amd import ciderd
    sets = _edge_sets()
    df = cider_oracle.document_frequency(sets)
    assert df[(21,)] == 1 and df[(21, 21, 21, 21)] == 1 and df[(11, 12)] == 1 and df[(5, 6, 7)] == 3 and df[(8,)] == 1
    sc, refs = ciderd.DeviceCiderD.from_refs(DEV, sets)
    assert refs.L == 64 and refs.max_set == 7 and refs.n_sets == 6
    _check_table(sc, df, [(30,), (21, 5), (7, 5), (11, 11)])
    # scores on this table, the caption of the empty set included (no reference: 0)
    hyps, owner = [[5, 6, 7], [9, 8, 9], [1, 2], [21] * 10, [11, 12, 13], [7, 6, 5, 6]], [0, 1, 2, 3, 4, 5]
    T, lens = _rows(hyps)
    got = sc.score_token_ids(T, torch.tensor(owner), refs, hyp_lens=lens).cpu().numpy()
    want = cider_oracle.corpus(hyps, owner, sets)[1]
    assert want[2] == 0.0 and got[2] == 0.0 and float(np.abs(got - np.asarray(want)).max()) <= TOL
    # the orders below 4 count their own grams only
    sc2, _ = ciderd.DeviceCiderD.from_refs(DEV, sets, n=2)
    df2 = cider_oracle.document_frequency(sets, 2)
    _check_table(sc2, df2, [(5, 6, 7), (1, 2, 3, 4)])


def test_table_of_one_word_references():
    """L = 1, and a unigram that every set holds: df == n_sets"""
    from show_edit_tell_amd import ciderd
    sets = [[[3]], [[3], [4]], [[4], [3], [3]], [[3], [5], [6], [3]]]
    sc, refs = ciderd.DeviceCiderD.from_refs(DEV, sets)
    assert refs.L == 1
    _check_table(sc, {(3,): 4, (4,): 2, (5,): 1, (6,): 1}, [(7,), (3, 3), (3, 4)])
    got = sc.score_token_ids(torch.tensor([[3], [4]]), torch.tensor([0, 1]), refs, hyp_lens=torch.tensor([1, 1]))
    want = cider_oracle.corpus([[3], [4]], [0, 1], sets)[1]
    assert want[0] == 0.0 and want[1] > 0.0 and float(np.abs(got.cpu().numpy() - np.asarray(want)).max()) <= TOL


def test_contention():
    """600 sets x 5 references of 8 ids over 12 words: every unigram and many bigrams are entered by hundreds of waves at once"""
    from show_edit_tell_amd import ciderd
    rng = np.random.default_rng(9)
    sets = [[[int(x) for x in rng.integers(1, 13, 8)] for _ in range(5)] for _ in range(600)]
    df = cider_oracle.document_frequency(sets)
    assert min(df[(w,)] for w in range(1, 13)) > 500 and sum(1 for g, c in df.items() if len(g) == 2 and c > 100) >= 100
    sc, _ = ciderd.DeviceCiderD.from_refs(DEV, sets)
    _check_table(sc, df, [(13,), (0,), (1, 13)])


def test_two_builds_agree(world):
    from show_edit_tell_amd import ciderd
    hyps, sets = cider_oracle.world_sides(world, True)
    grams = sorted(cider_oracle.document_frequency(sets))
    T = torch.from_numpy(world["T"]).to(DEV)
    idx = torch.arange(world["N"], dtype=torch.int32, device=DEV)
    out = []
    for _ in range(2):
        sc, refs = ciderd.DeviceCiderD.from_refs(DEV, world["gt"])
        out.append((_lookup(sc, grams), sc.score_token_ids(T, idx, refs), refs.recs))
    assert out[0][0] == out[1][0]
    assert torch.equal(_bits(out[0][1]), _bits(out[1][1])) and torch.equal(out[0][2], out[1][2])


def test_a_bound_too_small_drops_and_counts(world):
    """gram_bound = 0: a table of two slots.  The two grams that got a slot hold their whole count, every other arrival is
    counted as dropped, and the probes of the full table end."""
    from show_edit_tell_amd import _lib, ciderd
    from show_edit_tell_amd.device_metric import pack_ref_sets
    _, sets = cider_oracle.world_sides(world, True)
    df = cider_oracle.document_frequency(sets)
    sc0, _ = ciderd.DeviceCiderD.from_refs(DEV, world["gt"])              # a scorer object to carry the small table's handle
    tok, ln, off, R, L, max_set = pack_ref_sets(sets, "CIDEr-D", True)
    t, l, o = (torch.from_numpy(x).to(DEV) for x in (tok, ln, off))
    h = C.c_void_p()
    rc = sc0._lib.set_ciderd_device_create_corpus(t.data_ptr(), t.stride(0), l.data_ptr(), R, L, o.data_ptr(), len(sets), max_set, 0, 4,
                                                  6.0, _lib.stream_of(sc0.dev), C.byref(h))
    assert rc == 0 and h.value
    sc0._lib.set_ciderd_device_destroy(sc0._h)
    sc0._h = h
    grams = sorted(df)
    got = _lookup(sc0, grams)
    placed = [(g, c) for g, c in zip(grams, got) if c != 0.0]
    assert len(placed) == 2 and all(c == float(df[g]) for g, c in placed)
    assert sc0.dropped() == sum(df.values()) - sum(int(c) for _, c in placed)


# ---- scores ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_end", [False, True])
def test_scores_against_oracle_and_host_table(world, count_end):
    from show_edit_tell_amd import ciderd
    hyps, sets = cider_oracle.world_sides(world, count_end)
    want_mean, want = cider_oracle.corpus(hyps, range(world["N"]), sets)
    assert 1.0 < want_mean < 8.0
    sc, refs = ciderd.DeviceCiderD.from_refs(DEV, world["gt"], count_end=count_end)
    T = torch.from_numpy(world["T"]).to(DEV)
    idx = torch.arange(world["N"], dtype=torch.int32, device=DEV)
    lens = None if count_end else torch.tensor([len(h) for h in hyps], dtype=torch.int32, device=DEV)
    got = sc.score_token_ids(T, idx, refs, hyp_lens=lens)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (world["N"],)
    err = float(np.abs(got.cpu().numpy() - np.asarray(want)).max())
    print("CIDEr rows (count_end=%s): mean %.6f, max abs err vs oracle %.3e" % (count_end, want_mean, err))
    assert err <= TOL
    mean = sc.corpus_score(T, idx, refs, lens)
    assert mean.is_cuda and mean.dtype == torch.float64 and mean.dim() == 0 and abs(float(mean) - want_mean) <= TOL
    # the host-built table of the same counts: the same bits, records included
    hs = _host_scorer(cider_oracle.document_frequency(sets), len(sets))
    hrefs = hs.prepare_refs(sets)
    assert torch.equal(hrefs.recs, refs.recs)
    assert torch.equal(_bits(hs.score_token_ids(T, idx, hrefs, hyp_lens=lens)), _bits(got))


def test_pins_on_the_device():
    from show_edit_tell_amd import ciderd
    sc, refs = ciderd.DeviceCiderD.from_refs(DEV, [[[1, 2]], [[1, 3]]])
    T, lens = _rows([[1, 2], [1, 3]])
    got = sc.score_token_ids(T, torch.tensor([0, 1]), refs, hyp_lens=lens)
    assert got.cpu().tolist() == [5.0, 5.0] and float(sc.corpus_score(T, torch.tensor([0, 1]), refs, lens)) == 5.0
    sc, refs = ciderd.DeviceCiderD.from_refs(DEV, [[[4, 5, 6], [4, 5]]])
    T, lens = _rows([[4, 5, 6]])
    assert sc.score_token_ids(T, torch.tensor([0]), refs, hyp_lens=lens).cpu().tolist() == [0.0]
    assert float(sc.corpus_score(T[:0], torch.zeros(0, dtype=torch.int32), refs, lens[:0])) == 0.0      # no row: 0


def test_unpackable_id(world):
    """one reference holds the id 65534: its set scores NaN, the corpus value is NaN, and every other row is the oracle's with
    that reference's grams left out of df and N unchanged"""
    from show_edit_tell_amd import ciderd
    hyps, sets = cider_oracle.world_sides(world, True)
    bad_set, bad_ref = 9, 1
    sets = [[list(r) for r in rs] for rs in sets]
    sets[bad_set][bad_ref] = [3, 65534, 4, 0]
    sc, refs = ciderd.DeviceCiderD.from_refs(DEV, sets)
    df = cider_oracle.document_frequency(sets, leave_out={(bad_set, bad_ref)})
    assert (3, 65534) not in df
    grams = sorted(df)
    assert _lookup(sc, grams) == [float(df[g]) for g in grams] and sc.dropped() == 0
    T = torch.from_numpy(world["T"]).to(DEV)
    idx = torch.arange(world["N"], dtype=torch.int32, device=DEV)
    got = sc.score_token_ids(T, idx, refs).cpu().numpy()
    want = np.asarray(cider_oracle.corpus(hyps, range(world["N"]), sets, df=df)[1])
    others = np.arange(world["N"]) != bad_set
    assert math.isnan(got[bad_set]) and not np.isnan(got[others]).any()
    assert float(np.abs(got[others] - want[others]).max()) <= TOL
    assert math.isnan(float(sc.corpus_score(T, idx, refs)))


# ---- evaluate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_end", [False, True])
def test_validation_cider_against_oracle(world, count_end):
    from show_edit_tell_amd import evaluate
    T = torch.from_numpy(world["T"]).to(DEV)
    got = evaluate.validation_cider(T, None, world["gt"], DEV, count_end=count_end)
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
    hyps, sets = cider_oracle.world_sides(world, count_end)
    want = cider_oracle.corpus(hyps, range(world["N"]), sets)[0]
    print("CIDEr %.6f (tensor, count_end=%s), abs err %.3e" % (want, count_end, abs(float(got) - want)))
    assert 1.0 < want < 8.0 and abs(float(got) - want) <= TOL
    got = evaluate.validation_cider(world["lists"], None, world["gt"], DEV, count_end=count_end, word_map=world["wm"])
    want_l = cider_oracle.corpus(cider_oracle.world_sides(world, count_end, lists=True)[0], range(world["N"]), sets)[0]
    assert abs(float(got) - want_l) <= TOL
    assert count_end == (want_l != want)          # the list without <end> and the full row differ only where the 0 counts
    # an explicit set index: the captions in reverse order against the same sets — df and N still come from all sets
    idx = np.arange(world["N"])[::-1].copy()
    got = evaluate.validation_cider(torch.from_numpy(world["T"][idx]).to(DEV), torch.from_numpy(idx).to(DEV), world["gt"], DEV,
                                    count_end=count_end)
    assert abs(float(got) - want) <= TOL
    # a part of the captions: the table is that of the whole corpus
    got = evaluate.validation_cider(T[:7], None, world["gt"], DEV, count_end=count_end)
    assert abs(float(got) - cider_oracle.corpus(hyps[:7], range(7), sets)[0]) <= TOL


@pytest.mark.parametrize("count_end", [False, True])
def test_validation_scores_with_cider(world, count_end):
    from show_edit_tell_amd import evaluate
    keys = ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L"]
    for caps, kw in ((torch.from_numpy(world["T"]).to(DEV), {}), (world["lists"], dict(word_map=world["wm"]))):
        out = evaluate.validation_scores(caps, None, world["gt"], DEV, count_end=count_end, cider=True, **kw)
        assert list(out) == keys + ["CIDEr"]
        b = evaluate.validation_bleu(caps, None, world["gt"], DEV, count_end=count_end, **kw)
        single = {"Bleu_%d" % (k + 1): b[k] for k in range(4)}
        single["ROUGE_L"] = evaluate.validation_rouge_l(caps, None, world["gt"], DEV, count_end=count_end, **kw)
        single["CIDEr"] = evaluate.validation_cider(caps, None, world["gt"], DEV, count_end=count_end, **kw)
        plain = evaluate.validation_scores(caps, None, world["gt"], DEV, count_end=count_end, **kw)
        assert list(plain) == keys
        for k, v in out.items():
            assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 0
            assert torch.equal(_bits(v), _bits(single[k])), k
            assert k == "CIDEr" or torch.equal(_bits(v), _bits(plain[k])), k
        assert float(out["CIDEr"]) > 1.0
