"""CPU: what the device metrics share on the Python side (device_metric.py): the flattening of reference sets into one padded
upload under both length conventions, its refusals with each metric's message, the one prepared-reference class under both of
its names, the one definition of the four device scorers' front and of the three host scorers' front, and the refusal of a CPU
device by every device scorer."""
import numpy as np
import pytest

SETS = [[[5, 6, 0, 9], [7, 0]], [[3, 3, 3]], [[0, 4], [], [1, 2, 3, 4, 0, 0]]]      # 0 inside, at the end, in front, none; empty


def test_pack_after_zero_and_before_zero():
    from show_edit_tell_amd import bleu, device_metric as M
    assert bleu.strip_end is M.strip_end
    after = [[M.cut_after_zero(c) for c in refs] for refs in SETS]
    assert after == [[[5, 6, 0], [7, 0]], [[3, 3, 3]], [[0], [], [1, 2, 3, 4, 0]]]
    before = M.strip_end(SETS)
    assert before == [[[5, 6], [7]], [[3, 3, 3]], [[], [], [1, 2, 3, 4]]]
    for sets, L in ((after, 5), (before, 4)):
        tok, lens, off, R, got_L, max_set = M.pack_ref_sets(sets, "BLEU", False)
        flat = [c for refs in sets for c in refs]
        assert (R, got_L, max_set) == (6, L, 3)
        assert tok.dtype == np.int64 and tok.shape == (6, L) and tok.flags["C_CONTIGUOUS"]
        assert lens.dtype == np.int32 and lens.tolist() == [len(c) for c in flat]
        assert off.dtype == np.int64 and off.tolist() == [0, 2, 3, 6]
        for i, c in enumerate(flat):
            assert tok[i, :len(c)].tolist() == c and not tok[i, len(c):].any()
    assert M.cut_after_zero(np.array([4, 0, 0])) == [4, 0] and type(M.cut_after_zero(np.array([4]))[0]) is int


def test_empty_set_allowed_and_refused():
    from show_edit_tell_amd import device_metric as M
    sets = [[[1, 0]], [], [[2, 0], [3, 4, 0]]]
    tok, lens, off, R, L, max_set = M.pack_ref_sets(sets, "CIDEr-D", True)
    assert (R, L, max_set) == (3, 3, 2) and off.tolist() == [0, 1, 1, 3] and lens.tolist() == [2, 2, 3]
    with pytest.raises(ValueError) as e:
        M.pack_ref_sets(sets, "BLEU", False)
    assert str(e.value) == "reference set 1 is empty: BLEU needs at least one reference per hypothesis"


def test_no_reference_at_all_keeps_one_padded_row():
    from show_edit_tell_amd import device_metric as M
    for sets, n_sets in (([], 0), ([[], []], 2)):
        tok, lens, off, R, L, max_set = M.pack_ref_sets(sets, "CIDEr-D", True)
        assert (R, L, max_set) == (0, 1, 0)
        assert tok.shape == (1, 1) and lens.shape == (1,) and not tok.any() and not lens.any()      # valid pointers
        assert off.tolist() == [0] * (n_sets + 1)
    tok, lens, off, R, L, max_set = M.pack_ref_sets([[[]]], "BLEU", False)                          # one reference of no ids
    assert (R, L, max_set) == (1, 1, 1) and lens.tolist() == [0] and off.tolist() == [0, 1]


def test_reference_of_65_ids_is_refused_with_the_metric_name():
    from show_edit_tell_amd import device_metric as M
    assert (M.DEVICE_MAX_LEN, M.DEVICE_PACK_LIMIT) == (64, 65534)
    ok = [[[1] * 64]]
    assert M.pack_ref_sets(ok, "BLEU", False)[4] == 64
    long = [[[1, 0]], [[1] * 65]]
    for name, allow in (("CIDEr-D", True), ("BLEU", False)):
        with pytest.raises(ValueError) as e:
            M.pack_ref_sets(long, name, allow)
        assert str(e.value) == "a reference of 65 ids: the device %s scorer takes at most 64" % name


def test_one_prepared_refs_class_and_limits_under_both_names():
    from show_edit_tell_amd import bleu, ciderd, device_metric as M
    assert ciderd.PreparedRefs is bleu.PreparedBleuRefs is M.PreparedRefs
    p = ciderd.PreparedRefs("r", 5, 6, "o", 3, 2)
    assert (p.recs, p.L, p.n_refs, p.set_off, p.n_sets, p.max_set) == ("r", 5, 6, "o", 3, 2)
    assert isinstance(p, bleu.PreparedBleuRefs)
    assert ciderd.DEVICE_PACK_LIMIT == bleu.DEVICE_PACK_LIMIT == 65534 and ciderd.DEVICE_MAX_LEN == bleu.DEVICE_MAX_LEN == 64
    from show_edit_tell_amd import editdist, rouge
    record_based = (bleu.DeviceBleu, rouge.DeviceRougeL, editdist.DeviceEditDistance)
    for cls in (ciderd.DeviceCiderD,) + record_based:                      # one definition of the tensor plumbing
        assert issubclass(cls, M.DeviceSentenceScorer)
        assert cls._tokens is M.DeviceSentenceScorer._tokens and cls._i32 is M.DeviceSentenceScorer._i32
        assert cls._self_refs is M.DeviceSentenceScorer._self_refs and cls._score_rows is M.DeviceSentenceScorer._score_rows
        assert cls.pair_scores is M.DeviceSentenceScorer.pair_scores
    for cls in record_based:                                               # one definition of the record-based scorer
        assert issubclass(cls, M.RecordScorer)
        for name in ("_prepare", "prepare_refs", "pair_scores", "score_token_ids"):
            assert getattr(cls, name) is getattr(M.RecordScorer, name), (cls, name)
    assert len({cls.SCORE_ENTRY for cls in record_based}) == 3


def test_host_scorers_cut_rows_in_one_place():
    from show_edit_tell_amd import bleu, device_metric as M, editdist, rouge
    hosts = (bleu.Bleu(), rouge.RougeL(), editdist.EditDistance())
    for h in hosts:
        assert isinstance(h, M.HostSentenceScorer)
        assert type(h).score_token_ids is M.HostSentenceScorer.score_token_ids
        assert type(h)._score_lists is M.HostSentenceScorer._score_lists
    rows = np.array([[4, 5, 0, 6], [7, 0, 8, 9], [1, 2, 3, 4]])            # 3 rows, L = 4
    assert M.id_rows(rows, [-3, 2, 9], "hyp_lens") == [[], [7, 0], [1, 2, 3, 4]]      # clamped to [0, L]
    assert M.id_rows(rows, None, "hyp_lens") == [[4, 5, 0], [7, 0], [1, 2, 3, 4]]     # the 0 rule: the 0 stays
    refs = [[[4, 5, 0]], [[7, 0], [1, 2, 3, 4]]]
    for lens, want in (([-3, 2, 9], [0, 2, 4]), (None, [3, 2, 4])):
        got = [h.score_token_ids(rows, [0, 1, 1], refs, hyp_lens=lens)[0] for h in hosts]
        assert got[0][:, 8].tolist() == got[1][:, 1].tolist() == got[2][:, 1].tolist() == want      # the length each one saw
    for h in hosts:
        with pytest.raises(ValueError) as e:
            h.score_token_ids(rows, [0, 1], refs)
        assert str(e.value) == "hyp_set has 2 entries for 3 sentences"
        with pytest.raises(ValueError) as e:
            h.score_token_ids(rows, [0, 1, 1], refs, hyp_lens=[1, 2])
        assert str(e.value) == "hyp_lens has 2 entries for 3 sentences"
        with pytest.raises(ValueError) as e:                               # both sizes wrong: each scorer names what it always named
            h.score_token_ids(rows, [0, 1], refs, hyp_lens=[1, 2, 3, 4])
        assert str(e.value) == ("hyp_lens has 4 entries for 3 sentences" if isinstance(h, editdist.EditDistance)
                                else "hyp_set has 2 entries for 3 sentences")
        with pytest.raises(ValueError) as e:
            h.score_token_ids(rows[0], [0], refs)
        assert str(e.value) == "sentences are rows of a 2-D id array, got shape (4,)"


def test_both_scorers_refuse_cpu_with_their_messages():
    from show_edit_tell_amd import bleu, ciderd
    from show_edit_tell_amd._lib import SetError
    with pytest.raises(SetError) as e:
        ciderd.CiderD({("1",): 1}, 2).device("cpu")
    assert str(e.value) == "the device CIDEr-D scorer needs a GPU device, got cpu"
    with pytest.raises(SetError) as e:
        bleu.DeviceBleu("cpu")
    assert str(e.value) == "the device BLEU scorer needs a GPU device, got cpu"
    with pytest.raises(SetError) as e:
        bleu.device_scorer("cpu")
    assert str(e.value) == "the device BLEU scorer needs a GPU device, got cpu"
    from show_edit_tell_amd import editdist, rouge
    for make, name in ((rouge.DeviceRougeL, "ROUGE-L"), (rouge.device_scorer, "ROUGE-L"), (editdist.DeviceEditDistance, "edit distance"),
                       (editdist.device_scorer, "edit distance")):
        with pytest.raises(SetError) as e:
            make("cpu")
        assert str(e.value) == "the device %s scorer needs a GPU device, got cpu" % name
