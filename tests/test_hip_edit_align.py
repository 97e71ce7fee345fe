"""GPU: the canonical word alignment on the device (csrc/editdist_device.hip ed_align_k, editdist.DeviceEditDistance
.align_token_ids) against the walk-back through the full table in tests/edit_oracle.py — everything here is an integer, so
equality is asserted throughout — and evaluate.edit_statistics / edit_alignment / validation_edit against the host scorer."""
import numpy as np
import pytest
import torch

import edit_oracle
from hip_adapter import to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77


def _pairs():
    """(src, hyp): every grid and edge hypothesis against the first and the last reference of its set, both ways round, plus an
    empty source, an empty hypothesis, both empty and identical rows"""
    out = []
    for h, R in edit_oracle.grid() + edit_oracle.edge_cases():
        out.append((list(R[0]), list(h)))
        out.append((list(h), list(R[-1])))
    out += [([], [4, 5, 6]), ([4, 5, 6], []), ([], []), ([7, 8, 9, 7], [7, 8, 9, 7]), (list(range(1, 65)), list(range(1, 65)))]
    return out


def _build(zero_rule, L, Ls):
    """the pairs that fit hypothesis rows of L and source rows of Ls ids, as arrays with their expected outputs.  zero_rule: a
    sentence shorter than its row ends with 0 (an empty one is [0]) and rows are cut after it; else explicit lengths with junk
    (0s included) behind them"""
    rng = np.random.default_rng(3 if zero_rule else 4)
    pairs = [(s, h) for s, h in _pairs() if len(h) <= L and len(s) <= Ls]
    if zero_rule:
        end = lambda s, W: [0] if not s else (s[:-1] + [0] if len(s) < W else s)
        pairs = [(end(s, Ls), end(h, L)) for s, h in pairs]
    N = len(pairs)
    H, S = np.zeros((N, L), dtype=np.int64), np.zeros((N, Ls), dtype=np.int64)
    want = dict(stats=np.zeros((N, 8), dtype=np.int64), hyp_ops=np.zeros((N, L), dtype=np.int64),
                hyp_src=np.full((N, L), -1, dtype=np.int64), src_ops=np.zeros((N, Ls), dtype=np.int64))
    for i, (s, h) in enumerate(pairs):
        H[i, :len(h)], S[i, :len(s)] = h, s
        if not zero_rule:
            H[i, len(h):], S[i, len(s):] = rng.integers(0, 7, L - len(h)), rng.integers(0, 7, Ls - len(s))
        ho, hs, so, _ = edit_oracle.script(s, h)
        want["stats"][i] = edit_oracle.align_stats(s, h)
        want["hyp_ops"][i, :len(h)], want["hyp_src"][i, :len(h)], want["src_ops"][i, :len(s)] = ho, hs, so
    if zero_rule:
        assert all(edit_oracle.cut_after_zero(H[i]) == pairs[i][1] and edit_oracle.cut_after_zero(S[i]) == pairs[i][0] for i in range(N))
    st = want["stats"]
    assert N >= 25 and (st[:, 7] == 1).sum() >= 3                  # unchanged rows in every world
    if L == 64 and Ls == 64:                                       # the full world: all four operations in one script, often
        assert N >= 400 and (st[:, 3:7] > 0).all(1).sum() >= 20
    lens = None if zero_rule else (np.array([len(h) for _, h in pairs], dtype=np.int32), np.array([len(s) for s, _ in pairs], dtype=np.int32))
    return dict(pairs=pairs, H=H, S=S, lens=lens, want=want, N=N)


@pytest.fixture(scope="module")
def scorer():
    from show_edit_tell_amd import editdist
    return editdist.DeviceEditDistance(DEV)


@pytest.mark.parametrize("dims", [(64, 64), (20, 64), (64, 20), (7, 2)])
@pytest.mark.parametrize("zero_rule", [True, False])
def test_alignment_against_the_canonical_script(scorer, zero_rule, dims):
    w = _build(zero_rule, *dims)
    hl, sl = (None, None) if w["lens"] is None else w["lens"]
    stats, hyp_ops, hyp_src, src_ops = scorer.align_token_ids(to_dev(w["H"]), to_dev(w["S"]), hl, sl)
    assert (stats.dtype, hyp_ops.dtype, hyp_src.dtype, src_ops.dtype) == (torch.int32, torch.int8, torch.int32, torch.int8)
    assert all(t.is_cuda for t in (stats, hyp_ops, hyp_src, src_ops))
    N, (L, Ls) = w["N"], dims
    assert (tuple(stats.shape), tuple(hyp_ops.shape), tuple(hyp_src.shape), tuple(src_ops.shape)) == ((N, 8), (N, L), (N, L), (N, Ls))
    st = stats.cpu().numpy().astype(np.int64)
    assert np.array_equal(st, w["want"]["stats"])
    assert np.array_equal(hyp_ops.cpu().numpy(), w["want"]["hyp_ops"])
    assert np.array_equal(hyp_src.cpu().numpy(), w["want"]["hyp_src"])
    assert np.array_equal(src_ops.cpu().numpy(), w["want"]["src_ops"])
    # the identities on every row, and nothing beyond the lengths
    dist, len_h, len_s, keep, sub, ins, dele, same = st.T
    assert (keep + sub + ins == len_h).all() and (keep + sub + dele == len_s).all() and (sub + ins + dele == dist).all()
    assert ((dist == 0) == (same == 1)).all()
    ho, hs, so = hyp_ops.cpu().numpy(), hyp_src.cpu().numpy(), src_ops.cpu().numpy()
    beyond_h, beyond_s = np.arange(L)[None, :] >= len_h[:, None], np.arange(Ls)[None, :] >= len_s[:, None]
    assert (ho[beyond_h] == 0).all() and (hs[beyond_h] == -1).all() and (so[beyond_s] == 0).all()
    assert (ho[~beyond_h] > 0).all() and (so[~beyond_s] > 0).all()


def test_memory_contract_and_launch_independence(scorer):
    """strided inputs and outputs with sentinels between the rows and guard words around every output: only stats[i, 0..8),
    hyp_ops / hyp_src[i, 0..L) and src_ops[i, 0..src_L) are written; a row alone has the bits it has in the batch"""
    from show_edit_tell_amd import _lib
    w = _build(False, 20, 64)
    N, L, Ls, G = w["N"], 20, 64, 16
    ld_h, ld_s, ld_o, ld_so = 27, 70, 23, 66

    def wide(A, ld):
        buf = torch.full((A.shape[0], ld), 3, dtype=torch.int64, device=DEV)
        buf[:, :A.shape[1]] = to_dev(A)
        return buf
    H, S = wide(w["H"], ld_h), wide(w["S"], ld_s)
    hl, sl = (to_dev(x) for x in w["lens"])

    def run(rows):
        n = rows.stop - rows.start
        bufs = [torch.full((m + 2 * G,), SENT, dtype=dt, device=DEV) for m, dt in
                ((n * 8, torch.int32), (n * ld_o, torch.int8), (n * ld_o, torch.int32), (n * ld_so, torch.int8))]
        st, ho, hs, so = (b[G:] for b in bufs)
        rc = scorer._lib.set_edit_device_align(H[rows].data_ptr(), ld_h, hl[rows].data_ptr(), n, L, S[rows].data_ptr(), ld_s,
                                               sl[rows].data_ptr(), Ls, st.data_ptr(), ho.data_ptr(), ld_o, hs.data_ptr(),
                                               so.data_ptr(), ld_so, _lib.stream_of(scorer.dev))
        _lib.check(rc, "set_edit_device_align")
        out = []
        for b, m in zip(bufs, (n * 8, n * ld_o, n * ld_o, n * ld_so)):
            b = b.cpu()
            assert (b[:G] == SENT).all() and (b[G + m:] == SENT).all()
            out.append(b[G:G + m])
        return out[0].view(n, 8), out[1].view(n, ld_o), out[2].view(n, ld_o), out[3].view(n, ld_so)
    st, ho, hs, so = run(slice(0, N))
    assert (ho[:, L:] == SENT).all() and (hs[:, L:] == SENT).all() and (so[:, Ls:] == SENT).all()
    assert np.array_equal(st.numpy(), w["want"]["stats"]) and np.array_equal(ho[:, :L].numpy(), w["want"]["hyp_ops"])
    assert np.array_equal(hs[:, :L].numpy(), w["want"]["hyp_src"]) and np.array_equal(so[:, :Ls].numpy(), w["want"]["src_ops"])
    for i in (0, 1, N // 2, N - 1):
        one = run(slice(i, i + 1))
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one, (st, ho, hs, so))), i


def test_the_id_limit_and_limits(scorer):
    from show_edit_tell_amd._lib import SetError
    big, over = 65533, 65534
    H = to_dev(np.array([[1, big, 3], [1, over, 3], [1, 2, 3], [1, 2, over]], dtype=np.int64))
    S = to_dev(np.array([[big, 3], [1, 3], [over, 3], [1, 2]], dtype=np.int64))
    stats, ho, hs, so = scorer.align_token_ids(H, S, [3, 3, 3, 2], [2, 2, 2, 2])
    assert stats.cpu().tolist() == [[1, 3, 2, 2, 0, 1, 0, 0], [-1] * 8, [-1] * 8, [0, 2, 2, 2, 0, 0, 0, 1]]
    assert ho.cpu().tolist() == [[3, 1, 1], [0, 0, 0], [0, 0, 0], [1, 1, 0]]
    assert hs.cpu().tolist() == [[-1, 0, 1], [-1, -1, -1], [-1, -1, -1], [0, 1, -1]]
    assert so.cpu().tolist() == [[1, 1], [0, 0], [0, 0], [1, 1]]
    with pytest.raises(SetError):
        scorer.align_token_ids(torch.zeros(2, 65, dtype=torch.int64, device=DEV), torch.zeros(2, 5, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        scorer.align_token_ids(torch.zeros(2, 5, dtype=torch.int64, device=DEV), torch.zeros(3, 5, dtype=torch.int64, device=DEV))
    out = scorer.align_token_ids(torch.zeros(0, 5, dtype=torch.int64, device=DEV), torch.zeros(0, 7, dtype=torch.int64, device=DEV))
    assert [tuple(t.shape) for t in out] == [(0, 8), (0, 5), (0, 5), (0, 7)]


# ---- evaluate.edit_statistics / edit_alignment / validation_edit -----------------------------------------------------------
def _toy():
    """a toy vocabulary and six (previous caption, output) rows in the vocabulary's convention: unchanged, one substitution,
    an insertion and a deletion, a rewrite, an output that never ended, an empty input"""
    wm = {"<pad>": 0, "<unk>": 1, "<start>": 2, "<end>": 3}
    wm.update({"w%d" % k: k for k in range(4, 40)})
    S, E, P = wm["<start>"], wm["<end>"], wm["<pad>"]
    prev = [[S, 5, 6, 7, 8, E], [S, 5, 6, 7, 8, E], [S, 5, 6, 7, 8, 9, E], [S, 10, 11, E], [S, 5, 6, E], [S, E]]
    outs = [[S, 5, 6, 7, 8, E], [S, 5, 6, 30, 8, E], [S, 5, 31, 6, 7, 9, E], [S, 20, 21, 22, 23, E], [S, 5, 6, 7, 8, 9, 10, 11], [S, 12, E]]
    Lp = 9
    prev_t = torch.tensor([c + [P] * (Lp - len(c)) for c in prev])
    plen = torch.tensor([[len(c)] for c in prev])
    return wm, prev, outs, prev_t, plen


def _norm(c, wm, count_end):
    c = [0 if w == wm["<end>"] else w for w in c if w not in (wm["<start>"], wm["<pad>"])]
    return c[:c.index(0) + (1 if count_end else 0)] if 0 in c else c


@pytest.mark.parametrize("count_end", [False, True])
def test_edit_statistics_and_alignment(count_end):
    from show_edit_tell_amd import editdist, evaluate
    wm, prev, outs, prev_t, plen = _toy()
    B = len(prev)
    src, hyp = [_norm(c, wm, count_end) for c in prev], [_norm(c, wm, count_end) for c in outs]
    want = np.array([edit_oracle.align_stats(s, h) for s, h in zip(src, hyp)])
    assert want[:, 7].tolist() == [1, 0, 0, 0, 0, 0] and want[1, 4] == 1 and want[2, 5] == 1 and want[2, 6] == 1
    # the decoder's tensor form: ids with 0 = <end> and zeros behind it (the row that never ended fills its 7 columns); it
    # stays on the device
    L = 7
    seq = torch.zeros(B, L, dtype=torch.int64)
    for i, c in enumerate(outs):
        ids = [0 if w == wm["<end>"] else w for w in c[1:]]
        seq[i, :len(ids)] = torch.tensor(ids)
    seq_d = to_dev(seq)
    by_tensor = evaluate.edit_statistics(to_dev(prev_t), to_dev(plen), seq_d, wm, DEV, count_end)
    by_list = evaluate.edit_statistics(prev_t, plen, outs, wm, DEV, count_end)
    host = editdist.EditDistance().align_token_ids(
        np.array([h + [0] * (L - len(h)) for h in hyp]), np.array([s + [0] * (9 - len(s)) for s in src]),
        hyp_lens=[len(h) for h in hyp], src_lens=[len(s) for s in src])[0]
    assert np.array_equal(host, want)
    for k, c in (("dist", 0), ("keep", 3), ("sub", 4), ("ins", 5), ("del", 6), ("unchanged", 7)):
        assert by_tensor[k].is_cuda and by_tensor[k].dtype == torch.int32
        assert by_tensor[k].cpu().tolist() == want[:, c].tolist() == by_list[k].cpu().tolist(), k
    words = want[:, 2].sum()
    scal = {"unchanged_frac": want[:, 7].mean(), "mean_dist": want[:, 0].mean(), "edit_rate": want[:, 0].sum() / words}
    for k, v in scal.items():
        assert by_tensor[k].is_cuda and by_tensor[k].dtype == torch.float64 and by_tensor[k].dim() == 0
        assert abs(float(by_tensor[k]) - v) <= 1e-15 and torch.equal(by_tensor[k], by_list[k]), k
    # the alignment: the same tensors from both forms, and rows() in words
    a, b = evaluate.edit_alignment(to_dev(prev_t), to_dev(plen), seq_d, wm, DEV, count_end), \
        evaluate.edit_alignment(prev_t, plen, outs, wm, DEV, count_end)
    assert np.array_equal(a.stats.cpu().numpy(), want) and torch.equal(a.stats, b.stats)
    for i, (s, h) in enumerate(zip(src, hyp)):
        ho, hs, so, _ = edit_oracle.script(s, h)
        for t in (a, b):
            assert t.hyp_ops[i, :len(h)].cpu().tolist() == ho and t.hyp_src[i, :len(h)].cpu().tolist() == hs
            assert t.src_ops[i, :len(s)].cpu().tolist() == so
            assert not t.hyp_ops[i, len(h):].any() and not t.src_ops[i, len(s):].any() and (t.hyp_src[i, len(h):] == -1).all()
    rows = a.rows(wm)
    assert rows == b.rows(wm) and len(rows) == B
    end = [("<end>", "keep", "<end>")] if count_end else []
    assert rows[0] == ([("w5", "keep", "w5"), ("w6", "keep", "w6"), ("w7", "keep", "w7"), ("w8", "keep", "w8")] + end, [])
    assert rows[1] == ([("w5", "keep", "w5"), ("w6", "keep", "w6"), ("w30", "substitute", "w7"), ("w8", "keep", "w8")] + end, [])
    assert rows[2] == ([("w5", "keep", "w5"), ("w31", "insert", None), ("w6", "keep", "w6"), ("w7", "keep", "w7"),
                        ("w9", "keep", "w9")] + end, ["w8"])
    assert rows[5] == ([("w12", "insert", None)] + end, [])


def test_edit_statistics_of_nothing():
    from show_edit_tell_amd import evaluate
    wm = _toy()[0]
    st = evaluate.edit_statistics(torch.zeros(0, 5, dtype=torch.int64), None, torch.zeros(0, 6, dtype=torch.int64, device=DEV), wm, DEV)
    assert tuple(st["dist"].shape) == (0,) and float(st["unchanged_frac"]) == 0.0 and float(st["edit_rate"]) == 0.0


@pytest.mark.parametrize("count_end", [False, True])
def test_validation_edit_against_the_host_scorer(count_end):
    from show_edit_tell_amd import editdist, evaluate
    from show_edit_tell_amd.device_metric import strip_end
    rng = np.random.default_rng(21)
    N, L = 40, 16
    gt = [[[int(x) for x in rng.integers(1, 12, int(rng.integers(3, 12)))] + [0] for _ in range(int(rng.integers(1, 6)))] for _ in range(N)]
    H = np.zeros((N, L), dtype=np.int64)
    for i in range(N):
        c = [w for w in gt[i][int(rng.integers(0, len(gt[i])))] if w]
        c[int(rng.integers(0, len(c)))] = int(rng.integers(1, 12))
        if i % 3 == 0:
            c = c[1:]
        H[i, :len(c)] = c
    if count_end:
        want = editdist.EditDistance().corpus_score(H, np.arange(N), gt)
    else:
        lens = [int(np.flatnonzero(r == 0)[0]) for r in H]
        want = editdist.EditDistance().corpus_score(H, np.arange(N), strip_end(gt), hyp_lens=lens)
    got = evaluate.validation_edit(to_dev(H), None, gt, DEV, count_end=count_end)
    assert sorted(got) == ["similarity", "wer"] and 0.05 < want["wer"] < 0.6 and 0.4 < want["similarity"] < 1.0
    for k in got:
        assert got[k].is_cuda and got[k].dim() == 0 and abs(float(got[k]) - want[k]) <= 1e-12, k
