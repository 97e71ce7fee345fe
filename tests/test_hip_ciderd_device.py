"""GPU: CIDEr-D on the device (csrc/ciderd_device.hip, ciderd.DeviceCiderD) against the project's pure-Python statement of the
metric (CiderD.score, pinned to hand-stated values by tests/test_ciderd.py): the table, scores at every length / set-size edge,
launch independence and the memory contract, the self-critical reward, the SCST steps with reward="device" and the consensus
rerank.

Tolerance of a score: scores lie in [0, 10] and are sums of fewer than 4 * |set| * 64 products computed in double with a few
ulp of error each, which bounds the absolute error near 2e-11; 1e-9 is asserted.  Rewards are float32: 2 ulp of 10 (1.9e-6)."""
import json
import os

import numpy as np
import pytest
import torch

from hip_adapter import dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, TOL_REWARD = 1e-9, 1.9e-6
SENTINEL = -12345.678
MEASURED = {}


def _report(name, value):
    """the measured maxima, printed and (SET_CIDERD_ERRORS_OUT=file) collected for profiles/ciderd_device_errors.json"""
    MEASURED[name] = max(float(value), MEASURED.get(name, 0.0))
    print("measured %s = %.3e" % (name, value))
    out = os.environ.get("SET_CIDERD_ERRORS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _s(ids):
    from show_edit_tell_amd import ciderd
    return ciderd.tokens_to_str(ids) if len(ids) else ""


def _cut(row):
    row = [int(w) for w in row]
    return row[:row.index(0) + 1] if 0 in row else row


@pytest.fixture(scope="module")
def world():
    """Vocabulary of 58 words (ids 1..57 and 0 = <end>; 58 and 59 never occur in the corpus), 40 documents for the df table,
    the reference sets under test (0, 1, 5 and 7 references, references of length 0 and 64) and 257 hypotheses."""
    from show_edit_tell_amd import ciderd
    rng = np.random.default_rng(11)

    def sent(n):                                   # n words and the <end>
        return [int(w) for w in rng.integers(1, 58, n)] + [0]

    corpus = [[sent(int(rng.integers(2, 12))) for _ in range(5)] for _ in range(40)]
    sets = [[], [sent(7)], [sent(int(rng.integers(3, 15))) for _ in range(5)], [sent(int(rng.integers(1, 20))) for _ in range(7)],
            [[], sent(63), [int(w) for w in rng.integers(1, 58, 64)], sent(9)]]
    corpus += [s for s in sets if s]
    df, docs = ciderd.document_frequency([[_s(c) for c in refs] for refs in corpus])
    assert df[("0",)] == docs                      # every document holds the <end>: a table entry with df == ref_len, weight 0
    hyps = []
    for ln in (1, 2, 3, 4, 5, 19, 63, 64):         # ln ids: ln - 1 words and the 0
        hyps.append(sent(ln - 1))
    hyps.append([int(w) for w in rng.integers(1, 58, 64)])      # no 0: the whole row
    hyps.append([0, 5, 6, 7])                                   # starts with 0: one word, the rest is ignored
    hyps.append([9] * 10 + [0])                                 # tf > 1
    hyps.append([58, 59, 58, 59, 3, 0])                         # grams the table never saw
    rows, set_of = [], []
    for s in range(len(sets)):                                  # every edge hypothesis against every set
        for h in hyps:
            rows.append(h)
            set_of.append(s)
    k = 0
    while len(rows) < 257:                                      # near-copies of references: many shared grams, clipped counts
        s = 1 + k % 4
        ref = list(sets[s][k % len(sets[s])])
        base = [w for w in ref if w != 0][:40] or [3]
        for _ in range(int(rng.integers(0, 4))):
            base[int(rng.integers(0, len(base)))] = int(rng.integers(1, 58))
        if k % 5 == 0:
            base = base + base[:3]
        rows.append(base + [0])
        set_of.append(s)
        k += 1
    # a repeated word that the references hold too: min(g_h, g_r) clips
    rows[256], set_of[256] = [sets[1][0][0]] * 6 + [0], 1
    H = np.zeros((257, 64), dtype=np.int64)
    for i, r in enumerate(rows):
        H[i, :len(r)] = r
    return dict(df=df, docs=docs, sets=sets, H=H, set_of=np.asarray(set_of, dtype=np.int32))


@pytest.fixture(scope="module")
def scorers(world):
    from show_edit_tell_amd import ciderd
    return {n: ciderd.CiderD(world["df"], world["docs"], n=n) for n in (4, 2)}


@pytest.fixture(scope="module")
def reference(world, scorers):
    """CiderD.score of every hypothesis against its set, computed once: {n: (257,) float64}"""
    out = {}
    for n, sc in scorers.items():
        out[n] = np.array([sc.score(_s(_cut(world["H"][i])), [_s(_cut(c)) for c in world["sets"][world["set_of"][i]]])
                           for i in range(257)])
    assert out[4].max() > 1.0 and (out[4] > 0).sum() > 100     # the comparison is not one of zeros
    return out


def test_table_lookup():
    """a few thousand distinct grams, entries == capacity / 2 (probe chains exist): every stored count comes back, absent keys
    (ids 0 and 65533 among them) give 0"""
    from show_edit_tell_amd import ciderd
    rng = np.random.default_rng(5)
    grams = set()
    while len(grams) < 2048:
        k = int(rng.integers(1, 5))
        grams.add(tuple(str(int(w)) for w in rng.integers(1, 60, k)))
    grams = sorted(grams)
    df = {g: float(i % 37 + 1) for i, g in enumerate(grams)}
    df[("dog",)] = 3.0                              # dropped: not part of the 2048
    dsc = ciderd.CiderD(df, 100).device(DEV)
    assert dsc.n_entries == 2048                    # capacity 4096: half full
    keys = [ciderd.pack_key([int(w) for w in g]) for g in grams]
    # the chains: at least one key does not sit in its home slot (same hash as the library: ciderd_host.hip U64Hash)
    def home(x):
        m = (1 << 64) - 1
        x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & m; x ^= x >> 27; x = x * 0x94D049BB133111EB & m
        return (x ^ (x >> 31)) & 4095
    assert len({home(k) for k in keys}) < len(keys)
    got = dsc.lookup(keys).cpu().numpy()
    assert np.array_equal(got, np.array([df[g] for g in grams]))
    absent = [ciderd.pack_key([0]), ciderd.pack_key([65533]), ciderd.pack_key([0, 65533, 0, 65533]), ciderd.pack_key([65533] * 4)]
    have = set(keys)
    while len(absent) < 1000:
        k = ciderd.pack_key([int(w) for w in rng.integers(0, 65534, int(rng.integers(1, 5)))])
        if k not in have:
            absent.append(k)
    assert not dsc.lookup(absent).cpu().numpy().any()
    assert dsc.lookup([0]).item() == 0.0


@pytest.mark.parametrize("n", [4, 2])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_scores_against_python(world, scorers, reference, n, N):
    dsc = scorers[n].device(DEV)
    assert scorers[n].device(DEV) is dsc                        # cached per device
    refs = dsc.prepare_refs(world["sets"])
    assert (refs.n_sets, refs.n_refs, refs.max_set, refs.L) == (5, 17, 7, 64)
    # N = 5: the length-64 hypothesis against each of the five sets; N = 1: the length-19 one against the set of 5
    rows = np.arange(257) if N == 257 else np.arange(5) * 12 + 7 if N == 5 else np.array([2 * 12 + 5])
    got = dsc.score_token_ids(to_dev(world["H"][rows]), world["set_of"][rows], refs).cpu().numpy()
    err = np.abs(got - reference[n][rows]).max()
    _report("score_abs_err_n%d" % n, err)
    assert err <= TOL, (err, int(np.abs(got - reference[n][rows]).argmax()))


def test_short_rows_and_explicit_lengths(world, scorers, reference):
    """the same hypotheses as (N, 20) rows where they fit, and with explicit lengths instead of the 0 rule"""
    dsc = scorers[4].device(DEV)
    refs = dsc.prepare_refs(world["sets"])
    lens = np.array([len(_cut(r)) for r in world["H"]])
    fit = np.nonzero(lens <= 20)[0]
    got = dsc.score_token_ids(to_dev(world["H"][fit, :20]), world["set_of"][fit], refs).cpu().numpy()
    assert np.abs(got - reference[4][fit]).max() <= TOL
    junk = world["H"].copy()
    for i, l in enumerate(lens):
        junk[i, l:] = 7                                           # what lies behind the length is not read as words
    got = dsc.score_token_ids(to_dev(junk), world["set_of"], refs, hyp_lens=lens).cpu().numpy()
    assert np.abs(got - reference[4]).max() <= TOL


def test_pair_scores_against_single_references(world, scorers):
    sc = scorers[4]
    dsc = sc.device(DEV)
    refs = dsc.prepare_refs(world["sets"])
    rows = np.arange(0, 257, 3)
    s, pairs = dsc.score_token_ids(to_dev(world["H"][rows]), world["set_of"][rows], refs, return_pairs=True)
    pairs = pairs.cpu().numpy()
    assert pairs.shape == (len(rows), 7)
    err = 0.0
    for a, i in enumerate(rows):
        rs = world["sets"][world["set_of"][i]]
        want = [sc.score(_s(_cut(world["H"][i])), [_s(_cut(c))]) for c in rs]
        err = max([err] + [abs(pairs[a, r] - w) for r, w in enumerate(want)])
        assert not pairs[a, len(rs):].any()                       # beyond the set: the zeros of the allocation
    _report("pair_abs_err", err)
    assert err <= TOL


def _raw_score(dsc, H, set_of, refs, scores, pairs, pair_ld):
    from show_edit_tell_amd import _lib
    rc = dsc._lib.set_ciderd_device_score(dsc._h, H.data_ptr(), H.stride(0), None, H.shape[0], H.shape[1], set_of.data_ptr(),
                                          refs.recs.data_ptr(), refs.L, refs.n_refs, refs.set_off.data_ptr(), refs.n_sets,
                                          refs.max_set, scores.data_ptr(), None if pairs is None else pairs.data_ptr(), pair_ld,
                                          _lib.stream_of(dsc.dev))
    _lib.check(rc, "set_ciderd_device_score")


def test_launch_independence_and_guards(world, scorers):
    """row i alone, in the batch of 257 and in a second run: the same bits; only scores[0..N) and pair_scores[i, r < |set|] are
    written (guard words around both, the tail of short sets, the pair row of a refused set index)"""
    dsc = scorers[4].device(DEV)
    refs = dsc.prepare_refs(world["sets"])
    H, so = to_dev(world["H"]), to_dev(world["set_of"])
    N, G, ld = 257, 8, 9
    runs = []
    for _ in range(2):
        sbuf = torch.full((N + 2 * G,), SENTINEL, dtype=torch.float64, device=DEV)
        pbuf = torch.full((N * ld + 2 * G,), SENTINEL, dtype=torch.float64, device=DEV)
        _raw_score(dsc, H, so, refs, sbuf[G:], pbuf[G:], ld)
        runs.append((sbuf.cpu(), pbuf.cpu()))
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
    assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64))
    sbuf, pbuf = runs[0]
    assert (sbuf[:G] == SENTINEL).all() and (sbuf[G + N:] == SENTINEL).all()
    assert (pbuf[:G] == SENTINEL).all() and (pbuf[G + N * ld:] == SENTINEL).all()
    P = pbuf[G:G + N * ld].view(N, ld)
    size = torch.tensor([len(world["sets"][s]) for s in world["set_of"]])
    written = torch.arange(ld)[None, :] < size[:, None]
    assert (P[~written] == SENTINEL).all() and torch.isfinite(P[written]).all() and (P[written] != SENTINEL).all()
    assert torch.isfinite(sbuf[G:G + N]).all()
    for i in (0, 7, 19, 100, 256):
        one_s = torch.full((1 + 2 * G,), SENTINEL, dtype=torch.float64, device=DEV)
        one_p = torch.full((ld + 2 * G,), SENTINEL, dtype=torch.float64, device=DEV)
        _raw_score(dsc, H[i:i + 1], so[i:i + 1], refs, one_s[G:], one_p[G:], ld)
        assert torch.equal(one_s.cpu()[G:G + 1].view(torch.int64), sbuf[G + i:G + i + 1].view(torch.int64)), i
        assert torch.equal(one_p.cpu()[G:G + ld].view(torch.int64), P[i].contiguous().view(torch.int64)), i
    # a set index outside [0, n_sets): NaN in its score, nothing else
    bad = torch.tensor([2, -1, 5, 3], dtype=torch.int32, device=DEV)
    sbuf = torch.full((4 + 2 * G,), SENTINEL, dtype=torch.float64, device=DEV)
    pbuf = torch.full((4 * ld + 2 * G,), SENTINEL, dtype=torch.float64, device=DEV)
    _raw_score(dsc, H[200:204], bad, refs, sbuf[G:], pbuf[G:], ld)
    sb, pb = sbuf.cpu(), pbuf.cpu()[G:G + 4 * ld].view(4, ld)
    assert torch.isnan(sb[G + 1]) and torch.isnan(sb[G + 2]) and torch.isfinite(sb[G]) and torch.isfinite(sb[G + 3])
    assert (pb[1] == SENTINEL).all() and (pb[2] == SENTINEL).all() and (pb[0, :5] != SENTINEL).all()
    assert (sb[:G] == SENTINEL).all() and (sb[G + 4:] == SENTINEL).all()
    # an id the packing cannot hold: NaN for that row alone
    big = H[200:203].clone()
    big[1, 0] = 65534
    got = dsc.score_token_ids(big, [2, 2, 2], refs).cpu()
    assert torch.isnan(got[1]) and torch.isfinite(got[0]) and torch.isfinite(got[2])


def test_vectorise_record_and_limits(world, scorers):
    from show_edit_tell_amd._lib import SetError
    dsc = scorers[4].device(DEV)
    vecs, L = dsc.vectorise(to_dev(np.array([[9, 9, 9, 0, 4], [0, 0, 0, 0, 0]], dtype=np.int64)))
    rec = vecs.cpu().view(2, 8 + 8 * L)
    assert L == 5 and rec[0, 4] == 3 and rec[0, 5] == 4 and rec[1, 4] == 0 and rec[1, 5] == 1 and rec[0, 6] == 0
    keys = rec[0, 8:8 + 4 * L].view(4, L)
    from show_edit_tell_amd import ciderd
    assert keys[0].tolist() == [ciderd.pack_key([9]), 0, 0, ciderd.pack_key([0]), 0]      # the first lane of each gram only
    assert keys[1].tolist() == [ciderd.pack_key([9, 9]), 0, ciderd.pack_key([9, 0]), 0, 0]
    with pytest.raises(SetError):
        dsc.score_token_ids(torch.zeros(2, 65, dtype=torch.int64, device=DEV), [0, 0], dsc.prepare_refs([[[1, 0]]]))
    with pytest.raises(ValueError):
        dsc.prepare_refs([[[1] * 65]])


def test_reward_against_host(world, scorers):
    """self_critical_reward_device against self_critical_reward: 8 images x 3 samples, cider_weight 0.7"""
    from show_edit_tell_amd import ciderd
    sc = scorers[4]
    dsc = sc.device(DEV)
    rng = np.random.default_rng(8)
    gt = [[[int(w) for w in rng.integers(1, 58, int(rng.integers(3, 12)))] + [0] for _ in range(5)] for _ in range(8)]

    def near(b):
        c = [w for w in gt[b][int(rng.integers(0, 5))] if w][:18]
        c[int(rng.integers(0, len(c)))] = int(rng.integers(1, 58))
        row = np.zeros(20, dtype=np.int64)
        row[:len(c)] = c
        return row
    greedy = np.stack([near(b) for b in range(8)])
    sampled = np.stack([near(b % 8) for b in range(24)])                   # the repeated rollout's order: row b, image b % 8
    want = ciderd.self_critical_reward(sc, sampled, np.tile(greedy, (3, 1)), gt * 3, 0.7)
    refs = dsc.prepare_refs(gt)
    got = ciderd.self_critical_reward_device(dsc, to_dev(sampled), to_dev(greedy), refs, None, 0.7)
    assert got.dtype == torch.float32 and tuple(got.shape) == (24, 20) and got.is_cuda
    err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()
    _report("reward_abs_err", err)
    assert err <= TOL_REWARD and np.abs(want).max() > 0.1
    image_of = torch.arange(24, device=DEV) % 8
    again = ciderd.self_critical_reward_device(dsc, to_dev(sampled), to_dev(greedy), gt, image_of, 0.7)
    assert torch.equal(again, got)


def _scst_refs(wm, B, model_greedy):
    """the set-up of tests/test_hip_train.py::test_scst_train_step_with_ciderd_reward: 5 random captions per image over the real
    vocabulary — and the model's own greedy caption as the first, so that rewards are not all zero"""
    from show_edit_tell_amd import ciderd
    V = len(wm)
    rng = np.random.default_rng(3)
    allcaps = np.zeros((B, 5, 24), dtype=np.int64)
    for b in range(B):
        for j in range(5):
            n = int(rng.integers(3, 9))
            words = rng.integers(1, V - 4, n)
            if j == 0:
                g = [int(w) for w in model_greedy[b] if int(w) > 0][:20]
                words = np.array(g if g else [1], dtype=np.int64)
                n = len(words)
            allcaps[b, j, 0] = wm["<start>"]
            allcaps[b, j, 1:1 + n] = words
            allcaps[b, j, 1 + n] = wm["<end>"]
    gt = ciderd.ground_truth_lists(allcaps, wm)
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    return gt, ciderd.CiderD(df, max(docs, 2))


@pytest.mark.parametrize("net", ["editnet", "dcnet"])
def test_scst_step_device_reward_matches_host(net):
    """two identical models and seeds, one step each with reward="host" and reward="device": the mean reward agrees within
    1.9e-6, the loss within 1e-5 relative"""
    from show_edit_tell_amd import train
    out = {}
    for route in ("host", "device"):
        if net == "editnet":
            d, _, rl = editnet_modules("editnet_small")
            inputs = (to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"]))
            greedy_in = (to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]))
            step = train.scst_train_step
        else:
            d, _, rl = dcnet_modules("dcnet_small")
            inputs = (to_dev(d["prev"]), to_dev(d["plen"]))
            greedy_in = inputs
            step = train.dcnet_scst_train_step
        wm = d["wm"]
        with torch.no_grad():
            g, _ = rl(wm, *greedy_in, sample_max=True, sample_rl=False)
        gt, scorer = _scst_refs(wm, inputs[0].shape[0], g.cpu().numpy())
        opt = torch.optim.Adam(rl.parameters(), lr=1e-3)
        torch.manual_seed(4)
        out[route] = step(rl, opt, wm, *inputs, gt, scorer, n_samples=3, reward=route)
        assert all(torch.isfinite(p).all() for p in rl.parameters())
    (r_h, l_h), (r_d, l_d) = out["host"], out["device"]
    print("reward host %.9g device %.9g, loss host %.9g device %.9g" % (r_h, r_d, l_h, l_d))
    _report("scst_%s_reward_abs_diff" % net, abs(r_h - r_d))
    _report("scst_%s_loss_rel_diff" % net, abs(l_h - l_d) / max(abs(l_h), 1e-30))
    assert np.isfinite([r_h, l_h, r_d, l_d]).all()
    assert abs(r_h - r_d) <= TOL_REWARD
    assert abs(l_h - l_d) <= 1e-5 * abs(l_h)


def test_consensus_rerank_against_python(world, scorers):
    """3 images x 5 candidates against a numpy restatement on CiderD.score; image 1 holds two identical candidates (two votes);
    one weighted case"""
    from show_edit_tell_amd.evaluate import consensus_rerank, consensus_rerank_lists
    sc = scorers[4]
    dsc = sc.device(DEV)
    rng = np.random.default_rng(21)
    cands = []
    for i in range(3):
        base = [int(w) for w in rng.integers(1, 58, 9)]
        for j in range(5):
            c = list(base)
            for _ in range(j % 3):
                c[int(rng.integers(0, 9))] = int(rng.integers(1, 58))
            cands.append(c[:9 - (j % 2)] + [0])
    cands[5 + 3] = list(cands[5 + 1])
    T = np.zeros((15, 20), dtype=np.int64)
    for i, c in enumerate(cands):
        T[i, :len(c)] = c
    S = np.zeros((3, 5, 5))
    for i in range(3):
        for j in range(5):
            for r in range(5):
                S[i, j, r] = sc.score(_s(cands[i * 5 + j]), [_s(cands[i * 5 + r])])
    w = np.array([[0.4, 0.1, 0.2, 0.2, 0.1], [1, 1, 1, 1, 1], [0.0, 0.5, 0.0, 0.5, 0.0]])
    for weights in (None, w):
        ww = np.ones((3, 5)) if weights is None else weights
        want = np.zeros((3, 5))
        for i in range(3):
            for j in range(5):
                others = [r for r in range(5) if r != j]
                den = sum(ww[i, r] for r in others)
                want[i, j] = sum(ww[i, r] * S[i, j, r] for r in others) / den if den else 0.0
        best, util = consensus_rerank(dsc, to_dev(T), 5, weights)
        err = np.abs(util.cpu().numpy() - want).max()
        _report("consensus_abs_err", err)
        assert err <= TOL
        u = util.cpu().numpy()
        for i, b in enumerate(best.cpu().tolist()):
            assert want[i, b] >= want[i].max() - TOL              # the best of the restatement (the twins of image 1 may tie) ...
            assert b == int(np.flatnonzero(u[i] == u[i].max())[0])   # ... and of equal utilities the lowest index
        assert tuple(util.shape) == (3, 5) and util.is_cuda and best.dtype == torch.int64
    b2, u2 = consensus_rerank_lists(dsc, [cands[0:5], cands[5:10], cands[10:15]])
    best, util = consensus_rerank(dsc, to_dev(T), 5)
    assert b2 == best.cpu().tolist() and np.abs(np.array(u2) - util.cpu().numpy()).max() <= TOL
