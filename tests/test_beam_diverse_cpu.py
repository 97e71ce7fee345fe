"""No GPU: what the diverse beam-search tests rest on.
(a) tests/beam_diverse_oracle.py with one group is tests/beam_constrained_oracle.py's pick on the constrained fixtures; with
    penalty = 0 every group's picks are those of a constrained search of k = g slots.
(b) The lemma: the full-candidate oracle equals the variant that sees only each row's k best (what the kernel implements), on
    random inputs with deliberate ties and large penalties.
(c) Hand-written cases: a penalty that flips a pick, a word penalised twice, <end> exempt; the edge scenarios do what they say.
(d) Every direct fixture keeps MARGIN between adjacent keys of a group's g + 1 best and between the rank scores of an image, its
    penalty changes a pick, and hypotheses complete in it.
(e) The ABI validation of set_beam_pick_diverse_f32 through the loaded library (no compute call) and the argument errors of
    evaluate.beam_search_diverse*.
(f) The search fixture of tests/test_hip_beam_diverse_search.py on the golden numpy models: near ties stay within the cap."""
import ctypes as C

import numpy as np
import pytest

import beam_constrained_fixtures as F
import beam_constrained_oracle as BO
import beam_diverse_fixtures as D
import beam_diverse_oracle as DO

STATE = ("scores", "k_left", "best_score", "best_seq", "best_len", "done_score", "done_seq", "done_len", "n_done")


# ---- (a)
@pytest.mark.parametrize("shape,cname,models", [d for d in F.DIRECT if d[1] in ("all", "ngram", "alpha")])
def test_one_group_is_the_constrained_oracle(shape, cname, models):
    V, _, k, NI = F.SHAPES[shape]
    logits, seqs, scores = F.direct_inputs(shape, cname, models)
    ref = F.direct_reference(shape, cname, models)
    got = D.run_oracle(logits, seqs, scores, F.CONSTRAINTS[cname], k, V, F.L0, 1, 3.0)
    for t, (a, b) in enumerate(zip(got, ref)):
        for n in STATE:
            assert np.array_equal(a[0][n], b[0][n]), (t, n)
        assert np.array_equal(a[0]["g_left"][:, 0], b[0]["k_left"]) and not a[0]["done_group"].any()
        assert all(np.array_equal(a[j], b[j]) for j in (1, 2, 3)), t


@pytest.mark.parametrize("shape,cname,models", [d for d in D.DIRECT if d[2] == 1])
def test_without_a_penalty_every_group_is_a_search_of_its_own(shape, cname, models):
    V, _, k, G, NI = D.SHAPES[shape]
    g = k // G
    logits, seqs, scores = D.direct_inputs(shape, cname, models)
    got = D.direct_reference(shape, cname, models, None, 0.0)
    for gi in range(G):
        sl = slice(gi * g, gi * g + g)
        rows_of = (np.arange(NI)[:, None] * k + np.arange(gi * g, gi * g + g)[None, :]).reshape(-1)
        ref = F.run_oracle([[lg[rows_of] for lg in step] for step in logits], seqs[:, sl], scores[:, sl], D.CONSTRAINTS[cname],
                           g, V, F.L0)
        for t, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a[0]["scores"][:, sl], b[0]["scores"]) and np.array_equal(a[0]["g_left"][:, gi], b[0]["k_left"])
            assert np.array_equal(a[2].reshape(NI, k)[:, sl], b[2].reshape(NI, g)), (gi, t)
            assert np.array_equal(a[3].reshape(NI, k)[:, sl] - np.arange(NI)[:, None] * k - gi * g,
                                  b[3].reshape(NI, g) - np.arange(NI)[:, None] * g), (gi, t)
            for i in range(NI):                                            # the sequences, where the group picked at this step
                assert (a[4][i] is None or a[4][i][gi] is None) == (b[4][i] is None), (gi, t, i)
                if b[4][i] is not None and not b[4][i]["exhausted"]:
                    assert np.array_equal(a[1][i, sl, :F.L0 + t + 1], b[1][i, :, :F.L0 + t + 1]), (gi, t, i)
        last_a, last_b = got[-1][0], ref[-1][0]
        for i in range(NI):                                                # the group's completions, in order
            mine = [j for j in range(int(last_a["n_done"][i])) if last_a["done_group"][i, j] == gi]
            assert len(mine) == int(last_b["n_done"][i])
            assert np.array_equal(last_a["done_score"][i, mine], last_b["done_score"][i, :len(mine)])
            assert np.array_equal(last_a["done_seq"][i, mine], last_b["done_seq"][i, :len(mine)])


# ---- (b)
def test_lemma_a_rows_k_best_are_enough():
    """random steps on a small vocabulary whose logits are multiples of 0.5 (ties inside a row and, with penalties that are
    multiples of 0.5, between penalised and unpenalised keys) and penalties up to 1e4: the full g V candidates and the rows' k best
    give the same step, state carried over four steps"""
    rs = np.random.RandomState(20240611)
    cases = 0
    for trial in range(120):
        k = int(rs.choice([2, 3, 4, 6, 8]))
        G = int(rs.choice([d for d in range(1, k + 1) if k % d == 0]))
        V, NI = int(rs.randint(k + 2, 24)), 2
        penalty = float(rs.choice([0.5, 1.0, 2.5, 1e4]))
        c = BO.Constraints(no_repeat_ngram=int(rs.choice([0, 2])), banned=(5,) if rs.rand() < 0.3 else ())
        steps = [[np.round(rs.standard_normal((NI * k, V)) * 2.0) * 0.5] for _ in range(4)]
        for lg in steps:
            lg[0][:, F.END] -= 1.0
        seqs = np.full((NI, k, 8), F.START, np.int64)
        scores = np.full((NI, k), -np.inf)
        scores[:, ::k // G] = 0.0
        full = D.run_oracle(steps, seqs, scores, c, k, V, 1, G, penalty)
        part = D.run_oracle(steps, seqs, scores, c, k, V, 1, G, penalty, rows_only=True)
        for t, (a, b) in enumerate(zip(full, part)):
            for n in a[0]:
                assert np.array_equal(a[0][n], b[0][n]), (trial, t, n)
            assert all(np.array_equal(a[j], b[j]) for j in (1, 2, 3)), (trial, t)
        cases += 1
    assert cases == 120


# ---- (c)
def _one_step(rows, k, G, penalty, V=40):
    lg = np.full((k, V), -np.inf)
    for r, words in rows.items():
        for w, p in words.items():
            lg[r, w] = np.log(p)
    st = DO.new_state(1, k, G, 4, F.START)
    out, words, rws, info = DO.pick(lg, None, st, 1, BO.NEUTRAL, k, V, F.END, G, penalty)
    return st, words.tolist(), rws.tolist(), info


def test_hand_written_steps():
    rows = {0: {10: 0.6, 11: 0.4}, 1: {10: 0.55, 12: 0.45}}
    assert _one_step(rows, 2, 2, 0.0)[1] == [10, 10]
    st, words, rws, info = _one_step(rows, 2, 2, 0.3)                       # log 0.55 - 0.3 < log 0.45: the penalty flips the pick
    assert words == [10, 12] and rws == [0, 1]
    assert abs(st["scores"][0, 1] - np.log(0.45)) < 1e-12                               # and the carried score is x
    st, words, _, _ = _one_step({0: {10: 0.6, 11: 0.4}, 1: {10: 0.9, 12: 0.1}}, 2, 2, 0.3)
    assert words == [10, 10] and abs(st["scores"][0, 1] - np.log(0.9)) < 1e-12          # a penalised pick carries x, not y
    twice = {0: {10: 0.9, 12: 0.1}, 1: {10: 0.7, 13: 0.2, 14: 0.1}, 2: {10: 0.5, 11: 0.3, 15: 0.2}}
    assert _one_step(twice, 3, 3, 0.4)[1] == [10, 10, 11]                   # 2 x 0.4 on word 10
    assert _one_step({0: twice[0], 1: {13: 1.0}, 2: twice[2]}, 3, 3, 0.4)[1] == [10, 13, 10]      # one penalty keeps it
    st, words, _, info = _one_step({0: {F.END: 0.7, 10: 0.3}, 1: {F.END: 0.6, 10: 0.25, 11: 0.15}}, 2, 2, 5.0)
    assert st["n_done"][0] == 2 and st["done_group"][0, :2].tolist() == [0, 1]                    # <end> is not penalised
    assert np.allclose(st["done_score"][0, :2], np.log([0.7, 0.6])) and st["k_left"][0] == 0
    # <end> picks are not counted either: g = 2, group 0 takes <end> and 10, group 1 is penalised for 10 alone
    st, words, _, _ = _one_step({0: {F.END: 0.6, 10: 0.4}, 2: {10: 0.5, F.END: 0.3, 11: 0.2}}, 4, 2, 5.0)
    assert words == [10, 0, 11, 0] and st["g_left"][0].tolist() == [1, 1] and st["n_done"][0] == 2


def test_edge_scenarios_do_what_they_say():
    t = D.edge_reference("tie")
    assert t[0][2].tolist() == [20, 20, 40, 30]
    for i, (a, b) in enumerate(((20, 30), (40, 30))):
        top = t[0][4][i][1]["top"]
        assert top[0][0] == top[1][0] and {top[0][1] % D.EDGE_V, top[1][1] % D.EDGE_V} == {a, b}, top       # an exact tie of keys
        assert top[0][2] != top[1][2]                                       # of a penalised and an unpenalised value
    w = D.edge_reference("worst_case")
    assert w[0][2].tolist() == list(range(10, 18))
    assert D.edge_reference("twice")[0][2].tolist() == [10, 10, 11] and D.edge_reference("twice", 0.0)[0][2].tolist() == [10, 10, 10]
    e = D.edge_reference("end_exempt")
    assert e[0][0]["n_done"][0] == 2 and e[0][0]["done_group"][0, :2].tolist() == [0, 1] and e[0][2].tolist() == [20, 0, 21, 0]
    assert e[1][0]["n_done"][0] == 4 and e[1][0]["done_group"][0].tolist() == [0, 1, 0, 1] and e[1][0]["k_left"][0] == 0
    assert e[1][0]["best_len"][0] == 2 and np.isclose(e[1][0]["best_score"][0], np.log(np.float32(0.6)))
    f = D.edge_reference("early_none_finished")
    assert f[1][0]["g_left"].tolist() == [[0, 2], [2, 0], [0, 0]] and f[0][0]["g_left"].tolist() == [[1, 2], [2, 2], [1, 1]]
    assert f[1][4][1][1]["exhausted"] and f[2][4][0][0] is None and f[2][4][1][1] is None and f[2][4][2] is None
    assert f[2][0]["k_left"].tolist() == [2, 2, 0] and f[1][0]["n_done"].tolist() == [2, 0, 4]


# ---- (d)
def test_fixture_table():
    assert sorted(D.SEEDS) == D.DIRECT and len(D.DIRECT) == 20 and F.MARGIN <= 0.002
    assert {(v, ld, k, G, NI) for v, ld, k, G, NI in D.SHAPES.values()} == {
        (255, 256, 4, 2, 3), (1027, 1027, 8, 4, 1), (1027, 1027, 8, 8, 1), (4099, 4100, 6, 3, 3), (12289, 12292, 8, 2, 2)}


@pytest.mark.parametrize("shape,cname,models", D.DIRECT)
def test_direct_fixtures_keep_their_margins_and_their_penalty_is_live(shape, cname, models):
    gap, rgap, live, n_done = D.direct_quality(shape, cname, models)
    print(shape, cname, models, "key gap %.4f rank gap %.4f" % (gap, rgap), "live", live, "completed", n_done)
    assert gap >= F.MARGIN and rgap >= F.MARGIN and live and n_done > 0


# ---- (e)
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_abi_validation_before_any_hip_call(lib):
    from show_edit_tell_amd import _lib
    for name in ("set_beam_pick_diverse_f32", "set_beam_pick_diverse_workspace_bytes"):
        assert name in _lib.PROTOTYPES and name not in _lib.MISSING
    assert len(lib.set_beam_pick_diverse_f32.argtypes) == len(lib.set_beam_pick_constrained_f32.argtypes) + 4
    assert lib.set_abi_version() == 1
    wsb = lib.set_beam_pick_diverse_workspace_bytes
    assert wsb(0, 3) == 0 and wsb(2, 9) == 0 and wsb(2, 4) == lib.set_beam_pick_constrained_workspace_bytes(2, 4) > 0
    one = C.c_void_p(16)                      # (never dereferenced: the checks come first)

    def call(k=4, groups=2, penalty=0.5, dg=one, gl=one, c="default", ws=one, ws_bytes=1 << 20, nd=one, logits=one, Lmax=8, alpha=0.0):
        cc = _lib.BeamConstraintsC(0, 0, alpha, 0, None) if c == "default" else c
        return lib.set_beam_pick_diverse_f32(logits, None, 100, 2, k, 100, 99, 1, Lmax, one, one, one, one, one, one, one, one, one,
                                             one, one, one, nd, dg, gl, groups, penalty, None if cc is None else C.byref(cc),
                                             ws, ws_bytes, None)
    ARG, UNS = 1, 2
    assert call(dg=None) == ARG and call(gl=None) == ARG and call(c=None) == ARG and call(nd=None) == ARG and call(logits=None) == ARG
    assert call(ws=None) == ARG and call(ws=C.c_void_p(24)) == ARG and call(ws_bytes=wsb(2, 4) - 1) == ARG
    assert call(groups=0) == ARG and call(groups=-2) == ARG and call(groups=3) == ARG and call(k=6, groups=4) == ARG
    assert call(penalty=-0.1) == ARG and call(penalty=float("nan")) == ARG and call(penalty=float("inf")) == ARG
    assert call(alpha=-1.0) == ARG
    assert call(k=9, groups=3) == UNS and call(k=16, groups=2) == UNS and call(Lmax=257) == UNS


class _Vocab:
    vocab_size = 50
    _ABI = "editnet"


def test_argument_errors_before_any_device_work():
    from show_edit_tell_amd import evaluate as ev
    wm = {"<start>": 2, "<end>": 3, "<unk>": 1, "<pad>": 0}
    m = _Vocab()
    d = _Vocab()
    d._ABI = "dcnet"
    for kw in (dict(beam_size=0), dict(beam_size=9, groups=3), dict(beam_size=6, groups=4), dict(beam_size=6, groups=0),
               dict(beam_size=4.5, groups=1), dict(diversity_penalty=-1.0), dict(diversity_penalty=float("nan")),
               dict(diversity_penalty=float("inf")), dict(max_steps=0), dict(max_steps=255),
               dict(constraints=ev.BeamConstraints(banned_words=("dog",))), dict(constraints=ev.BeamConstraints(banned_words=(3,)))):
        with pytest.raises(ValueError):
            ev.beam_search_diverse(m, None, None, None, wm, **kw)
        with pytest.raises(ValueError):
            ev.beam_search_diverse(d, None, None, wm, **kw)
        with pytest.raises(ValueError):
            ev.beam_search_diverse_ensemble(m, d, None, None, None, wm, **kw)
    with pytest.raises(TypeError):
        ev.beam_search_diverse(m, None, None, None, wm, constraints="no_repeat_ngram=2")
    with pytest.raises(ValueError):
        ev.beam_search_diverse((m, d), None, None, None, wm)
    with pytest.raises(ValueError):
        ev.beam_search_diverse(m, None, None, wm)                           # EditNet without image features
    with pytest.raises(ValueError):
        ev.beam_search_diverse_ensemble(d, m, None, None, None, wm)


# ---- (f)
@pytest.mark.parametrize("model", ["editnet", "dcnet", "ensemble"])
def test_search_fixture_on_the_golden_models(model):
    """the oracle's diverse search on beam_small_e5's numpy models with the GPU test's images, (k, G), penalties and constraints:
    picks whose key is closer than GAP to the next one stay within NEAR_TIE_FRACTION of all picks; with the very large penalty the
    groups' first words differ pairwise; completed hypotheses obey the constraints"""
    import nbest_oracle as NO
    from oracle import cases
    from test_beam_constrained_cpu import np_models
    d = dict(cases.build_beam(F.SEARCH_FIXTURE))
    d["sd_e"], d["sd_d"] = NO.shifted(d, F.SEARCH_SHIFT)
    wm = d["wm"]
    start, end = wm["<start>"], wm["<end>"]
    for cname, c in sorted(D.search_constraints().items()):
        for k, G in D.SEARCH_SHAPES:
            for penalty in (D.SEARCH_PENALTY, D.SEARCH_BIG_PENALTY):
                picks = near = 0
                for b in F.SEARCH_IMAGES:
                    states, V = np_models(d, b, k, model)

                    def step(words):
                        return [s.step(words) for s in states]

                    def reindex(rows):
                        for s in states:
                            s.reindex(np.asarray(rows))
                    ans, every, steps = DO.search(step, reindex, 1, k, V, start, end, c, D.SEARCH_MAX_STEPS, G, penalty)
                    p, n = near_ties(steps, 0)
                    picks, near = picks + p, near + n
                    assert len(ans[0]) == G
                    for seq, r, gi in every[0]:
                        assert not F.violates(seq, c, end), (cname, seq)
                    if penalty == D.SEARCH_BIG_PENALTY:
                        first = [w for _, gi, e in DO.groups_of(steps[0]) for w in [e["top"][0][1] % V] if w != end]
                        assert len(set(first)) == len(first), first
                print(model, cname, (k, G), penalty, "picks", picks, "near ties", near)
                assert near <= F.NEAR_TIE_FRACTION * picks, (model, cname, k, G, penalty, near, picks)


def near_ties(steps, i):
    """(counted picks of image i over a search, how many of them have a key closer than GAP to the next candidate's)"""
    picks = near = 0
    for info in steps:
        for e in (info[i] or []):
            if e:
                v = [y for y, _, _ in e["top"]]
                gaps = [p - q for p, q in zip(v, v[1:])][:e["counted"]]
                picks += len(gaps)
                near += sum(1 for x in gaps if x < F.GAP)
    return picks, near
