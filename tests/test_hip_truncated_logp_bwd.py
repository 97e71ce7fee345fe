"""GPU: the backward of the truncated log-prob (csrc/epilogue.hip sample_logp_bwd_opts_k, include/set_hip.h
set_sample_pick_opts_key_f32 / set_sample_logp_bwd_opts_f32) against float64 autograd of the masked log-softmax on the fixtures
of tests/trunc_bwd_fixtures.py (whose margins tests/test_truncated_logp_bwd_cpu.py asserts on the oracle alone); the neutral call
against the existing backward bit for bit; autograd_ops.sample_pick with options; the sequence nodes against the per-operator
route and the fused no-grad rollout through `sample_rollout`; the self-critical steps with options."""
import ctypes as C

import numpy as np
import pytest
import torch

import trunc_bwd_fixtures as FX
import trunc_sample_oracle as TS
from hip_adapter import dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, ABS = 2e-5, 2e-7          # |d - d64| <= REL |g| inv_t p64 + ABS |g| inv_t: the ulp of y - lse for magnitudes <= 64 plus a
#                                few ulp of expf on p, one rounding of 1 - p


def _lib():
    from show_edit_tell_amd import _lib
    return _lib, _lib.load()


def _opts(o):
    L, _ = _lib()
    return None if o is None else L.SampleOpts(temperature=o[0], top_k=o[1], top_p=o[2])


def _nan_rows(x, ld, lead=0):
    """(R, V) -> a NaN-filled device buffer holding the rows at a leading dimension of ld, `lead` floats into the allocation;
    returns (buffer, view of the rows' first element)"""
    R, V = x.shape
    buf = torch.full((lead + R * ld + 8,), float("nan"), device=DEV)
    view = buf[lead:lead + R * ld].view(R, ld)
    view[:, :V] = torch.from_numpy(x).to(DEV)
    return buf, view


def _forward(x, ld, opts, blocks, seed=2024):
    """set_sample_pick_opts_key_f32 on the R rows as `blocks` launches of R / blocks rows each (the (T, B) logs of a rollout),
    every launch a step t = 0 with its own offset -> (logits buffer, logits view, raw, lse, logp, key) as device tensors"""
    L, lib = _lib()
    R, V = x.shape
    B = R // blocks
    buf, view = _nan_rows(x, ld)
    raw = torch.full((R,), -7, dtype=torch.long, device=DEV)
    lse, logp = torch.full((R,), float("nan"), device=DEV), torch.full((R,), float("nan"), device=DEV)
    key = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    seq, it = torch.zeros(B, 2, dtype=torch.long, device=DEV), torch.zeros(B, dtype=torch.long, device=DEV)
    unf, alive = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    o = _opts(opts)
    st = L.stream_of(torch.device(DEV))
    for t in range(blocks):
        r = slice(t * B, (t + 1) * B)
        L.check(lib.set_sample_pick_opts_key_f32(view[r].data_ptr(), ld, B, V, 0, 2, -1, seed, t, L.ptr(seq), L.ptr(it), L.ptr(unf),
                                                 L.ptr(alive), raw[r].data_ptr(), lse[r].data_ptr(), logp[r].data_ptr(), st,
                                                 C.byref(o) if o else None, key[r].data_ptr()), "set_sample_pick_opts_key_f32")
    torch.cuda.synchronize()
    return buf, view, raw, lse, logp, key


def _backward(view, ld, V, lse, raw, key, g, opts, ldd, lead=0):
    """set_sample_logp_bwd_opts_f32 into a NaN-prefilled buffer of leading dimension ldd -> (R, ldd) numpy, guard columns included"""
    L, lib = _lib()
    R = raw.shape[0]
    dbuf = torch.full((lead + R * ldd + 8,), float("nan"), device=DEV)
    d = dbuf[lead:lead + R * ldd].view(R, ldd)
    o = _opts(opts)
    L.check(lib.set_sample_logp_bwd_opts_f32(view.data_ptr(), ld, L.ptr(lse), L.ptr(raw), None if key is None else L.ptr(key),
                                             L.ptr(g), d.data_ptr(), ldd, R, V, C.byref(o) if o else None,
                                             L.stream_of(torch.device(DEV))), "set_sample_logp_bwd_opts_f32")
    torch.cuda.synchronize()
    assert torch.isnan(dbuf[:lead]).all() and torch.isnan(dbuf[lead + R * ldd:]).all(), "written outside the rows"
    return d.cpu().numpy()


def _check_against_float64(what, x, ld, opts, blocks, ldds, raw_override=None):
    """forward with the key, then the backward at every ldd of `ldds`: exact kept set, exact zeros outside it, NaN guard columns,
    the float64 gradient within the tolerance -> (d of the first ldd, raw, kept)"""
    R, V = x.shape
    buf, view, raw, lse, logp, key = _forward(x, ld, opts, blocks)
    raw_np = raw.cpu().numpy()
    assert raw_np.min() >= 0 and raw_np.max() < V
    y32 = TS.scaled(x, opts[0])
    kept_dev = FX.order_key(y32) >= key.cpu().numpy().view(np.uint32)[:, None]
    g = np.linspace(-1.5, 2.0, R).astype(np.float32) + np.float32(0.25)
    if raw_override is not None:
        for r, v in raw_override.items():
            raw_np[r] = v
        raw = torch.from_numpy(raw_np).to(DEV)
    d64, kept, p64, inv_t = FX.grad64(x, opts, raw_np, g)
    assert np.array_equal(kept_dev, kept), (what, "kept_key does not reproduce the oracle's set", np.nonzero(kept_dev != kept))
    if opts[1] == 0 or opts[1] >= V:
        if opts[2] == 1.0:
            assert (key == 0).all(), (what, "nothing is cut: the key must be 0")
    assert kept[np.arange(R), raw_np][raw_np >= 0].all()
    tol = (REL * p64 + ABS) * np.abs(g.astype(np.float64))[:, None] * inv_t
    first = None
    for ldd in ldds:
        d = _backward(view, ld, V, lse, raw, key, torch.from_numpy(g).to(DEV), opts, ldd)
        assert np.isnan(d[:, V:]).all(), (what, ldd, "guard columns written")
        d = d[:, :V]
        assert not np.isnan(d).any(), (what, ldd)
        assert (d[~kept] == 0.0).all(), (what, ldd, "a word outside the kept set has a gradient")
        assert (d[raw_np < 0] == 0.0).all(), (what, ldd)
        err = np.abs(d.astype(np.float64) - d64)
        worst = float((err / np.maximum(tol, 1e-300)).max())                  # (a row with g == 0: err and tol are both 0)
        print(what, "ldd", ldd, "max |d - d64| / tol = %.3f, max abs err %.2e" % (worst, float(err.max())))
        assert (err <= tol).all(), (what, ldd, worst)
        if first is None:
            first = d
        else:
            assert np.array_equal(first, d, equal_nan=True), (what, ldd, "the two layouts disagree")
    return first, raw_np, kept


# ------------------------------------------------------------------------------------------- 1. the operator against float64
@pytest.mark.parametrize("R", FX.ROWS)
@pytest.mark.parametrize("V,ld", FX.SHAPES)
def test_truncated_logp_backward_against_float64(V, ld, R):
    x = FX.rows(V, R)
    blocks = 3 if R == 15 else 1
    odd = (V + 2) | 1
    for opts in FX.OPTS:
        # ldd == ld; ldd != ld (a multiple of 4 where ld is one: still the float4 path); an odd ldd (the scalar path)
        _check_against_float64((V, ld, R, opts), x, ld, opts, blocks, [ld, ((V + 3) & ~3) + 4, odd])


@pytest.mark.parametrize("path", sorted(TS.SPECIAL))
def test_zeros_ties_a_dominant_word_and_a_left_row(path):
    """trunc_sample_oracle.special_rows plus a copy of row 0 whose raw_id is -1: +0.0 / -0.0 at the k boundary as the oracle; the
    tie group of three across the k boundary gets one and the same non-zero gradient (the drawn word apart); the row whose one
    word alone exceeds top_p is exactly zero throughout; the row the loop had left is zeros"""
    V, ld, words = TS.SPECIAL[path]
    a, b, c, d_, e = words
    x4 = TS.special_rows(V, words)
    x = np.concatenate([x4, x4[:1]])
    for opts in TS.SPECIAL_OPTS:
        d, raw, kept = _check_against_float64(("special", path, opts), x, ld, opts, 1, [ld, ld + 3], raw_override={4: -1})
        assert (d[4] == 0.0).all()
        if opts[1] == 3:
            assert kept[0, c] and kept[0, d_] and kept[1, [c, d_, e]].all()
            for r in (1, 2):
                tie = [w for w in (c, d_, e) if w != raw[r]]
                assert len({d[r, w].tobytes() for w in tie}) == 1 and d[r, tie[0]] != 0.0, (path, opts, r)
        if opts[2] < 1.0:
            assert kept[3].sum() == 1 and raw[3] == a and (d[3] == 0.0).all(), (path, opts)


# ------------------------------------------------------------------------------------------- 2. the neutral call
@pytest.mark.parametrize("V,ld,lead", [(1027, 1028, 0), (203, 203, 0), (204, 204, 1)])
def test_neutral_call_is_the_existing_backward(V, ld, lead):
    """NULL key with NULL or neutral options: set_sample_logp_bwd_f32 bit for bit, on the float4 path, the scalar path and the
    scalar path a misaligned base forces"""
    L, lib = _lib()
    R = 9
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
    buf, view = _nan_rows(x, ld, lead)
    lse = torch.logsumexp(view[:, :V].double(), 1).float()
    raw_np = rng.integers(0, V, R)
    raw_np[4] = -1
    raw = torch.from_numpy(raw_np).to(DEV)
    g = torch.from_numpy(rng.standard_normal(R).astype(np.float32)).to(DEV)
    ldd = ld + 4
    want = torch.full((R, ldd), float("nan"), device=DEV)
    L.check(lib.set_sample_logp_bwd_f32(view.data_ptr(), ld, L.ptr(lse), L.ptr(raw), L.ptr(g), L.ptr(want), ldd, R, V,
                                        L.stream_of(torch.device(DEV))), "set_sample_logp_bwd_f32")
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    assert (want[4, :V] == 0).all() and np.abs(want[:, :V]).max() > 0
    for o in (None, TS.NEUTRAL):
        got = _backward(view, ld, V, lse, raw, None, g, o, ldd, lead=lead)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (V, ld, lead, o)
    zero_key = torch.zeros(R, dtype=torch.int32, device=DEV)
    got = _backward(view, ld, V, lse, raw, zero_key, g, None, ldd, lead=lead)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------- 3. autograd_ops.sample_pick(..., opts)
def test_sample_pick_with_options_gradient_against_float64():
    """the twin of tests/test_hip_sampling.py::test_sample_logp_backward_matches_autograd with the masked oracle as restatement"""
    from show_edit_tell_amd import autograd_ops as A
    B, V = 9, 203
    x = FX.rows(V, B)
    opts = (0.7, 5, 0.9)
    logits = torch.from_numpy(x).to(DEV).requires_grad_(True)
    state = A.SampleState(B, 2, 1, -1, torch.device(DEV), seed=77, offset=3)
    logp = A.sample_pick(logits, state, 0, _opts(opts))
    g = np.linspace(-1.0, 2.0, B).astype(np.float32)
    (logp * torch.from_numpy(g).to(DEV)).sum().backward()
    raw = state.seq[:, 0].cpu().numpy()                                      # end_idx -1: no rewrite, seq holds the drawn word
    d64, kept, p64, inv_t = FX.grad64(x, opts, raw, g)
    assert kept[np.arange(B), raw].all()
    d = logits.grad.cpu().numpy()
    assert (d[~kept] == 0.0).all()
    tol = (REL * p64 + ABS) * np.abs(g.astype(np.float64))[:, None] * inv_t
    assert (np.abs(d - d64) <= tol).all(), float((np.abs(d - d64) / tol).max())
    lp64 = np.log(p64[np.arange(B), raw])
    assert np.abs(logp.detach().cpu().numpy() - lp64).max() <= 2e-5
    # without options the operator makes the calls it made before
    l2 = torch.from_numpy(x).to(DEV).requires_grad_(True)
    s2 = A.SampleState(B, 2, 1, -1, torch.device(DEV), seed=77, offset=3)
    A.sample_pick(l2, s2, 0).sum().backward()
    assert l2.grad.shape == (B, V) and torch.isfinite(l2.grad).all()


# ------------------------------------------------------------------------------------------- 4. / 5. the nodes
ROLL = dict(temperature=0.8, top_k=5, top_p=0.95)


def _small_editnet():
    import test_hip_sequence as SQ
    from show_edit_tell_amd import editnet_rl, synth
    V, D, A_, F, B = 203, 64, 32, 256, 6
    wm = synth.word_map(V)
    sd = synth.editnet_state(9, V, D, A_, F, emb_scale=3.0, fc_scale=4.0, gain=2.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    m = editnet_rl.DecoderC(wm, D, D, D, A_, F)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    X, _, _, prev, plen = SQ._inputs(B, 36, F, 20, V, 20)
    return m.to(DEV).eval(), (wm, prev, plen, X), B


def _small_dcnet():
    from show_edit_tell_amd import dcnet_rl, synth
    V, D, A_, Cc, E, B = 203, 64, 32, 32, 64, 6
    wm = synth.word_map(V)
    sd = synth.dcnet_state(4, V, D, A_, Cc, E, 3.0, 4.0, 2.0)
    prev, plen = (torch.from_numpy(x).to(DEV) for x in synth.prev_captions(3, B, 20, V, 5))
    rl = dcnet_rl.DAE(wm, None, D, A_, Cc, E)
    rl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return rl.to(DEV).eval(), (wm, prev, plen), B


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_rollout_node_with_options_equals_per_operator_route(kind, monkeypatch):
    """tests/test_hip_sequence.py::test_rollout_node_equals_per_operator_rollout with options, through sample_rollout"""
    from show_edit_tell_amd import editnet
    m, head, B = _small_editnet() if kind == "editnet" else _small_dcnet()
    wgt = torch.linspace(0.5, 1.5, B * m.max_len, device=DEV).view(B, m.max_len)
    out = []
    for seq_node in (False, True):
        monkeypatch.setattr(editnet, "_XE_SEQUENCE", seq_node)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        seq, logp = m.sample_rollout(*head, **ROLL)
        assert logp.requires_grad and not seq.requires_grad
        (logp * wgt).sum().backward()
        out.append((seq.clone(), logp.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()
                                                          if p.grad is not None}))
    (s0, l0, g0), (s1, l1, g1) = out
    assert torch.equal(s0, s1) and int((s0 > 0).sum()) > B
    assert torch.allclose(l0, l1, atol=1e-5)
    assert set(g0) == set(g1)
    gmax = max(float(g.abs().max()) for g in g0.values())
    assert gmax > 0
    for k in g0:
        if k.endswith("full_att.bias"):
            continue
        err = float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-6 * gmax)
        assert err < 1e-3, (k, err)


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_grad_rollout_samples_what_the_fused_rollout_samples(kind):
    """same seed and options in eval mode: the grad-enabled node and the fused no-grad loop draw the same sequences and agree on
    the log-probs — the distribution differentiated is the one sampled from.  Neutral options through sample_rollout are
    forward(sample_max=False, sample_rl=True); forward itself still refuses options where gradients flow."""
    m, head, B = _small_editnet() if kind == "editnet" else _small_dcnet()
    with torch.no_grad():
        m.sample_rollout(*head, **ROLL)
        m.sample_rollout(*head, **ROLL)                                      # (the second call builds the token table)
        torch.manual_seed(23)
        seq_n, logp_n = m.sample_rollout(*head, **ROLL)
    torch.manual_seed(23)
    seq_g, logp_g = m.sample_rollout(*head, **ROLL)
    assert logp_g.requires_grad and not logp_n.requires_grad
    assert torch.equal(seq_n, seq_g) and int((seq_g > 0).sum()) > B
    assert torch.allclose(logp_n, logp_g.detach(), atol=1e-5)
    torch.manual_seed(5)
    s0, l0 = m.sample_rollout(*head)
    torch.manual_seed(5)
    s1, l1 = m(*head, sample_max=False, sample_rl=True)
    assert torch.equal(s0, s1) and torch.equal(l0.detach(), l1.detach())
    with pytest.raises(ValueError):
        m(*head, sample_max=False, sample_rl=True, top_k=5)
    m.train()
    with torch.no_grad(), pytest.raises(ValueError):
        m(*head, sample_max=False, sample_rl=True, top_k=5)


# ------------------------------------------------------------------------------------------- 6. the self-critical steps
SCST = dict(top_k=20, temperature=0.8)


def _references(B, wm):
    """the set-up of tests/test_hip_train.py::test_scst_train_step_with_ciderd_reward"""
    from show_edit_tell_amd import ciderd
    V = len(wm)
    rng = np.random.default_rng(3)
    allcaps = np.zeros((B, 5, 12), dtype=np.int64)
    for b in range(B):
        for j in range(5):
            n = int(rng.integers(3, 9))
            allcaps[b, j, 0] = wm["<start>"]
            allcaps[b, j, 1:1 + n] = rng.integers(1, V - 4, n)
            allcaps[b, j, 1 + n] = wm["<end>"]
    gt = ciderd.ground_truth_lists(allcaps, wm)
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    return gt, ciderd.CiderD(df, max(docs, 2))


def _scst(kind):
    from show_edit_tell_amd import train
    from show_edit_tell_amd.dcnet_rl import DAEWithAR
    if kind == "editnet":
        d, _, rl = editnet_modules("editnet_small")
        model, core = rl, rl
        lead = (to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"]))
        step = train.scst_train_step
    else:
        d, _, rl = dcnet_modules("dcnet_small")
        model, core = DAEWithAR(dae=rl).to(DEV), rl
        lead = (to_dev(d["prev"]), to_dev(d["plen"]))
        step = train.dcnet_scst_train_step
    gt, scorer = _references(lead[-1].shape[0], d["wm"])
    opt = torch.optim.Adam(core.parameters(), lr=1e-3)
    return model, core, lambda **kw: step(model, opt, d["wm"], *lead, gt, scorer, **kw)


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_scst_step_with_options(kind, monkeypatch):
    """top_k = 20, T = 0.8 on the small golden: finite loss, a finite gradient on every trainable parameter, weights that move —
    and every sampled word lies in the kept set trunc_sample_oracle finds on the step's own (logged) float32 logits, its
    log-prob being the oracle's truncated log-prob within 2e-5"""
    model, core, step = _scst(kind)
    seen = []
    orig = core.sample_rollout

    def spy(*a, **kw):
        seq, logp = orig(*a, **kw)
        Lg = logp.grad_fn.L                                                  # the node's logs, before its backward drops them
        seen.append((kw, Lg["LOGITS"].detach().cpu().numpy().copy(), Lg["RAW"].cpu().numpy().copy(),
                     Lg["LOGP"].detach().cpu().numpy().copy()))
        return seq, logp

    monkeypatch.setattr(core, "sample_rollout", spy)
    before = {k: p.detach().clone() for k, p in core.named_parameters()}
    torch.manual_seed(4)
    for n_samples in (1, 2):
        reward, loss = step(n_samples=n_samples, **SCST)
        assert np.isfinite(reward) and np.isfinite(loss)
        for k, p in core.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert all(torch.isfinite(p).all() for p in core.parameters())
    moved = [k for k, p in core.named_parameters() if not torch.equal(before[k], p.detach())]
    assert len(moved) > len(before) // 2, moved
    assert len(seen) == 2
    checked = 0
    for kw, logits, raw, logp in seen:
        assert kw["top_k"] == 20 and kw["temperature"] == 0.8
        T_, B_, V = logits.shape
        for t in range(T_):
            live = raw[t] >= 0
            if not live.any():
                continue
            dr = TS.truncated_draw(logits[t], (0.8, 20, 1.0), 0, 0)
            rows = np.nonzero(live)[0]
            assert dr.kept[rows, raw[t][rows]].all(), (t, "a sampled word outside the kept set")
            assert np.abs(dr.logp[rows, raw[t][rows]] - logp[t][rows]).max() <= 2e-5, t
            assert (dr.kept.sum(1) >= 20).all()
            checked += len(rows)
    assert checked >= seen[0][1].shape[1]


@pytest.mark.parametrize("n_samples", [1, 2])
@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_scst_step_with_neutral_options_is_the_step_without_them(kind, n_samples):
    """equal seeds, fresh models: the step given temperature=1, top_k=0, top_p=1 draws the sequences and returns the reward and
    loss of the step without the keywords, and never goes through sample_rollout.  ONE step per model, and no comparison of the
    updated weights: the embedding gradient is a torch index_add_ (floating-point atomics), so the weights after a step are not
    reproducible bit for bit from run to run, with or without the keywords"""
    res = []
    for kw in ({}, dict(temperature=1.0, top_k=0, top_p=1.0)):
        model, core, step = _scst(kind)
        before = [p.detach().clone() for p in core.parameters()]
        outs = []
        h = core.register_forward_hook(lambda mod, a, out: outs.append(out[0].clone()))
        core.sample_rollout = None                                           # (would raise if the neutral step called it)
        torch.manual_seed(4)
        r = step(n_samples=n_samples, **kw)
        h.remove()
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, core.parameters()))
        res.append((r, outs))
    (r0, o0), (r1, o1) = res
    assert r0 == r1 and np.isfinite(r0).all() and len(o0) == len(o1) == 2     # (greedy baseline, sampled rollout)
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    assert o0[1].shape[0] == n_samples * o0[0].shape[0]
