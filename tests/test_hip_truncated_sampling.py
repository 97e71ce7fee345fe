"""GPU: temperature, top-k and top-p in the sampled pick (csrc/epilogue.hip sample_pick_k<.., TRUNC>, include/set_hip.h
SetSampleOpts) against the float64 restatement of tests/trunc_sample_oracle.py: neutral options are the existing calls bit for
bit; the kept set is exact and the draws are the oracle's on fixtures that tests/test_truncated_sampling_cpu.py shows to keep
clear of every boundary; chi-square of the renormalised distribution; top_k = 1 is the greedy pick; the bookkeeping, embedding
gather and LSTM tail are untouched; the fused rollouts and evaluate.sample_captions; the Python refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity
import pick_oracle as PO
import test_hip_pick_epilogues as PE
import trunc_sample_oracle as TS
from hip_adapter import dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
DEV = PE.DEV
TOL = 2e-5                                   # lse / step_logp against float64 (tests/test_hip_sampling.py, same quantities)


def _lib():
    from show_edit_tell_amd import _lib
    return _lib, _lib.load()


def _opts(o):
    L, _ = _lib()
    return None if o is None else L.SampleOpts(temperature=o[0], top_k=o[1], top_p=o[2])


def launch(ro, dev, n, bias_ptr, V, t, end, opts, *, ld, mode=1, seed=2024, offset=0, E=None, tail=None, plain=False):
    """one set_pick_slabs_opts_f32 call (plain: set_pick_slabs_f32) on slabs already on the device (PE.padded); returns the code"""
    L, lib = _lib()
    lt, lp, stride = dev
    a = L.PickArgs(logits=lp, ld=ld, stride=stride, bias=bias_ptr, end_idx=end, seq=ro.seq.ptr, seq_logp=ro.seq_logp.ptr,
                   it=ro.it.ptr, unfinished=ro.unf.ptr, alive=ro.alive.ptr, seed=seed, offset=offset, raw_ids=ro.raw.ptr,
                   lse=ro.lse.ptr, step_logp=ro.lp.ptr, n=n, B=ro.B, V=V, t=t, max_len=ro.max_len, D=ro.D, mode=mode)
    hold = []
    if E is not None:
        et = torch.from_numpy(np.ascontiguousarray(E, np.float32)).to(DEV)
        a.table, a.emb_out = et.data_ptr(), ro.emb.ptr
        hold.append(et)
    if tail is not None:
        a.tail = C.pointer(tail)
    st = L.stream_of(torch.device(DEV))
    o = _opts(opts)
    rc = lib.set_pick_slabs_f32(C.byref(a), st) if plain else lib.set_pick_slabs_opts_f32(C.byref(a), C.byref(o) if o else None, st)
    torch.cuda.synchronize()
    del hold
    return rc


def rows_on_device(slabs, ld, B):
    """(n, R, V) distinct rows -> (n, B, ld) on the device, row b = row b % R, NaN in the padding (PE.padded layout)"""
    n, R, V = slabs.shape
    stride = B * ld + 8
    buf = torch.full((n, stride), float("nan"), device=DEV)
    src = torch.from_numpy(np.ascontiguousarray(slabs)).to(DEV)
    for i in range(n):
        buf[i, :B * ld].view(B // R, R, ld)[:, :, :V] = src[i]
    return buf, buf.data_ptr(), stride


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def outputs(ro):
    return [ro.seq.get(), ro.it.get(), ro.raw.get(), bits(ro.lse.get()), bits(ro.lp.get())]


def check_draws(what, ro, d, row_of, V):
    """kept set exact, draws pinned (a draw within MARGIN_MIN of a CDF boundary may be its `alt`), lse / step_logp against float64"""
    raw, lse, lp = ro.raw.get(), ro.lse.get().astype(np.float64), ro.lp.get().astype(np.float64)
    assert raw.shape == (len(row_of),) and raw.min() >= 0 and raw.max() < V, (what, "a row was left out")
    out = np.nonzero(~d.kept[row_of, raw])[0]
    assert len(out) == 0, (what, "words outside the kept set", out[:8], raw[out[:8]])
    diff = np.nonzero(raw != d.ids)[0]
    for b in diff:
        assert d.margin[b] < TS.MARGIN_MIN and raw[b] == d.alt[b], (what, "row", b, raw[b], d.ids[b], d.alt[b], d.margin[b])
    e1 = float(np.abs(lse - d.lse[row_of]).max())
    e2 = float(np.abs(lp - d.logp[row_of, raw]).max())
    print(what, "lse err %.2e step_logp err %.2e, %d draws at a boundary" % (e1, e2, len(diff)))
    assert e1 <= TOL and e2 <= TOL, (what, e1, e2)


# ------------------------------------------------------------------------------------------- 1. neutral options
@pytest.mark.parametrize("V,ld", [(203, 204), (1028, 1028), (9490, 9490)])
def test_neutral_options_are_the_existing_calls(V, ld):
    L, lib = _lib()
    B, max_len, end = 64, 3, V - 1
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((1, B, V)) * 2.0).astype(np.float32)
    dev = PE.padded(x, ld)
    st = L.stream_of(torch.device(DEV))

    def pick(opts_entry, o):
        ro = PE.Rollout(B, max_len)
        args = (dev[1], ld, B, V, 0, max_len, end, 31, 5, ro.seq.ptr, ro.it.ptr, ro.unf.ptr, ro.alive.ptr, ro.raw.ptr, ro.lse.ptr,
                ro.lp.ptr, st)
        oo = _opts(o)
        rc = lib.set_sample_pick_opts_f32(*args, C.byref(oo) if oo else None) if opts_entry else lib.set_sample_pick_f32(*args)
        torch.cuda.synchronize()
        assert rc == 0
        return outputs(ro)

    def slabs(plain, o):
        ro = PE.Rollout(B, max_len)
        assert launch(ro, dev, 1, None, V, 0, end, o, ld=ld, seed=31, offset=5, plain=plain) == 0
        return outputs(ro) + [bits(ro.seq_logp.get())]

    want = pick(False, None)
    assert want[2].min() >= 0 and len(set(want[2].tolist())) > 8
    for o in (None, TS.NEUTRAL):
        for got, ref in zip(pick(True, o), want):
            assert np.array_equal(got, ref), ("set_sample_pick_opts_f32", o)
    want = slabs(True, None)
    for o in (None, TS.NEUTRAL):
        for got, ref in zip(slabs(False, o), want):
            assert np.array_equal(got, ref), ("set_pick_slabs_opts_f32", o)


def _rollout_c(kind, rl, d, seed, opts, opts_entry):
    """the fused sampled rollout through the C entry point itself (as the module's no-grad path calls it)"""
    L, lib = _lib()
    wm = d["wm"]
    prev, plen = to_dev(d["prev"]).long().contiguous(), to_dev(d["plen"]).reshape(-1).long().contiguous()
    B, max_len = prev.shape[0], rl.max_len
    seq = torch.full((B, max_len), -3, dtype=torch.long, device=DEV)
    logp = torch.full((B, max_len), -3.0, device=DEV)
    st = L.stream_of(torch.device(DEV))
    oo = _opts(opts)
    tail = (C.byref(oo) if oo else None,) if opts_entry else ()
    if kind == "editnet":
        X = to_dev(d["X"]).float().contiguous()
        dims = rl._dims(B, prev.shape[1], X.shape[1], max_len + 1)
        ws, w = rl._workspace(dims), rl._weights(dims)
        fn = lib.set_editnet_sample_opts if opts_entry else lib.set_editnet_sample
        rc = fn(C.byref(w), C.byref(dims), L.ptr(X), None, L.ptr(prev), L.ptr(plen), int(wm["<start>"]), int(wm["<end>"]), max_len,
                seed, 7 << 40, L.ptr(seq), L.ptr(logp), L.ptr(ws), ws.numel(), st, *tail)
    else:
        dims = rl._dims(B, prev.shape[1], max_len + 1)
        ws, w = rl._workspace(dims), rl._weights(dims)
        fn = lib.set_dcnet_sample_opts if opts_entry else lib.set_dcnet_sample
        rc = fn(C.byref(w), C.byref(dims), L.ptr(prev), L.ptr(plen), int(wm["<start>"]), int(wm["<end>"]), max_len, seed, 7 << 40,
                L.ptr(seq), L.ptr(logp), L.ptr(ws), ws.numel(), st, *tail)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return seq.cpu().numpy(), logp.cpu().numpy()


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_fused_rollout_with_neutral_options_is_the_existing_rollout(kind):
    d, _, rl = editnet_modules("editnet_small") if kind == "editnet" else dcnet_modules("dcnet_small")
    _rollout_c(kind, rl, d, 5, None, False)                                  # (the first call builds the token table)
    seq, logp = _rollout_c(kind, rl, d, 5, None, False)
    assert (seq > 0).any()
    for o in (None, TS.NEUTRAL):
        s2, l2 = _rollout_c(kind, rl, d, 5, o, True)
        assert np.array_equal(seq, s2) and np.array_equal(bits(logp), bits(l2)), (kind, o)


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_module_rollout_with_neutral_options_is_the_plain_sample_export(kind):
    """the module's no-grad sampled forward makes ONE call, set_<abi>_sample_opts with a NULL options pointer: for a seed it
    returns, bit for bit, what the plain set_<abi>_sample export returns for the seed and the offset rng hands out after the
    same torch.manual_seed, run by hand into a workspace of its own (3 rows of the small fixture)"""
    from show_edit_tell_amd import rng
    L, lib = _lib()
    d, _, rl = editnet_modules("editnet_small") if kind == "editnet" else dcnet_modules("dcnet_small")
    wm, B, max_len = d["wm"], 3, rl.max_len
    prev, plen = to_dev(d["prev"][:B]).long().contiguous(), to_dev(d["plen"][:B]).reshape(-1).long().contiguous()
    X = to_dev(d["X"][:B]).float().contiguous() if kind == "editnet" else None
    rl.eval()

    def module(**kw):
        with torch.no_grad():
            if kind == "editnet":
                return rl(wm, prev, plen, X, sample_max=False, sample_rl=True, **kw)
            return rl(wm, prev, plen, sample_max=False, sample_rl=True, **kw)

    module()
    module()                                                                 # (the second call builds the token table)
    torch.manual_seed(29)
    seq, logp = module()
    torch.manual_seed(29)
    seq_n, logp_n = module(temperature=1.0, top_k=0, top_p=1.0)
    torch.manual_seed(29)
    seed = rng.next_seed()
    dims = rl._dims(B, prev.shape[1], X.shape[1], max_len + 1) if kind == "editnet" else rl._dims(B, prev.shape[1], max_len + 1)
    w = rl._weights(dims)                                                    # (the view the module decodes with)
    ws = torch.empty(getattr(lib, "set_%s_workspace_bytes" % kind)(C.byref(dims)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0 and ws.data_ptr() != rl._ws.data_ptr()
    seq_c = torch.full((B, max_len), -3, dtype=torch.long, device=DEV)
    logp_c = torch.full((B, max_len), -3.0, device=DEV)
    head = (C.byref(w), C.byref(dims)) + ((L.ptr(X), None) if kind == "editnet" else ()) + (L.ptr(prev), L.ptr(plen))
    rc = getattr(lib, "set_%s_sample" % kind)(*head, int(wm["<start>"]), int(wm["<end>"]), max_len, seed,
                                             rng.offset(rng.SITE_ROLLOUT), L.ptr(seq_c), L.ptr(logp_c), L.ptr(ws), ws.numel(),
                                             L.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert seq.shape == (B, max_len) and (seq > 0).any()
    assert torch.equal(seq, seq_c) and torch.equal(logp, logp_c), kind
    assert torch.equal(seq_n, seq_c) and torch.equal(logp_n, logp_c), kind


# ------------------------------------------------------------------------------------------- 2. / 3. kept set, pinned draws
@pytest.mark.parametrize("n", TS.GRID_N)
@pytest.mark.parametrize("V,ld", TS.GRID_V)
def test_kept_set_is_exact_and_draws_are_pinned(V, ld, n):
    """every temperature and option set of the grid on 64 rows (8 distinct ones) of n slabs + bias"""
    slabs, bias, logits = TS.grid_case(V, n)
    B = TS.GRID_B
    row_of = np.arange(B) % TS.GRID_R
    dev = rows_on_device(slabs, ld, B)
    reg = TS.is_reg(V, ld, dev[2])
    assert reg == TS.is_reg(V, ld)
    bt, bp, _ = PE.padded(bias[None, None, :], V)
    top = logits.argmax(1)
    for T in TS.GRID_T:
        for top_k, top_p in TS.grid_options(V):
            opts = (T, top_k, top_p)
            ro = PE.Rollout(B, 2)
            assert launch(ro, dev, n, bp, V, 0, V + 5, opts, ld=ld) == 0
            d = TS.truncated_draw(logits, opts, 2024, 0, reg=reg, row_of=row_of)
            check_draws(("grid", V, ld, n, opts), ro, d, row_of, V)
            raw = ro.raw.get()
            if top_k == 1 or top_p == 1e-6:
                assert np.array_equal(raw, top[row_of]) and (ro.lp.get() == 0).all(), opts
            assert np.array_equal(ro.seq.get()[:, 0], raw) and np.array_equal(ro.it.get(), raw)


@pytest.mark.parametrize("path", sorted(TS.SPECIAL))
def test_zeros_ties_negative_rows_and_a_dominant_word(path):
    """4096 rows of the four chosen rows (trunc_sample_oracle.special_rows): +0.0 and -0.0 across the k boundary are both kept
    and both drawn; each word of a tie group of three across the k boundary is drawn, in a negative row too; a word that alone
    exceeds top_p is every draw of its row, with step_logp 0 within 1e-6"""
    V, ld, words = TS.SPECIAL[path]
    a, b, c, d_, e = words
    x = TS.special_rows(V, words)
    B = TS.SPECIAL_B
    row_of = np.arange(B) % 4
    dev = rows_on_device(x[None], ld, B)
    reg = TS.is_reg(V, ld, dev[2])
    assert reg == (path == "reg")
    for opts in TS.SPECIAL_OPTS:
        ro = PE.Rollout(B, 2)
        assert launch(ro, dev, 1, None, V, 0, V + 5, opts, ld=ld) == 0
        d = TS.truncated_draw(x, opts, 2024, 0, reg=reg, row_of=row_of)
        check_draws(("special", path, opts), ro, d, row_of, V)
        raw, lp = ro.raw.get(), ro.lp.get()
        if opts[1] == 3 and opts[2] == 1.0:
            assert set(raw[row_of == 0].tolist()) == {a, b, c, d_}, "a zero was never drawn"
            assert set(raw[row_of == 1].tolist()) == set(words) == set(raw[row_of == 2].tolist()), "a tied word was never drawn"
        if opts[2] < 1.0:
            assert (raw[row_of == 3] == a).all() and np.abs(lp[row_of == 3]).max() <= 1e-6


# ------------------------------------------------------------------------------------------- 4. distribution
@pytest.mark.parametrize("V,ld,seed", TS.CHI_CASES)
def test_truncated_distribution_chi_square(V, ld, seed):
    """106 496 draws from one row with top_k = 20, T = 0.7, top_p = 0.9 against the renormalised kept distribution: bins of an
    expected count >= 8, p-value > 1e-4"""
    from scipy import stats
    L, lib = _lib()
    row = TS.chi_row(V, seed)
    B, reps = 8192, 13
    buf = torch.zeros(B, ld, device=DEV)
    buf[:, :V] = torch.from_numpy(row).to(DEV)[None]
    o = _opts(TS.CHI_OPTS)
    d0 = TS.truncated_draw(row[None], TS.CHI_OPTS, 777, 0, reg=TS.is_reg(V, ld), row_of=np.zeros(1, int))
    p = np.exp(np.where(d0.kept[0], d0.logp[0], -np.inf))
    assert abs(p.sum() - 1) < 1e-12
    counts = np.zeros(V, np.int64)
    st = L.stream_of(torch.device(DEV))
    state = [torch.zeros(B, 18, dtype=torch.long, device=DEV), torch.zeros(B, dtype=torch.long, device=DEV),
             torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(20, dtype=torch.int32, device=DEV)]
    raw_d, lse_d, lp_d = torch.empty(B, dtype=torch.long, device=DEV), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    for r in range(reps):
        L.check(lib.set_sample_pick_opts_f32(L.ptr(buf), ld, B, V, 0, 18, V - 1, 777, r, *(L.ptr(s) for s in state), L.ptr(raw_d),
                                             L.ptr(lse_d), L.ptr(lp_d), st, C.byref(o)), "set_sample_pick_opts_f32")
        torch.cuda.synchronize()
        raw = raw_d.cpu().numpy()
        assert raw.min() >= 0 and raw.max() < V and d0.kept[0][raw].all()
        counts += np.bincount(raw, minlength=V)
        assert np.abs(lse_d.cpu().numpy() - d0.lse[0]).max() <= TOL
        assert np.abs(lp_d.cpu().numpy() - d0.logp[0][raw]).max() <= TOL
    nd = counts.sum()
    order = np.argsort(-p)[:int(d0.kept[0].sum())]
    bins_e, bins_o, ce, co = [], [], 0.0, 0
    for e, ob in zip(p[order] * nd, counts[order]):
        ce += e
        co += ob
        if ce >= 8.0:
            bins_e.append(ce)
            bins_o.append(co)
            ce, co = 0.0, 0
    if ce > 0:
        bins_e[-1] += ce
        bins_o[-1] += co
    assert len(bins_e) >= 3 and min(bins_e) >= 8.0
    chi2 = float((((np.array(bins_o) - np.array(bins_e)) ** 2) / np.array(bins_e)).sum())
    pval = float(stats.chi2.sf(chi2, len(bins_e) - 1))
    print("chi-square V %d: %d bins, chi2 %.2f, p %.3g" % (V, len(bins_e), chi2, pval))
    assert pval > 1e-4, (V, chi2, len(bins_e), pval)


# ------------------------------------------------------------------------------------------- 5. top_k = 1
@pytest.mark.parametrize("V,ld", [(1028, 1028), (203, 205)])
def test_top_k_one_is_the_greedy_pick(V, ld):
    slabs, bias, logits = TS.grid_case(V, 3)
    srt = np.sort(logits, 1)
    assert (srt[:, -1] > srt[:, -2]).all(), "a row's maximum is not unique"
    B = TS.GRID_B
    dev = rows_on_device(slabs, ld, B)
    bt, bp, _ = PE.padded(bias[None, None, :], V)
    greedy, sample = PE.Rollout(B, 2), PE.Rollout(B, 2)
    assert launch(greedy, dev, 3, bp, V, 0, V + 5, None, ld=ld, mode=0) == 0
    assert launch(sample, dev, 3, bp, V, 0, V + 5, (1.0, 1, 1.0), ld=ld, mode=1) == 0
    assert np.array_equal(sample.raw.get(), logits.argmax(1)[np.arange(B) % TS.GRID_R])
    assert np.array_equal(sample.it.get(), greedy.it.get()) and np.array_equal(sample.seq.get(), greedy.seq.get())
    assert (sample.lp.get() == 0).all() and (sample.seq_logp.get()[:, 0] == 0).all()


# ------------------------------------------------------------------------------------------- 6. bookkeeping, gather, tail
@pytest.mark.parametrize("ld", [52, 51])
def test_bookkeeping_is_unchanged_with_truncation(ld):
    """six steps with T = 0.5, top_k = 5 on integer logits: the device's words lie in the kept set and are the oracle's draws;
    fed to pick_oracle.book_step they give the <end> rewrite, the latch, alive, the seq / seq_logp stores and the gathered
    relu(E[it]) of every step; every row has ended after t = 3, so t = 4 and 5 write nothing and report raw_ids -1"""
    V, B, end, D, max_len = 50, 64, 48, 8, 6
    opts = (0.5, 5, 1.0)
    rng = np.random.default_rng(ld)
    E = rng.standard_normal((V, D)).astype(np.float32)
    ro = PE.Rollout(B, max_len, D)
    reg = TS.is_reg(V, ld, B * ld + 8)
    broken_at = None
    for t in range(6):
        x = rng.integers(-8, 9, size=(1, B, V)).astype(np.float32)
        x[0, :, end] = 8 if t < 3 else 40                                    # <end> among the kept words; alone from t = 3 on
        x[0, ::7, 0] = 9                                                     # some rows may pick word 0 without <end>
        dev = PE.padded(x, ld)
        assert launch(ro, dev, 1, None, V, t, end, opts, ld=ld, seed=99, offset=7, E=E) == 0
        raw = ro.raw.get()
        if broken_at is not None:
            assert (raw == -1).all() and (ro.lp.get() == 0).all()
            PO.book_step(np.zeros(B, np.int64), np.zeros(B), t, max_len, end, ro.st)
        else:
            d = TS.truncated_draw(x[0], opts, 99, 7, t=t, reg=reg)
            assert d.kept[np.arange(B), raw].all(), ("a word outside the kept set", t)
            ok = (raw == d.ids) | ((d.margin < TS.MARGIN_MIN) & (raw == d.alt))
            assert ok.all(), (t, np.nonzero(~ok)[0])
            PO.book_step(raw, d.logp[np.arange(B), raw], t, max_len, end, ro.st)
            ro.emb_want = PO.relu_embed(E, ro.st["it"]).astype(np.float32)
            if ro.st["alive"][t] == 0:
                broken_at = t
        ro.check(("truncated bookkeeping", ld, t))
    assert broken_at == 3 and (ro.st["seq"][:, 4:] == PE.FILL).all() and ro.st["alive"][0] > 0


@pytest.mark.parametrize("TD", [1024, 2048])
def test_lstm_tail_is_unchanged_with_truncation(TD):
    """the next cell of rows whose draw is decided (one possible word; top_k = 2 then reaches down to -inf), as
    test_pick_tail_finishes_the_next_cell does for the untruncated kernel"""
    L, lib = _lib()
    rng = np.random.default_rng(TD)
    V, B, end, rows, g0n = 6, 3, 2, 5, 3
    picks = [end, V - 1, 3]
    ro = PE.Rollout(B, 3)
    slabs = np.full((2, B, V), -np.inf, np.float32)
    for b, w in enumerate(picks):
        slabs[:, b, w] = rng.integers(-8, 9, size=2)
    g0 = rng.standard_normal((g0n, B, 4 * TD)).astype(np.float32)
    pre = rng.standard_normal((B, 4 * TD)).astype(np.float32)
    col0 = 4
    tab = rng.standard_normal((V, 4 * TD)).astype(np.float32)
    c0 = rng.standard_normal((rows, TD)).astype(np.float32)
    g0_t, g0_p, g0_stride = PE.padded(g0, 4 * TD + 4)
    tab_host = np.full((V, col0 + 4 * TD + 8), np.nan, np.float32)
    tab_host[:, col0:col0 + 4 * TD] = tab
    tab_t = torch.from_numpy(tab_host).to(DEV)
    c_g, h_g = PE.Guarded(c0), PE.Guarded(np.full((rows, TD), 9.0, np.float32))
    pre_t, pre_p, _ = PE.padded(pre, 4 * TD + 8)
    tail = L.PickTail(g0=g0_p, g0_stride=g0_stride, g0_ld=4 * TD + 4, tab=tab_t.data_ptr(), ld_tab=tab_host.shape[1],
                      c_in=c_g.ptr, c_out=c_g.ptr, h_out=h_g.ptr, g0_n=g0n, col0=col0, nrows=V, D=TD, pre=pre_p, ldpre=4 * TD + 8)
    assert launch(ro, PE.padded(slabs, 8), 2, None, V, 0, end, (0.8, 2, 0.9), ld=8, seed=11, offset=TD, tail=tail) == 0
    it = np.array([0, V - 1, 3])
    assert ro.it.get().tolist() == it.tolist() and ro.raw.get().tolist() == picks and (ro.lp.get() == 0).all()
    h64, c64 = PO.lstm_tail(g0, pre, tab[it], c0[:B])
    h, c = h_g.get(), c_g.get()
    assert np.array_equal(h[B:], np.full((rows - B, TD), 9.0, np.float32)) and np.array_equal(c[B:], c0[B:]), "rows past B"
    eh, ec = parity.maxerr(h[:B], h64), parity.maxerr(c[:B], c64)
    print("truncated tail D %d: h err %.2e c err %.2e" % (TD, eh, ec))
    assert eh <= parity.STATE_TOL and ec <= parity.STATE_TOL


# ------------------------------------------------------------------------------------------- 7. fused rollouts
def _oracle_state(kind, d):
    from oracle import dcnet_np as DN
    from oracle import editnet_np as EN
    P = EN.cast_params(d["sd"])
    if kind == "editnet":
        S = EN.SeqState(P, d["X"], d["prev"], d["plen"])
        return lambda words: EN.step(S, words, len(words))
    S = DN.SeqState(P, d["prev"], d["plen"])
    return lambda words: DN.step(S, words, len(words))


def _model_call(kind, rl, d, **kw):
    wm = d["wm"]
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    with torch.no_grad():
        if kind == "editnet":
            return rl(wm, prev, plen, to_dev(d["X"]), sample_max=False, sample_rl=True, **kw)
        return rl(wm, prev, plen, sample_max=False, sample_rl=True, **kw)


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_fused_truncated_rollout_replayed_through_the_oracle(kind):
    """T = 0.8, top_k = 5, top_p = 0.95 at every timestep: reproducible for a seed, another seed differs; every live word lies
    in the kept set of the oracle's logits (or its oracle logit is within 1e-4 of the threshold) and the stored log-prob is the
    oracle's truncated log-prob within 1e-4"""
    d, _, rl = editnet_modules("editnet_small") if kind == "editnet" else dcnet_modules("dcnet_small")
    wm = d["wm"]
    T, top_k, top_p = TS.ROLLOUT_OPTS
    kw = dict(temperature=T, top_k=top_k, top_p=top_p)
    rl.eval()
    _model_call(kind, rl, d, **kw)                                           # (the first call builds the token table)
    torch.manual_seed(11)
    seq, logp = _model_call(kind, rl, d, **kw)
    torch.manual_seed(11)
    seq2, logp2 = _model_call(kind, rl, d, **kw)
    torch.manual_seed(12)
    seq3, _ = _model_call(kind, rl, d, **kw)
    assert torch.equal(seq, seq2) and torch.equal(logp, logp2) and not torch.equal(seq, seq3)
    seq, logp = seq.cpu().numpy(), logp.cpu().numpy()
    B = seq.shape[0]
    assert seq.shape == (B, 18) and (logp <= 0).all()
    step = _oracle_state(kind, d)
    words, live, checked, excused = np.full(B, wm["<start>"], np.int64), np.ones(B, bool), 0, 0
    for t in range(18):
        y = TS.scaled(step(words), T)
        dr = TS.truncated_draw(y, (1.0, top_k, top_p), 0, 0)                 # (y is already scaled)
        for b in range(B):
            if not live[b]:
                continue
            w = int(seq[b, t])
            cands = [w] if w > 0 else [wm["<end>"], 0]                       # the row drew <end> (or <pad>): either explains it
            thr = y[b][dr.kept[b]].min()
            if not any(dr.kept[b, c] for c in cands):
                assert any(abs(float(y[b, c]) - thr) <= 1e-4 for c in cands), (b, t, w, y[b, cands], thr)
                excused += 1
            else:
                err = min(abs(dr.logp[b, c] - logp[b, t]) for c in cands if dr.kept[b, c])
                assert err < 1e-4, (b, t, w, err)
                checked += 1
            live[b] = w > 0
        words = seq[:, t].copy()
        if not live.any():
            break
    print(kind, "checked", checked, "excused", excused)
    assert checked >= B and excused <= checked // 10


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_sample_captions(kind):
    from show_edit_tell_amd import evaluate
    d, _, rl = editnet_modules("editnet_small") if kind == "editnet" else dcnet_modules("dcnet_small")
    wm = d["wm"]
    inputs = ((to_dev(d["X"]),) if kind == "editnet" else ()) + (to_dev(d["prev"]), to_dev(d["plen"]))
    NI, n = d["prev"].shape[0], 4
    evaluate.sample_captions(rl, *inputs, wm, n_samples=n)                   # (the first call builds the token table)
    torch.manual_seed(3)
    seq, logp = evaluate.sample_captions(rl, *inputs, wm, n_samples=n, temperature=2.0)
    assert seq.shape == (NI, n, 18) and logp.shape == (NI, n, 18) and seq.dtype == torch.long and logp.dtype == torch.float32
    for i in range(NI):
        assert not all(torch.equal(seq[i, 0], seq[i, j]) for j in range(1, n)), ("the samples of image %d are all equal" % i)
    torch.manual_seed(3)
    seq_b, logp_b = evaluate.sample_captions(rl, *inputs, wm, n_samples=n, temperature=2.0)
    assert torch.equal(seq, seq_b) and torch.equal(logp, logp_b)
    # top_k = 1: every sample is the greedy decode, on rows whose greedy top-2 gap exceeds 1e-3 at every step (all of them)
    step = _oracle_state(kind, d)
    words, live, gap = np.full(NI, wm["<start>"], np.int64), np.ones(NI, bool), np.full(NI, np.inf)
    for t in range(18):
        lg = step(words).astype(np.float64)
        top2 = -np.partition(-lg, 1, axis=1)[:, :2]
        gap = np.where(live, np.minimum(gap, top2[:, 0] - top2[:, 1]), gap)
        w = lg.argmax(1)
        w[w == wm["<end>"]] = 0
        live &= w > 0
        words = np.where(live, w, 0)
        if not live.any():
            break
    assert (gap > 1e-3).all(), ("the fixture has a row whose greedy decode is not decided", gap)
    with torch.no_grad():
        if kind == "editnet":
            greedy, _ = rl(wm, inputs[1], inputs[2], inputs[0], True, False)
        else:
            greedy, _ = rl(wm, inputs[0], inputs[1], True, False)
    seq1, logp1 = evaluate.sample_captions(rl, *inputs, wm, n_samples=n, top_k=1)
    for j in range(n):
        assert torch.equal(seq1[:, j], greedy), j
    assert (logp1 == 0).all()


# ------------------------------------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_python_refusals(kind):
    d, _, rl = editnet_modules("editnet_small") if kind == "editnet" else dcnet_modules("dcnet_small")
    wm = d["wm"]
    head = (wm, to_dev(d["prev"]), to_dev(d["plen"])) + ((to_dev(d["X"]),) if kind == "editnet" else ())
    rl.eval()
    with torch.no_grad():
        for kw in (dict(top_k=5), dict(temperature=0.5), dict(top_p=0.9)):
            with pytest.raises(ValueError):
                rl(*head, sample_max=True, sample_rl=True, **kw)
            with pytest.raises(ValueError):
                rl(*head, sample_max=True, sample_rl=False, **kw)
        for kw in (dict(top_k=-1), dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(temperature=float("nan"))):
            with pytest.raises(ValueError):
                rl(*head, sample_max=False, sample_rl=True, **kw)
    for p in rl.parameters():
        p.requires_grad_(True)
    with pytest.raises(ValueError):                                          # gradients enabled: the autograd rollout
        rl(*head, sample_max=False, sample_rl=True, top_k=5)
    rl.train()
    with torch.no_grad(), pytest.raises(ValueError):
        rl(*head, sample_max=False, sample_rl=True, top_p=0.9)
    rl.eval()
    with torch.no_grad():                                                    # neutral values: the call made is today's
        rl(*head, sample_max=False, sample_rl=True)                          # (the first call builds the token table)
        torch.manual_seed(4)
        a = rl(*head, sample_max=False, sample_rl=True)
        torch.manual_seed(4)
        b = rl(*head, sample_max=False, sample_rl=True, temperature=1.0, top_k=0, top_p=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
