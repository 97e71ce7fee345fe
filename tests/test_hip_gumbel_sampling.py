"""GPU: the Gumbel-max sampler (include/set_hip.h "Gumbel-max draw"): the device noise against the float64 restatement
(tests/gumbel_oracle.py), the per-step pick (csrc/epilogue.hip gumbel_pick_k), the persistent launch of the sampled loop
(csrc/decode_persistent_wide.hip, sampled mode) against the per-step loop word for word, evaluate.sample_captions with
sampler="gumbel", and the refusals of the persistent entry."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gumbel_fixtures as GF
import gumbel_oracle as GO
from hip_adapter import adaptive_module, dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, 1, 2
NOISE_TOL = 1e-5          # |g| <= 23: an ulp is 1.9e-6; two logs and one add cost a few ulps
GAP_MIN = 4e-5            # four times the noise bound: above it the word is the oracle's
LOGP_TOL = 2e-5           # the sampled-pick test's tolerance for step_logp / lse (tests/test_hip_sampling.py)


def _lib():
    from show_edit_tell_amd import _lib
    return _lib, _lib.load()


def _opts(t):
    from show_edit_tell_amd._lib import SampleOpts
    return None if t == 1.0 else SampleOpts(temperature=t, top_k=0, top_p=1.0)


def _fill(rows, V, t, seed, offset):
    L, lib = _lib()
    out = torch.empty(rows, V, dtype=torch.float32, device=DEV)
    L.check(lib.set_gumbel_fill_f32(L.ptr(out), rows, V, t, seed, offset, L.stream_of(torch.device(DEV))), "set_gumbel_fill_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _pick(logits, t, max_len, end_idx, seed, offset, state=None, temperature=1.0):
    """one call of set_gumbel_pick_f32; returns (state, raw_ids, lse, step_logp) as numpy"""
    L, lib = _lib()
    B, V = logits.shape
    if state is None:
        state = dict(seq=torch.zeros(B, max_len, dtype=torch.long, device=DEV), it=torch.zeros(B, dtype=torch.long, device=DEV),
                     unf=torch.zeros(B, dtype=torch.int32, device=DEV), alive=torch.zeros(max_len + 2, dtype=torch.int32, device=DEV))
    raw = torch.empty(B, dtype=torch.long, device=DEV)
    lse = torch.empty(B, dtype=torch.float32, device=DEV)
    lp = torch.empty(B, dtype=torch.float32, device=DEV)
    o = _opts(temperature)
    L.check(lib.set_gumbel_pick_f32(L.ptr(logits), logits.stride(0), B, V, t, max_len, end_idx, seed, offset, L.ptr(state["seq"]),
                                    L.ptr(state["it"]), L.ptr(state["unf"]), L.ptr(state["alive"]), L.ptr(raw), L.ptr(lse), L.ptr(lp),
                                    L.stream_of(torch.device(DEV)), C.byref(o) if o is not None else None), "set_gumbel_pick_f32")
    torch.cuda.synchronize()
    return state, raw.cpu().numpy(), lse.cpu().numpy(), lp.cpu().numpy()


# ------------------------------------------------------------------------------------------- 5. the noise
@pytest.mark.parametrize("t", [0, 7])
def test_device_noise_matches_the_oracle(t):
    """rows = 3, V = 1027 (no multiple of 4 or 256): maximum absolute error <= 1e-5 against float64; another offset differs"""
    seed, offset = 0x0123456789ABCDEF, GF.OFFSET
    got = _fill(3, 1027, t, seed, offset)
    want = GO.noise(seed, offset, range(3), t, 1027)
    err = float(np.abs(got - want).max())
    print("max |g_device - g_float64| at t = %d: %.3e" % (t, err))
    assert err <= NOISE_TOL, err
    other = _fill(3, 1027, t, seed, offset + 1)
    assert (other != got).mean() > 0.99


# ------------------------------------------------------------------------------------------- 6. the per-step pick
def _padded(lg, pad):
    """device logits with leading stride V + pad (pad such that the stride is no multiple of 4: the generic kernel)"""
    B, V = lg.shape
    buf = torch.zeros(B, V + pad)
    buf[:, :V] = torch.from_numpy(lg)
    return buf.to(DEV)[:, :V]


@pytest.mark.parametrize("V", [5, 1027, 9490])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_pick_matches_the_oracle(V, rows, temperature):
    """the word equals the oracle's arg-max wherever its top two perturbed scores differ by more than 4e-5 (either of the two
    below that); step_logp / lse within the sampled-pick test's tolerance; temperature 0.5 scales the logits first.  Both
    kernels: the register path (stride a multiple of 4, here a padded buffer) and the generic one."""
    lg = GF.pick_logits(V, rows)
    inv_t = float(np.float32(1.0) / np.float32(temperature))
    ids, gap, second, logp, lse = GO.draw(lg, GF.PICK_SEED, GF.OFFSET, 0, inv_t)
    for pad in ((-V) % 4, (-V) % 4 + 1):
        _, raw, dlse, dlp = _pick(_padded(lg, pad), 0, 6, V + 7, GF.PICK_SEED, GF.OFFSET, None, temperature)
        for b in range(rows):
            if gap[b] > GAP_MIN:
                assert raw[b] == ids[b], (pad, b, raw[b], ids[b], gap[b])
            else:
                assert raw[b] in (ids[b], second[b]), (pad, b, raw[b], ids[b], second[b], gap[b])
        y = GO.scaled(lg, inv_t).astype(np.float64)
        assert np.abs(dlse - lse).max() < LOGP_TOL
        assert np.abs(dlp - (y[np.arange(rows), raw] - lse)).max() < LOGP_TOL


@pytest.mark.parametrize("pad", [0, 1])
def test_pick_takes_the_lower_index_of_an_exact_tie(pad):
    """a row whose two largest perturbed scores are exactly equal: y is chosen so that fl32(y + g) is the same float at both
    words (g = the device's own noise; float addition is the same on the host)"""
    V, t, seed = 1028, 0, 4242
    g = _fill(1, V, t, seed, GF.OFFSET)[0]
    lg = np.zeros((1, V), np.float32)
    a, b, S = 77, 901, np.float32(40.0)

    def solve(i):
        y = np.float32(S - g[i])
        for _ in range(64):
            s = np.float32(y + g[i])
            if s == S:
                return y
            y = np.nextafter(y, np.float32(np.inf) if s < S else np.float32(-np.inf), dtype=np.float32)
        raise AssertionError("no float32 y with y + g == S")

    lg[0, a], lg[0, b] = solve(a), solve(b)
    assert np.float32(lg[0, a] + g[a]) == np.float32(lg[0, b] + g[b]) == S and lg[0, a] != lg[0, b]
    x = _padded(lg, pad) if pad else to_dev(lg)
    _, raw, _, _ = _pick(x, t, 6, V + 7, seed, GF.OFFSET)
    assert raw[0] == a, raw


def test_pick_bookkeeping_matches_reference_loop():
    """<end> -> 0, the `unfinished` latch, seq stores, the early `break` and raw_ids = -1 after it (editnet_rl.py:529-547): the
    bookkeeping test of tests/test_hip_sampling.py with the Gumbel pick"""
    V, B, max_len = 50, 64, 6
    end = V - 1
    rng = np.random.default_rng(5)
    state, unf, broken_at = None, None, None
    seq_ref = np.zeros((B, max_len), np.int64)
    for t in range(max_len):
        lg = rng.standard_normal((B, V)).astype(np.float32)
        lg[:, end] += 1.5 + (6.0 if t >= 2 else 0.0)
        if t == 3:
            lg[:, end] += 50.0
        state, raw, lse, lp = _pick(to_dev(lg), t, max_len, end, 99, 7, state)
        if broken_at is not None:
            assert (raw == -1).all() and (lp == 0).all()
            continue
        ids, gap, _, _, _ = GO.draw(lg, 99, 7, t)
        assert np.array_equal(raw[gap > GAP_MIN], ids[gap > GAP_MIN])
        it = raw.copy()
        it[it == end] = 0
        unf = (it > 0) if t == 0 else (unf & (it > 0))
        it = it * unf
        seq_ref[:, t] = it
        assert np.array_equal(state["it"].cpu().numpy(), it)
        assert np.array_equal(state["unf"].cpu().numpy().astype(bool), unf)
        assert int(state["alive"][t]) == int(unf.sum())
        if unf.sum() == 0:
            broken_at = t
    assert broken_at is not None and broken_at < max_len - 1
    assert np.array_equal(state["seq"].cpu().numpy(), seq_ref)


@pytest.mark.parametrize("pad", [0, 1])
def test_pick_distribution_chi_square(pad):
    """device draws from the 7-word distribution (8192 rows x 3 timesteps; pad 1: the register kernel, stride 8): the chi-square
    test of tests/test_hip_sampling.py against softmax(y)"""
    row = GO.SEVEN_WORDS
    B = 8192
    x = _padded(np.repeat(row[None], B, 0).copy(), pad) if pad else to_dev(np.repeat(row[None], B, 0).copy())
    counts = np.zeros(7, np.int64)
    st = None
    for t in range(3):
        st, raw, _, _ = _pick(x, t, 18, 100, 777, 3, st)
        assert raw.min() >= 0 and raw.max() < 7
        counts += np.bincount(raw, minlength=7)
    p = np.exp(row.astype(np.float64) - row.max())
    p /= p.sum()
    chi2, nb, pval = GO.chi_square_pvalue(counts, p)
    assert pval > 1e-4, (chi2, nb, pval)


# ------------------------------------------------------------------------------------------- 7. the persistent launch
def _with_env(key, val, fn):
    old = os.environ.get(key)
    os.environ[key] = val
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


SENT = -12345


def _rollout(rl, entry, wm, prev, plen, X, seed, temperature, max_len, table=True, image_mean=None):
    """one call of a C rollout entry (set_editnet_gumbel_persistent / set_editnet_sample_gumbel) on the model's weights; the
    outputs are filled with a sentinel first.  Returns (rc, seq, seq_logp)."""
    L, lib = _lib()
    B = X.shape[0]
    dims = rl._dims(B, prev.shape[1], X.shape[1], max_len + 1)
    ws = rl._workspace(dims)
    w = rl._weights(dims) if table else rl._weights()
    seq = torch.full((B, max_len), SENT, dtype=torch.long, device=DEV)
    logp = torch.full((B, max_len), float(SENT), dtype=torch.float32, device=DEV)
    o = _opts(temperature)
    rc = getattr(lib, entry)(C.byref(w), C.byref(dims), L.ptr(X), L.ptr(image_mean), L.ptr(prev), L.ptr(plen.reshape(-1)), int(wm["<start>"]),
                             int(wm["<end>"]), max_len, seed, GF.OFFSET, L.ptr(seq), L.ptr(logp), L.ptr(ws), ws.numel(),
                             L.stream_of(torch.device(DEV)), C.byref(o) if o is not None else None)
    torch.cuda.synchronize()
    return rc, seq.cpu().numpy(), logp.cpu().numpy()


def _decisions(seq):
    """decisions of every row: up to and including the step that ended it"""
    return [int((r == 0).argmax()) + 1 if (r == 0).any() else len(r) for r in seq]


def _replay_logits(xe, wm, prev, plen, X, seq):
    """the per-step route's logits of every decision of `seq`, by a teacher-forced forward (SET_DEC_PERSISTENT=0) on the tokens
    themselves: list of (n_b, V) arrays"""
    B, max_len = seq.shape
    n = _decisions(seq)
    caps = np.zeros((B, max_len + 1), np.int64)
    for b in range(B):
        caps[b, 0] = int(wm["<start>"])
        caps[b, 1:n[b]] = seq[b, :n[b] - 1]
        caps[b, n[b]] = int(wm["<end>"])
    clen = np.array(n, np.int64).reshape(-1, 1) + 1
    with torch.no_grad():
        pred, _, dl, sort_ind = _with_env("SET_DEC_PERSISTENT", "0",
                                          lambda: xe(X, to_dev(caps), to_dev(clen), prev, plen, False, 0.0))
    torch.cuda.synchronize()
    pred, sort_ind = pred.cpu().numpy(), sort_ind.cpu().numpy()
    out = [None] * B
    for i, b in enumerate(sort_ind):
        assert dl[i] == n[b]
        out[b] = pred[i, :n[b]]
    return out


def _check_route(seq, logp, logits, seed, inv_t, limit, end):
    """every decision of a route against the oracle's draw on that route's own replayed logits.  Returns the list of (row, step)
    accepted as "either word" (top-two gap below `limit`, the word is one of the two)."""
    either = []
    for b, lg in enumerate(logits):
        for t in range(lg.shape[0]):
            ids, gap, second, lp, _ = GO.draw(lg[t][None], seed, GF.OFFSET, t, inv_t, rows=[b])
            tok = lambda w: 0 if w == end else int(w)
            if seq[b, t] == tok(ids[0]):
                assert abs(logp[b, t] - lp[0]) < 1e-4 + LOGP_TOL, (b, t, logp[b, t], lp[0])
                continue
            assert gap[0] < limit and seq[b, t] == tok(second[0]), (b, t, seq[b, t], ids[0], second[0], gap[0])
            either.append((b, t))
    return either


def _prepare(B):
    d, xe, rl = editnet_modules(GF.CASE)
    end = int(d["wm"]["<end>"])
    with torch.no_grad():
        rl.fc.bias[end] += GF.END_BOOST[B]
        xe.fc.bias[end] += GF.END_BOOST[B]
    prev, plen, X = (to_dev(a) for a in GF.inputs(B))
    with torch.no_grad():
        for _ in range(2):
            rl(d["wm"], prev, plen, X, True, False)                # (the token table exists from the second call on)
    return d, xe, rl, prev, plen, X, end


@pytest.mark.parametrize("B", GF.ROWS)
def test_persistent_launch_matches_the_per_step_loop(B):
    """rows 1, 5 (temperature 0.5) and 16, max_len 6, <end> boosted so that rows finish at different steps: the persistent entry
    answers SET_OK; the same seed through set_editnet_sample_gumbel gives the same tokens, except after a step whose top-two gap
    of perturbed scores (oracle, on the route's own logits) lies below 4e-4 inv_t + 4e-5 — from there the row is followed by
    forced replay of its own tokens; seq_logp within 1e-4 + the log-prob tolerance; such steps stay within 2 % of all decisions
    and never fill a row."""
    d, xe, rl, prev, plen, X, end = _prepare(B)
    wm, seed, temp = d["wm"], GF.SEEDS[B], GF.TEMPERATURE[B]
    rc, seq_p, logp_p = _rollout(rl, "set_editnet_gumbel_persistent", wm, prev, plen, X, seed, temp, GF.MAX_LEN)
    assert rc == OK, rc
    rc, seq_s, logp_s = _rollout(rl, "set_editnet_sample_gumbel", wm, prev, plen, X, seed, temp, GF.MAX_LEN)
    assert rc == OK, rc
    assert (seq_p != SENT).all() and (seq_s != SENT).all() and np.isfinite(logp_p).all()
    again = _rollout(rl, "set_editnet_gumbel_persistent", wm, prev, plen, X, seed, temp, GF.MAX_LEN)
    assert np.array_equal(again[1], seq_p) and np.array_equal(again[2], logp_p), "run-to-run deterministic"
    limit, inv_t = GF.gap_limit(B), GF.inv_t(B)
    e_s = _check_route(seq_s, logp_s, _replay_logits(xe, wm, prev, plen, X, seq_s), seed, inv_t, limit, end)
    e_p = _check_route(seq_p, logp_p, _replay_logits(xe, wm, prev, plen, X, seq_p), seed, inv_t, limit, end)
    n = _decisions(seq_s)
    total = sum(n)
    print("B = %d: %d decisions, either-word steps: per-step %r, persistent %r" % (B, total, e_s, e_p))
    loose = {b for b, _ in e_s + e_p}
    for b in range(B):
        if b in loose:
            continue
        assert np.array_equal(seq_p[b], seq_s[b]), (b, seq_p[b], seq_s[b])
        assert np.abs(logp_p[b] - logp_s[b]).max() < 1e-4 + LOGP_TOL
    assert len(e_s) + len(e_p) <= GF.NEAR_TIE_FRACTION * 2 * total
    for b in loose:
        assert sum(1 for r, _ in e_s if r == b) < n[b] and sum(1 for r, _ in e_p if r == b) < _decisions(seq_p)[b]
    if B > 1:
        assert 1 in n and len(set(n)) >= 3, n                       # one row ends at the first step, rows end at different steps
    _, lib = _lib()
    assert lib.set_last_hip_error() == 0


# ------------------------------------------------------------------------------------------- 8. evaluate.sample_captions
_CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
import gumbel_fixtures as GF
from hip_adapter import editnet_modules, to_dev
from show_edit_tell_amd import evaluate
d, xe, rl = editnet_modules(GF.CASE)
prev, plen, X = (to_dev(a) for a in GF.inputs(1))
torch.manual_seed(2024)
seq, logp = evaluate.sample_captions(rl, X, prev, plen, d["wm"], n_samples=5, sampler="gumbel")
torch.cuda.synchronize()
print("RESULT " + json.dumps(seq.cpu().tolist()))
"""


def _tags(fn):
    L, lib = _lib()
    lib.set_profile_enable(1)
    out = fn()
    torch.cuda.synchronize()
    names = [r["tag"] for r in L.profile_report()]
    lib.set_profile_enable(0)
    return out, names


def test_sample_captions_gumbel_editnet(tmp_path):
    """shapes (NI, 5, max_len); torch.manual_seed reproduces a call; the five rows of an image differ; the in-process call is the
    persistent launch and a fresh child process with SET_DEC_PERSISTENT=0 returns the same tokens (rows without a step below
    the gap limit: exactly; others up to their first such step); the default sampler="cdf" is the model's own sampled call."""
    from show_edit_tell_amd import evaluate, rng
    d, xe, rl = editnet_modules(GF.CASE)
    wm, end = d["wm"], int(d["wm"]["<end>"])
    prev, plen, X = (to_dev(a) for a in GF.inputs(1))
    with torch.no_grad():
        for _ in range(2):
            rl(wm, prev, plen, X, True, False)
    torch.manual_seed(2024)
    (seq, logp), names = _tags(lambda: evaluate.sample_captions(rl, X, prev, plen, wm, n_samples=5, sampler="gumbel"))
    assert "persistent_gumbel" in names, names
    assert seq.shape == (1, 5, rl.max_len) and logp.shape == (1, 5, rl.max_len) and seq.dtype == torch.long
    torch.manual_seed(2024)
    seq2, logp2 = evaluate.sample_captions(rl, X, prev, plen, wm, n_samples=5, sampler="gumbel")
    assert torch.equal(seq, seq2) and torch.equal(logp, logp2)
    rows = seq[0].cpu().numpy()
    assert len({tuple(r) for r in rows.tolist()}) == 5, rows
    # the per-step route in a fresh process
    e = dict(os.environ)
    e.update(SET_DEC_PERSISTENT="0", SET_PERSISTENT_LOCK_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=e, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "RESULT " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    child = np.array(json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0]), np.int64)[0]
    torch.manual_seed(2024)
    seed = rng.next_seed()
    X5, prev5, plen5 = X.repeat_interleave(5, 0), prev.repeat_interleave(5, 0), plen.repeat_interleave(5, 0)
    logits = _replay_logits(xe, wm, prev5, plen5, X5, rows)
    limit = GF.gap_limit(1)
    either = _check_route(rows, logp[0].cpu().numpy(), logits, seed, 1.0, limit, end)
    for b in range(5):
        gaps = [GO.draw(logits[b][t][None], seed, GF.OFFSET, t, 1.0, rows=[b])[1][0] for t in range(logits[b].shape[0])]
        first = next((t for t, g in enumerate(gaps) if g < limit), None)
        if first is None:
            assert np.array_equal(child[b], rows[b]), (b, child[b], rows[b])
        else:
            assert np.array_equal(child[b, :first], rows[b, :first]), (b, first)
    assert len(either) <= 1
    # the default is the inverse-CDF route, call for call
    torch.manual_seed(77)
    a = evaluate.sample_captions(rl, X, prev, plen, wm, n_samples=5)
    torch.manual_seed(77)
    with torch.no_grad():
        b = rl(wm, prev5, plen5.reshape(-1), X5, sample_max=False, sample_rl=True)
    assert torch.equal(a[0].view(5, -1), b[0]) and torch.equal(a[1].view(5, -1), b[1])
    torch.manual_seed(77)
    c = evaluate.sample_captions(rl, X, prev, plen, wm, n_samples=5, sampler="cdf")
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_sample_captions_gumbel_dcnet():
    """DCNet takes the per-step loop: shapes, reproducibility, distinct rows, tokens against the oracle's draw on the replayed
    logits are covered for EditNet above; here the draw is checked through the log-probs (finite, <= 0) and temperature"""
    from show_edit_tell_amd import evaluate
    d, xe, rl = dcnet_modules("dcnet_full_b4")
    wm = d["wm"]
    prev, plen = to_dev(d["prev"][:2]), to_dev(d["plen"][:2])
    with torch.no_grad():
        for _ in range(2):                                         # (the token table exists from the second call on: one route below)
            rl(wm, prev.repeat_interleave(5, 0), plen.repeat_interleave(5, 0), True, False)
    torch.manual_seed(5)
    seq, logp = evaluate.sample_captions(rl, prev, plen, wm, n_samples=5, sampler="gumbel", temperature=0.7)
    torch.manual_seed(5)
    seq2, logp2 = evaluate.sample_captions(rl, prev, plen, wm, n_samples=5, sampler="gumbel", temperature=0.7)
    assert seq.shape == (2, 5, rl.max_len) and torch.equal(seq, seq2) and torch.equal(logp, logp2)
    assert torch.isfinite(logp).all() and float(logp.max()) <= 0.0
    for i in range(2):
        assert len({tuple(r) for r in seq[i].cpu().tolist()}) == 5
    torch.manual_seed(6)
    other, _ = evaluate.sample_captions(rl, prev, plen, wm, n_samples=5, sampler="gumbel", temperature=0.7)
    assert not torch.equal(other, seq)
    with pytest.raises(ValueError):
        evaluate.sample_captions(rl, prev, plen, wm, sampler="gumbel", top_k=5)
    torch.manual_seed(9)
    a = evaluate.sample_captions(rl, prev, plen, wm, n_samples=5)
    torch.manual_seed(9)
    with torch.no_grad():
        b = rl(wm, prev.repeat_interleave(5, 0), plen.reshape(-1).repeat_interleave(5, 0), sample_max=False, sample_rl=True)
    assert torch.equal(a[0].view(10, -1), b[0]) and torch.equal(a[1].view(10, -1), b[1])


# ------------------------------------------------------------------------------------------- 9. refusals
def test_persistent_entry_refusals_leave_the_outputs_untouched():
    """17 rows, adaptive features and a model without a token table: SET_ERR_UNSUPPORTED from set_editnet_gumbel_persistent with
    seq / seq_logp still holding the sentinel; the Python route then returns the per-step loop's result"""
    from show_edit_tell_amd import rng
    d, xe, rl = editnet_modules(GF.CASE)
    wm = d["wm"]
    rs = np.random.RandomState(17)
    T, R, F = d["prev"].shape[1], d["X"].shape[1], d["X"].shape[2]

    def rows(B):
        plen = rs.randint(1, T + 1, size=(B, 1)).astype(np.int64)
        prev = rs.randint(4, 9000, size=(B, T)).astype(np.int64) * (np.arange(T)[None] < plen)
        return to_dev(prev), to_dev(plen), to_dev(np.abs(rs.randn(B, R, F)).astype(np.float32))

    prev, plen, X = rows(4)
    # no token table (a fresh model)
    rc, seq, logp = _rollout(rl, "set_editnet_gumbel_persistent", wm, prev, plen, X, 3, 1.0, 6, table=False)
    assert rc == UNSUPPORTED and (seq == SENT).all() and (logp == SENT).all()
    with torch.no_grad():
        for _ in range(2):
            rl(wm, prev, plen, X, True, False)
    rc, seq, logp = _rollout(rl, "set_editnet_gumbel_persistent", wm, prev, plen, X, 3, 1.0, 6)
    assert rc == OK and (seq != SENT).all()                        # (the same call with the table is taken)
    rc, seq, logp = _with_env("SET_DEC_PERSISTENT", "0",
                              lambda: _rollout(rl, "set_editnet_gumbel_persistent", wm, prev, plen, X, 3, 1.0, 6))
    assert rc == UNSUPPORTED and (seq == SENT).all() and (logp == SENT).all()
    # 17 rows
    prev17, plen17, X17 = rows(17)
    rc, seq, logp = _rollout(rl, "set_editnet_gumbel_persistent", wm, prev17, plen17, X17, 3, 1.0, 6)
    assert rc == UNSUPPORTED and (seq == SENT).all() and (logp == SENT).all()
    # ... and the Python route falls back to the per-step loop: the direct call's tokens with the same seed
    torch.manual_seed(31)
    with torch.no_grad():
        (got, got_lp), names = _tags(lambda: rl(wm, prev17, plen17, X17, sample_max=False, sample_rl=True, sampler="gumbel"))
    assert "persistent_gumbel" not in names and "gumbel_pick" in names, names
    torch.manual_seed(31)
    seed = rng.next_seed()
    rc, seq, logp = _rollout(rl, "set_editnet_sample_gumbel", wm, prev17, plen17, X17, seed, 1.0, rl.max_len)
    assert rc == OK and np.array_equal(got.cpu().numpy(), seq) and np.array_equal(got_lp.cpu().numpy(), logp)
    # adaptive features
    da, ra = adaptive_module("editnet_adaptive_small")
    pa, la, Xa, ma = (to_dev(da[k]) for k in ("prev", "plen", "X", "image_mean"))
    for _ in range(3):                                             # (a token table, where these dims take one, exists from the second call on)
        rc, seq, logp = _rollout(ra, "set_editnet_gumbel_persistent", da["wm"], pa, la, Xa, 3, 1.0, 6, image_mean=ma)
        assert rc == UNSUPPORTED and (seq == SENT).all() and (logp == SENT).all()
