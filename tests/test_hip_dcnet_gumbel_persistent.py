"""GPU: DCNet's Gumbel-max sampled decode as prologue + ONE persistent launch (csrc/decode_persistent.hip, sampled mode;
include/set_hip.h set_dcnet_gumbel_persistent): against the per-step loop (set_dcnet_sample_gumbel) and the float64 draw
(tests/gumbel_oracle.py) on each route's own replayed logits, the Python route (dcnet_rl.DAE.forward, evaluate.sample_captions),
the refusals of the entry, and the launch alternating with the greedy, teacher-forced and beam launches of the same model.
Fixtures: tests/dcnet_gumbel_fixtures.py (seeds and boosts chosen on the oracle alone, tests/test_dcnet_gumbel_cpu.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dcnet_gumbel_fixtures as DF
import gumbel_oracle as GO
from hip_adapter import dcnet_modules, to_dev
from test_hip_gumbel_sampling import LOGP_TOL, SENT, _check_route, _decisions, _lib, _opts, _tags, _with_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, 1, 2


def _rollout(rl, entry, wm, prev, plen, seed, temperature, max_len, table=True, opts=None, null_seq=False):
    """one call of a C rollout entry (set_dcnet_gumbel_persistent / set_dcnet_sample_gumbel) on the model's weights; the outputs
    are filled with a sentinel first.  Returns (rc, seq, seq_logp)."""
    L, lib = _lib()
    B = prev.shape[0]
    dims = rl._dims(B, prev.shape[1], max_len + 1)
    ws = rl._workspace(dims)
    w = rl._weights(dims) if table else rl._weights()
    seq = torch.full((B, max_len), SENT, dtype=torch.long, device=DEV)
    logp = torch.full((B, max_len), float(SENT), dtype=torch.float32, device=DEV)
    o = _opts(temperature) if opts is None else opts
    rc = getattr(lib, entry)(C.byref(w), C.byref(dims), L.ptr(prev), L.ptr(plen.reshape(-1)), int(wm["<start>"]), int(wm["<end>"]),
                             max_len, seed, DF.OFFSET, None if null_seq else L.ptr(seq), L.ptr(logp), L.ptr(ws), ws.numel(),
                             L.stream_of(torch.device(DEV)), C.byref(o) if o is not None else None)
    torch.cuda.synchronize()
    return rc, seq.cpu().numpy(), logp.cpu().numpy()


def _replay_logits(xe, wm, prev, plen, seq):
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
        pred, _, dl, sort_ind = _with_env("SET_DEC_PERSISTENT", "0", lambda: xe(to_dev(caps), to_dev(clen), prev, plen))
    torch.cuda.synchronize()
    pred, sort_ind = pred.cpu().numpy(), sort_ind.cpu().numpy()
    out = [None] * B
    for i, b in enumerate(sort_ind):
        assert dl[i] == n[b]
        out[b] = pred[i, :n[b]]
    return out


def _warm(rl, wm, prev, plen):
    """(the token table exists from the second no-grad call on)"""
    with torch.no_grad():
        for _ in range(2):
            rl(wm, prev, plen, True, False)


def _prepare(case):
    d, xe, rl = dcnet_modules(DF.CASE)
    end = int(d["wm"]["<end>"])
    with torch.no_grad():
        rl.fc.bias[end] += DF.END_BOOST[case]
        xe.fc.bias[end] += DF.END_BOOST[case]
    prev, plen = (to_dev(a) for a in DF.inputs(case))
    _warm(rl, d["wm"], prev, plen)
    return d, xe, rl, prev, plen, end


# ------------------------------------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize("case", DF.CASES)
def test_persistent_launch_matches_the_per_step_loop_and_the_oracle(case):
    """rows 1 and 4 (resident variant), 5 (one caption five times) and 8 (temperature 0.5) and 2 rows padded to T = 24 (general
    variant), max_len 6: SET_OK on sentinel-filled outputs, every word and log-prob written, log-probs finite and <= 0, a second
    call bit-identical; the same seed through set_dcnet_sample_gumbel gives the same tokens row by row; every decision of both
    routes equals the float64 draw on the route's own replayed logits with its log-prob within 1e-4 + 2e-5.  "Either word" (top-two
    gap below 4e-4 inv_t + 4e-5, the word is the oracle's second) is capped at 2 % of all decisions of both routes and never fills a
    row; tests/test_dcnet_gumbel_cpu.py shows that the reference alone stays ten times clear of that gap."""
    d, xe, rl, prev, plen, end = _prepare(case)
    wm, seed, temp, B = d["wm"], DF.SEEDS[case], DF.TEMPERATURE[case], DF.ROWS[case]
    rc, seq_p, logp_p = _rollout(rl, "set_dcnet_gumbel_persistent", wm, prev, plen, seed, temp, DF.MAX_LEN)
    assert rc == OK, rc
    rc, seq_s, logp_s = _rollout(rl, "set_dcnet_sample_gumbel", wm, prev, plen, seed, temp, DF.MAX_LEN)
    assert rc == OK, rc
    assert (seq_p != SENT).all() and (logp_p != SENT).all() and (seq_s != SENT).all() and (logp_s != SENT).all()
    assert np.isfinite(logp_p).all() and float(logp_p.max()) <= 0.0
    again = _rollout(rl, "set_dcnet_gumbel_persistent", wm, prev, plen, seed, temp, DF.MAX_LEN)
    assert again[0] == OK and np.array_equal(again[1], seq_p) and np.array_equal(again[2], logp_p), "run-to-run deterministic"
    limit, inv_t = DF.gap_limit(case), DF.inv_t(case)
    e_s = _check_route(seq_s, logp_s, _replay_logits(xe, wm, prev, plen, seq_s), seed, inv_t, limit, end)
    e_p = _check_route(seq_p, logp_p, _replay_logits(xe, wm, prev, plen, seq_p), seed, inv_t, limit, end)
    n = _decisions(seq_s)
    total = sum(n)
    print("case %r: %d decisions, finish %r, either-word steps: per-step %r, persistent %r" % (case, total, n, e_s, e_p))
    loose = {b for b, _ in e_s + e_p}
    for b in range(B):
        if b in loose:
            continue
        assert np.array_equal(seq_p[b], seq_s[b]), (b, seq_p[b], seq_s[b])
        assert np.abs(logp_p[b] - logp_s[b]).max() < 1e-4 + LOGP_TOL
    assert len(e_s) + len(e_p) <= DF.NEAR_TIE_FRACTION * 2 * total
    for b in loose:
        assert sum(1 for r, _ in e_s if r == b) < n[b] and sum(1 for r, _ in e_p if r == b) < _decisions(seq_p)[b]
    if B > 1:
        assert 1 in n and len(set(n)) >= min(3, B), n              # one row ends at the first step, rows end at different steps
    _, lib = _lib()
    assert lib.set_last_hip_error() == 0


# ------------------------------------------------------------------------------------------- 2. the route
_CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
import dcnet_gumbel_fixtures as DF
from hip_adapter import dcnet_modules, to_dev
from show_edit_tell_amd import evaluate
d, xe, rl = dcnet_modules(DF.CASE)
prev, plen = (to_dev(a[:1]) for a in DF.inputs(5))
torch.manual_seed(2024)
seq, logp = evaluate.sample_captions(rl, prev, plen, d["wm"], n_samples=5, sampler="gumbel")
torch.cuda.synchronize()
print("RESULT " + json.dumps(seq.cpu().tolist()))
"""


def test_python_route_takes_the_persistent_launch(tmp_path):
    """5 rows through DAE.forward and through evaluate.sample_captions (five samples of one caption): the profile shows
    persistent_gumbel and no gumbel_pick; torch.manual_seed reproduces the call; the five rows differ; a fresh child process with
    SET_DEC_PERSISTENT=0 returns the same tokens (rows without a step below the gap limit: exactly; others up to their first such
    step).  9 rows: the per-step loop, with the tokens of a direct set_dcnet_sample_gumbel call under the same seed.  The default
    and sampler="cdf" are the model's own sampled call."""
    from show_edit_tell_amd import evaluate, rng
    d, xe, rl = dcnet_modules(DF.CASE)
    wm, end = d["wm"], int(d["wm"]["<end>"])
    prev5, plen5 = (to_dev(a) for a in DF.inputs(5))
    prev, plen = prev5[:1], plen5[:1]
    _warm(rl, wm, prev5, plen5)
    torch.manual_seed(11)
    with torch.no_grad():
        (fwd, _), names = _tags(lambda: rl(wm, prev5, plen5.reshape(-1), sample_max=False, sample_rl=True, sampler="gumbel"))
    assert "persistent_gumbel" in names and "gumbel_pick" not in names, names
    assert fwd.shape == (5, rl.max_len)
    torch.manual_seed(2024)
    (seq, logp), names = _tags(lambda: evaluate.sample_captions(rl, prev, plen, wm, n_samples=5, sampler="gumbel"))
    assert "persistent_gumbel" in names and "gumbel_pick" not in names, names
    assert seq.shape == (1, 5, rl.max_len) and logp.shape == (1, 5, rl.max_len) and seq.dtype == torch.long
    torch.manual_seed(2024)
    seq2, logp2 = evaluate.sample_captions(rl, prev, plen, wm, n_samples=5, sampler="gumbel")
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
    logits = _replay_logits(xe, wm, prev5, plen5, rows)
    limit = DF.gap_limit(5)
    either = _check_route(rows, logp[0].cpu().numpy(), logits, seed, 1.0, limit, end)
    for b in range(5):
        gaps = [GO.draw(logits[b][t][None], seed, DF.OFFSET, t, 1.0, rows=[b])[1][0] for t in range(logits[b].shape[0])]
        first = next((t for t, g in enumerate(gaps) if g < limit), None)
        if first is None:
            assert np.array_equal(child[b], rows[b]), (b, child[b], rows[b])
        else:
            assert np.array_equal(child[b, :first], rows[b, :first]), (b, first)
    assert len(either) <= 1
    # 9 rows: the per-step loop with the same draws
    rs = np.random.RandomState(9)
    T = prev.shape[1]
    plen9 = rs.randint(1, T + 1, size=(9, 1)).astype(np.int64)
    prev9 = rs.randint(4, 9000, size=(9, T)).astype(np.int64) * (np.arange(T)[None] < plen9)
    prev9, plen9 = to_dev(prev9), to_dev(plen9)
    _warm(rl, wm, prev9, plen9)
    torch.manual_seed(31)
    with torch.no_grad():
        (got, got_lp), names = _tags(lambda: rl(wm, prev9, plen9.reshape(-1), sample_max=False, sample_rl=True, sampler="gumbel"))
    assert "persistent_gumbel" not in names and "gumbel_pick" in names, names
    torch.manual_seed(31)
    seed = rng.next_seed()
    rc, seq9, logp9 = _rollout(rl, "set_dcnet_sample_gumbel", wm, prev9, plen9, seed, 1.0, rl.max_len)
    assert rc == OK and np.array_equal(got.cpu().numpy(), seq9) and np.array_equal(got_lp.cpu().numpy(), logp9)
    # the default is the inverse-CDF route, call for call
    torch.manual_seed(77)
    a = evaluate.sample_captions(rl, prev, plen, wm, n_samples=5)
    torch.manual_seed(77)
    with torch.no_grad():
        b = rl(wm, prev5, plen5.reshape(-1), sample_max=False, sample_rl=True)
    assert torch.equal(a[0].view(5, -1), b[0]) and torch.equal(a[1].view(5, -1), b[1])
    torch.manual_seed(77)
    c = evaluate.sample_captions(rl, prev, plen, wm, n_samples=5, sampler="cdf")
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    torch.manual_seed(77)
    with torch.no_grad():
        c2 = rl(wm, prev5, plen5.reshape(-1), sample_max=False, sample_rl=True, sampler="cdf")
    assert torch.equal(b[0], c2[0]) and torch.equal(b[1], c2[1])


# ------------------------------------------------------------------------------------------- 3. refusals
def test_persistent_entry_refusals_leave_the_outputs_untouched():
    """a model without a token table, SET_DEC_PERSISTENT=0 and 9 rows: SET_ERR_UNSUPPORTED from set_dcnet_gumbel_persistent with
    seq / seq_logp still holding the sentinel; the same call with the table and <= 8 rows is SET_OK.  top_k / top_p in the
    options, max_len > 255 and a NULL seq: SET_ERR_ARG."""
    from show_edit_tell_amd._lib import SampleOpts
    d, xe, rl = dcnet_modules(DF.CASE)
    wm = d["wm"]
    prev, plen = (to_dev(a) for a in DF.inputs(4))
    entry = "set_dcnet_gumbel_persistent"

    def untouched(r):
        return r[0] == UNSUPPORTED and (r[1] == SENT).all() and (r[2] == SENT).all()

    assert untouched(_rollout(rl, entry, wm, prev, plen, 3, 1.0, 6, table=False))     # no token table (a fresh model)
    _warm(rl, wm, prev, plen)
    rc, seq, logp = _rollout(rl, entry, wm, prev, plen, 3, 1.0, 6)
    assert rc == OK and (seq != SENT).all() and (logp != SENT).all()                  # (the same call with the table is taken)
    assert untouched(_with_env("SET_DEC_PERSISTENT", "0", lambda: _rollout(rl, entry, wm, prev, plen, 3, 1.0, 6)))
    rs = np.random.RandomState(9)
    T = prev.shape[1]
    plen9 = rs.randint(1, T + 1, size=(9, 1)).astype(np.int64)
    prev9 = rs.randint(4, 9000, size=(9, T)).astype(np.int64) * (np.arange(T)[None] < plen9)
    prev9, plen9 = to_dev(prev9), to_dev(plen9)
    _warm(rl, wm, prev9, plen9)
    assert untouched(_rollout(rl, entry, wm, prev9, plen9, 3, 1.0, 6))
    prev8, plen8 = prev9[:8].contiguous(), plen9[:8].contiguous()
    _warm(rl, wm, prev8, plen8)
    rc, seq, logp = _rollout(rl, entry, wm, prev8, plen8, 3, 1.0, 6)
    assert rc == OK and (seq != SENT).all()

    def arg(r):
        return r[0] == ARG and (r[1] == SENT).all() and (r[2] == SENT).all()

    assert arg(_rollout(rl, entry, wm, prev, plen, 3, 1.0, 6, opts=SampleOpts(temperature=1.0, top_k=5, top_p=1.0)))
    assert arg(_rollout(rl, entry, wm, prev, plen, 3, 1.0, 6, opts=SampleOpts(temperature=1.0, top_k=0, top_p=0.9)))
    assert arg(_rollout(rl, entry, wm, prev, plen, 3, 1.0, 256))
    assert arg(_rollout(rl, entry, wm, prev, plen, 3, 1.0, 6, null_seq=True))
    _, lib = _lib()
    assert lib.set_last_hip_error() == 0


# ------------------------------------------------------------------------------------------- 4. interleaving
def test_sampled_launch_alternates_with_the_other_launches():
    """one process runs the sampled, greedy, teacher-forced and beam launches of the same model in turn, twice round: every
    result of the second round equals the first round's bit for bit, and every call is its own persistent launch (the
    per-instantiation LDS cap and residency records of csrc/decode_persistent.h do not mix)."""
    from show_edit_tell_amd import evaluate
    d, xe, rl = dcnet_modules(DF.CASE)
    wm = d["wm"]
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    caps, clen = to_dev(d["caps"]), to_dev(d["clen"])
    prev5, plen5 = (to_dev(a) for a in DF.inputs(5))
    _warm(rl, wm, prev, plen)
    _warm(rl, wm, prev5, plen5)
    with torch.no_grad():
        for _ in range(2):
            xe(caps, clen, prev, plen)
            evaluate.beam_search_dcnet(rl, prev[1:2], plen[1:2], wm, 3)

    def sampled(p, l):
        r = _rollout(rl, "set_dcnet_gumbel_persistent", wm, p, l, 5, 1.0, DF.MAX_LEN)
        assert r[0] == OK
        return r[1:]

    def teacher():
        with torch.no_grad():
            pred, _, _, sort_ind = xe(caps, clen, prev, plen)
        return pred.cpu().numpy(), sort_ind.cpu().numpy()

    def greedy():
        with torch.no_grad():
            return tuple(t.cpu().numpy() for t in rl(wm, prev, plen, True, False))

    def beam():
        got = evaluate._beam_search_dcnet_persistent(rl, prev[1:2], plen[1:2], wm, 3)
        assert got is not None
        return np.array(got[0], np.int64), np.array([got[1]])

    steps = [("persistent_gumbel", lambda: sampled(prev, plen)), ("persistent_decode", greedy),
             ("persistent_gumbel", lambda: sampled(prev5, plen5)), ("persistent_decode", teacher), ("persistent_beam", beam)]
    rounds = []
    for _ in range(2):
        out = []
        for tag, fn in steps:
            res, names = _tags(fn)
            assert tag in names, (tag, names)
            out.append(res)
        rounds.append(out)
    for (tag, _), a, b in zip(steps, rounds[0], rounds[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), tag
    _, lib = _lib()
    assert lib.set_last_hip_error() == 0
