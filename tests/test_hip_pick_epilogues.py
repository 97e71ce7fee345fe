"""GPU: the vocabulary-row epilogues on chosen logits, at their own edges — greedy_pick_k / sample_pick_k (csrc/epilogue.hip)
through set_pick_slabs_f32, beam_pick_k (csrc/beam.hip) through set_beam_pick_f32 / set_beam_pick_nbest_f32 — against the numpy
restatements of tests/pick_oracle.py (pinned by tests/test_pick_oracle_cpu.py).

Exact pass: slab values and bias are small integers stored as fp32, so every partial sum in any order is exact, the device logit
equals the integer sum bit for bit and ties are real ties.  Words, `it`, `unfinished`, `alive`, `seq` and the gathered
relu(E[it]) must then equal the restatement exactly on every row; seq_logp is compared with float64 within LOGP_TOL = 2e-5 (the
bound tests/test_hip_sampling.py uses for lse and the gathered log-prob at these row lengths).  Logits live in NaN-filled
storage (ld > V), every output sits between guard bytes and is compared whole."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity
import pick_oracle as PO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGP_TOL = 2e-5
PAD = 256                                    # guard bytes on either side of every output
FILL = -3                                    # what seq / seq_logp hold before the first step


def _lib():
    from show_edit_tell_amd import _lib
    return _lib, _lib.load()


class Guarded:
    """a device array between two runs of 0x5A bytes; get() checks the runs and returns the array"""
    def __init__(self, init):
        init = np.ascontiguousarray(init)
        self.shape, self.dtype, self.n = init.shape, init.dtype, init.nbytes
        host = np.full(self.n + 2 * PAD, 0x5A, np.uint8)
        host[PAD:PAD + self.n] = init.view(np.uint8).ravel()
        self.t = torch.from_numpy(host).to(DEV)
        self.ptr = self.t.data_ptr() + PAD
        assert self.ptr % 16 == 0

    def get(self):
        host = self.t.cpu().numpy()
        assert (host[:PAD] == 0x5A).all() and (host[PAD + self.n:] == 0x5A).all(), "a guard byte was overwritten"
        return host[PAD:PAD + self.n].view(self.dtype).reshape(self.shape).copy()


def padded(a, ld, off=0, stride=None):
    """device copy of a (..., rows, cols) with leading dimension ld (and slab stride) in NaN-filled storage that starts `off`
    floats into an aligned allocation.  Returns (tensor kept alive, pointer, stride)."""
    a = np.asarray(a, np.float32)
    a3 = a.reshape((-1,) + a.shape[-2:])
    n, rows, cols = a3.shape
    stride = rows * ld + 8 if stride is None else stride
    host = np.full(off + n * stride + 8, np.nan, np.float32)
    host[off:off + n * stride].reshape(n, stride)[:, :rows * ld].reshape(n, rows, ld)[:, :, :cols] = a3
    t = torch.from_numpy(host).to(DEV)
    return t, t.data_ptr() + 4 * off, stride


class Rollout:
    """the caller-owned state of one rollout on the device (guarded) and in the restatement"""
    def __init__(self, B, max_len, D=0, n_alive=None):
        self.B, self.max_len, self.D = B, max_len, D
        self.st = PO.new_state(B, max_len, n_alive, fill=FILL)
        self.seq = Guarded(self.st["seq"])
        self.seq_logp = Guarded(self.st["seq_logp"].astype(np.float32))
        self.it, self.unf, self.alive = Guarded(self.st["it"]), Guarded(self.st["unf"]), Guarded(self.st["alive"])
        self.emb = Guarded(np.full((B, max(D, 1)), -7.0, np.float32))
        self.emb_want = np.full((B, max(D, 1)), -7.0, np.float32)
        self.raw, self.lse, self.lp = (Guarded(np.full(B, -5, np.int64)), Guarded(np.full(B, -5.0, np.float32)),
                                       Guarded(np.full(B, -5.0, np.float32)))

    def check(self, what):
        """every output of the greedy mode against the restatement's state"""
        st = self.st
        assert np.array_equal(self.seq.get(), st["seq"]), (what, "seq", self.seq.get(), st["seq"])
        assert np.array_equal(self.it.get(), st["it"]), (what, "it", self.it.get(), st["it"])
        assert np.array_equal(self.unf.get(), st["unf"]), (what, "unfinished")
        assert np.array_equal(self.alive.get(), st["alive"]), (what, "alive", self.alive.get(), st["alive"])
        got, want = self.seq_logp.get().astype(np.float64), st["seq_logp"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "seq_logp NaNs", got, want)
        assert np.array_equal(got == FILL, want == FILL), (what, "seq_logp written where it must not be, or the reverse")
        err = float(np.nanmax(np.abs(got - want), initial=0.0))
        print(what, "seq_logp max err %.2e" % err)
        assert err <= LOGP_TOL, (what, "seq_logp", err)
        assert np.array_equal(self.emb.get(), self.emb_want), (what, "relu(E[it])")


def launch(ro, slabs, bias, V, t, end, *, ld, off=0, bias_off=0, E=None, mode=0, seed=0, offset=0, tail=None, dev=None):
    """one set_pick_slabs_f32 call on slabs (n, B, V) (dev: the (tensor, pointer, stride) they already have on the device);
    returns the return code"""
    L, lib = _lib()
    slabs = np.asarray(slabs, np.float32)
    lt, lp, stride = padded(slabs, ld, off) if dev is None else dev
    a = L.PickArgs(logits=lp, ld=ld, stride=stride, end_idx=end, seq=ro.seq.ptr, seq_logp=ro.seq_logp.ptr, it=ro.it.ptr,
                   unfinished=ro.unf.ptr, alive=ro.alive.ptr, seed=seed, offset=offset, raw_ids=ro.raw.ptr, lse=ro.lse.ptr,
                   step_logp=ro.lp.ptr, n=slabs.shape[0], B=ro.B, V=V, t=t, max_len=ro.max_len, D=ro.D, mode=mode)
    hold = [lt]
    if bias is not None:
        bt, bp, _ = padded(np.asarray(bias, np.float32)[None, None, :], V, bias_off)
        a.bias = bp
        hold.append(bt)
    if E is not None:
        et = torch.from_numpy(np.ascontiguousarray(E, np.float32)).to(DEV)
        a.table, a.emb_out = et.data_ptr(), ro.emb.ptr
        hold.append(et)
    if tail is not None:
        a.tail = C.pointer(tail)
    rc = lib.set_pick_slabs_f32(C.byref(a), L.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    del hold
    return rc


def greedy_call(ro, slabs, bias, V, t, end, E=None, row_limit=None, **kw):
    """one greedy launch and the same step of the restatement"""
    assert launch(ro, slabs, bias, V, t, end, E=E, **kw) == 0
    PO.greedy_step(PO.slab_logits(slabs, bias, V), t, ro.max_len, end, ro.st, row_limit)
    if E is not None:
        ro.emb_want = PO.relu_embed(E, ro.st["it"]).astype(np.float32)


def int_slabs(rng, n, B, V, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=(n, B, V)).astype(np.float32)


def up4(v):
    return (v + 3) // 4 * 4


# ------------------------------------------------------------------------------------------- greedy: the grid
# (V, ld, base offset in floats, slabs, bias: None / "a" aligned / "m" misaligned pointer)
BASE = (1023, 1024, 0, 3, "a")
GRID = ([BASE] + [(V, up4(V) + 4, 0, 3, "a") for V in (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 12287, 12288, 12289)] +
        [(1023, 1025, 0, 3, "a"), (1023, 1027, 0, 3, "a"), (1024, 1028, 1, 3, "a"), (1023, 1024, 1, 3, "a")] +       # scalar by ld / base
        [(1023, 1024, 0, n, "a") for n in (1, 2, 4, 5)] + [(1023, 1025, 0, n, "a") for n in (1, 2, 4, 5)] +
        [(1023, 1024, 0, 3, None), (1024, 1028, 0, 3, "a"), (1024, 1028, 0, 3, "m"), (1023, 1024, 0, 3, "m"), (1024, 1025, 0, 3, "m")] +
        [(12288, 12292, 0, 6, "a"), (12289, 12292, 1, 5, "m"), (257, 259, 0, 4, None), (4, 4, 0, 2, "a"), (1, 1, 0, 3, "a"),
         (1, 4, 0, 1, None), (4099, 4100, 1, 2, "a"), (12287, 12288, 0, 2, None), (5, 8, 0, 6, "m"), (256, 256, 0, 1, None)])


@pytest.mark.parametrize("V,ld,off,n,bias_kind", GRID)
def test_greedy_exact_grid(V, ld, off, n, bias_kind):
    """One launch on integer logits at every row length, layout, slab count and bias path at which greedy_pick_k changes course
    (each axis against the base case V = 1023 / ld = 1024 / 3 slabs / aligned bias, plus crossed cases), with the embedding
    gather: exact on every row.  Every row holds its maximum at two words at least."""
    rng = np.random.default_rng(V * 131 + ld * 7 + off * 3 + n)
    B = 3 if V > 2000 else 7
    D = 8
    end = V - 1 if V > 1 else 5
    slabs = int_slabs(rng, n, B, V)
    bias = None if bias_kind is None else rng.integers(-8, 9, size=V).astype(np.float32)
    x = PO.slab_logits(slabs, bias, V)
    for r in range(B if V > 1 else 0):                               # every row's maximum a second time, at another word
        i = int(np.argmax(x[r]))
        j = int((i + 1 + rng.integers(0, V - 1)) % V)
        slabs[:, r, j] = slabs[:, r, i]
        if bias is not None:
            slabs[0, r, j] += bias[i] - bias[j]
    x = PO.slab_logits(slabs, bias, V)
    assert V == 1 or ((x == x.max(1, keepdims=True)).sum(1) > 1).all(), "a row of this case holds no tie"
    E = rng.standard_normal((V, D)).astype(np.float32)
    ro = Rollout(B, 3, D)
    greedy_call(ro, slabs, bias, V, 0, end, E=E, ld=ld, off=off, bias_off=1 if bias_kind == "m" else 0)
    ro.check(("grid", V, ld, off, n, bias_kind))


def test_greedy_gathers_a_long_embedding_row():
    """D = 1028: the gather's second pass is one thread wide"""
    rng = np.random.default_rng(5)
    V, B, D = 9, 4, 1028
    E = rng.standard_normal((V, D)).astype(np.float32)
    ro = Rollout(B, 2, D)
    greedy_call(ro, int_slabs(rng, 2, B, V), None, V, 0, 3, E=E, ld=12)
    ro.check("long embedding row")


# ------------------------------------------------------------------------------------------- greedy: where the tie lies
END_T = 100
# REG: thread tid owns words (tid + 256 q) * 4 + e;  scalar: thread tid owns words tid + 256 i
TIES = {
    "reg": dict(ld=4100, pairs=[(8, 10), (20, 1044), (4, 1024), (9, 13), (12, 1032), (128, 1024), (16, 256), (256, 1044),
                                (0, 4098), (50, END_T), (END_T, 200), (1024, 1028), (4096, 4098)]),
    "scalar": dict(ld=4101, pairs=[(20, 276), (1, 256), (2, 3), (3, 258), (32, 256), (16, 64), (64, 261), (0, 4098), (50, END_T),
                                   (END_T, 200), (255, 256), (4095, 4098)]),
}


@pytest.mark.parametrize("path", ["reg", "scalar"])
@pytest.mark.parametrize("n", [1, 3])
def test_greedy_tie_placement(path, n):
    """The row's maximum stands at exactly two words; the lower index must win wherever the two lie: in one float4, in two
    chunks of one thread, thread 0's second chunk against thread 1's first (the order a thread-major scan gets wrong without
    the index compare), two lanes of a wave (xor distances 1 and 32, the higher word on the LOWER lane), two waves, first and
    last column, and <end> against a lower and a higher word."""
    V, ld, pairs = 4099, TIES[path]["ld"], TIES[path]["pairs"]
    rng = np.random.default_rng(n)
    for lo in range(0, len(pairs), 9):
        chunk = pairs[lo:lo + 9]
        B = len(chunk)
        slabs = int_slabs(rng, n, B, V, -8, 2)
        for b, (i, j) in enumerate(chunk):
            slabs[:, b, i] = 8
            slabs[:, b, j] = 8
        ro = Rollout(B, 2)
        greedy_call(ro, slabs, None, V, 0, END_T, ld=ld)
        ro.check(("tie placement", path, n, lo))
        want = [0 if min(p) == END_T else min(p) for p in chunk]
        assert ro.st["it"].tolist() == want and ro.it.get().tolist() == want


# ------------------------------------------------------------------------------------------- greedy: degenerate rows
@pytest.mark.parametrize("ld", [1028, 1029])
def test_greedy_degenerate_rows(ld):
    """all-NaN and all--inf rows: word 0, NaN log-prob, row 0 of the table gathered; one NaN among finite logits: the finite
    arg-max wins, the log-prob is NaN; -inf at some words: never picked, finite log-prob."""
    rng = np.random.default_rng(ld)
    V, B, D, end = 1025, 6, 8, 7
    slabs = int_slabs(rng, 2, B, V, -8, 6)
    slabs[1, 0, :] = np.nan
    slabs[0, 1, :] = -np.inf
    slabs[1, 2, 0] = np.nan                                          # the NaN on the first word, the maximum further on, twice
    slabs[:, 2, 700] = 8
    slabs[:, 2, 900] = 8
    slabs[0, 3, ::2] = -np.inf                                       # every even word impossible, the last one (1024) included
    slabs[:, 3, 1023] = 8
    slabs[0, 4, :] = -np.inf
    slabs[0, 4, 1024] = 3                                            # one possible word, the last: log-prob 0
    E = rng.standard_normal((V, D)).astype(np.float32)
    ro = Rollout(B, 2, D)
    greedy_call(ro, slabs, None, V, 0, end, E=E, ld=ld)
    ro.check(("degenerate rows", ld))
    assert ro.st["it"].tolist()[:5] == [0, 0, 700, 1023, 1024]
    lp = ro.seq_logp.get()[:, 0]
    assert np.isnan(lp[:3]).all() and np.isfinite(lp[3:]).all() and lp[4] == 0.0


# ------------------------------------------------------------------------------------------- greedy: six steps
def _script(rng, B, V, steps, end, ends_at, zero_at=None):
    """integer logits whose arg-max is a plain word (1 .. V - 3) until row b's step ends_at[b], <end> there; zero_at = (row,
    step): that row picks word 0 instead"""
    lg = rng.integers(-8, 9, size=(steps, 2, B, V)).astype(np.float32)
    for t in range(steps):
        for b in range(B):
            top = end if t == ends_at[b] else int(rng.integers(1, V - 2))
            if zero_at == (b, t):
                top = 0
            lg[t, :, b, top] = 12
    return lg


@pytest.mark.parametrize("ld", [52, 51])
def test_greedy_six_steps_bookkeeping(ld):
    """Six calls t = 0 .. 5 on scripted logits, compared whole after every call.  (a) rows end at different steps, one by picking
    word 0 without <end> (it latches: its later plain words are not written); every row is finished after t = 3, so the calls
    t = 4, 5 find alive[3] == 0 and write nothing to seq / seq_logp.  (b) max_len = 4 with rows still running: t = 4, 5 write
    nothing either.  (c) set_decode_row_limits ends rows 1 and 3 early."""
    L, lib = _lib()
    V, B, end, D = 50, 6, 48, 8
    rng = np.random.default_rng(ld)
    E = rng.standard_normal((V, D)).astype(np.float32)
    # (a)
    lg = _script(rng, B, V, 6, end, ends_at=[0, 2, 3, 99, 1, 3], zero_at=(3, 1))
    lg[2:, :, 3, 20] = 14                                            # row 3 latched at t = 1; it goes on preferring word 20
    ro = Rollout(B, 6, D)
    for t in range(6):
        greedy_call(ro, lg[t], None, V, t, end, E=E, ld=ld)
        ro.check(("six steps (a)", ld, t))
    assert ro.st["alive"].tolist()[:6] == [5, 3, 2, 0, 0, 0]
    assert (ro.st["seq"][:, 4:] == FILL).all() and (ro.st["seq"][3, 1:4] == 0).all()
    # (b)
    lg = _script(rng, B, V, 6, end, ends_at=[99, 1, 99, 99, 5, 99])
    ro = Rollout(B, 4, D, n_alive=8)
    for t in range(6):
        greedy_call(ro, lg[t], None, V, t, end, E=E, ld=ld)
        ro.check(("six steps (b)", ld, t))
    assert ro.st["alive"].tolist()[:6] == [6, 5, 5, 5, 5, 4] and (ro.st["seq"] != FILL).all()
    # (c)
    limits = np.array([99, 2, 99, 1, 4, 99], np.int32)
    lim_d = torch.from_numpy(limits).to(DEV)
    lg = _script(rng, B, V, 6, end, ends_at=[99, 99, 2, 99, 99, 99])
    ro = Rollout(B, 6, D)
    try:
        assert lib.set_decode_row_limits(L.ptr(lim_d)) == 0
        for t in range(6):
            greedy_call(ro, lg[t], None, V, t, end, E=E, row_limit=limits, ld=ld)
            ro.check(("six steps (c)", ld, t))
    finally:
        lib.set_decode_row_limits(None)
    assert ro.st["alive"].tolist()[:6] == [5, 4, 3, 2, 2, 2]
    assert ro.st["seq"][1, :3].tolist()[1:] == [0, 0] and ro.st["seq"][3, 0] == 0 and ro.st["seq"][4, 3] == 0
    greedy_call(ro, lg[0], None, V, 0, end, E=E, ld=ld)             # the limit is gone: step 0 again, row 3 runs on
    assert ro.st["it"][3] > 0 and ro.it.get()[3] == ro.st["it"][3]


# ------------------------------------------------------------------------------------------- the LSTM tail
def _tail_case(mode, g0n, with_pre, TD, seed, latched=False):
    """V = 6 words, 3 rows that pick <end> (-> table row 0), the last word and a middle word; the next cell of every row against
    float64.  State buffers hold B + 2 rows, operands are NaN-padded past their 4 D columns.  latched: the launch is step t = 1
    of a rollout whose row 0 picked word 0 at t = 0; it now prefers the plain word 4 and must still take table row 0 (with a
    tail every thread of the greedy kernel derives the word from unfinished[b] itself)."""
    L, lib = _lib()
    rng = np.random.default_rng(seed)
    V, B, end, rows = 6, 3, 2, 5
    picks = [4 if latched else end, V - 1, 3]
    t = 1 if latched else 0
    ro = Rollout(B, 3)
    if latched:
        first = int_slabs(rng, 2, B, V, -8, 2)
        for b, w in enumerate([0, 1, 1]):
            first[:, b, w] = 7
        greedy_call(ro, first, None, V, 0, end, ld=8)
        assert ro.st["unf"].tolist() == [0, 1, 1]
    if mode == 0:
        slabs = int_slabs(rng, 2, B, V, -8, 2)
        for b, w in enumerate(picks):
            slabs[:, b, w] = 7
    else:                                                            # one possible word per row: the draw is decided
        slabs = np.full((2, B, V), -np.inf, np.float32)
        for b, w in enumerate(picks):
            slabs[:, b, w] = rng.integers(-8, 9, size=2)
    g0 = rng.standard_normal((g0n, B, 4 * TD)).astype(np.float32)
    pre = rng.standard_normal((B, 4 * TD)).astype(np.float32) if with_pre else None
    col0 = 4
    tab = rng.standard_normal((V, 4 * TD)).astype(np.float32)
    c0 = rng.standard_normal((rows, TD)).astype(np.float32)
    g0_t, g0_p, g0_stride = padded(g0, 4 * TD + 4)
    tab_host = np.full((V, col0 + 4 * TD + 8), np.nan, np.float32)
    tab_host[:, col0:col0 + 4 * TD] = tab
    tab_t = torch.from_numpy(tab_host).to(DEV)
    c_g, h_g = Guarded(c0), Guarded(np.full((rows, TD), 9.0, np.float32))
    tail = L.PickTail(g0=g0_p, g0_stride=g0_stride, g0_ld=4 * TD + 4, tab=tab_t.data_ptr(), ld_tab=tab_host.shape[1],
                      c_in=c_g.ptr, c_out=c_g.ptr, h_out=h_g.ptr, g0_n=g0n, col0=col0, nrows=V, D=TD)
    if with_pre:
        pre_t, pre_p, _ = padded(pre, 4 * TD + 8)
        tail.pre, tail.ldpre = pre_p, 4 * TD + 8
    assert launch(ro, slabs, None, V, t, end, ld=8, mode=mode, seed=11, offset=seed, tail=tail) == 0
    it = np.array([0, V - 1, 3])
    assert ro.it.get().tolist() == it.tolist()
    h64, c64 = PO.lstm_tail(g0, pre, tab[it], c0[:B])
    h, c = h_g.get(), c_g.get()
    assert np.array_equal(h[B:], np.full((rows - B, TD), 9.0, np.float32)) and np.array_equal(c[B:], c0[B:]), "rows past B"
    eh, ec = parity.maxerr(h[:B], h64), parity.maxerr(c[:B], c64)
    print("tail mode %d slabs %d pre %s D %d: h err %.2e c err %.2e" % (mode, g0n, with_pre, TD, eh, ec))
    assert eh <= parity.STATE_TOL and ec <= parity.STATE_TOL
    if mode == 0:
        PO.greedy_step(PO.slab_logits(slabs, None, V), t, ro.max_len, end, ro.st)
        ro.check(("tail", g0n, with_pre, TD, latched))
    else:
        assert ro.raw.get().tolist() == picks and (ro.lp.get() == 0).all()


TAIL_CASES = [(n, pre, 64) for n in (1, 2, 3, 4) for pre in (False, True)] + [(3, True, D) for D in (4, 1024, 1028, 2048)] + [
    (1, False, 1028), (4, False, 2048), (2, True, 4)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("g0n,with_pre,TD", TAIL_CASES)
def test_pick_tail_finishes_the_next_cell(g0n, with_pre, TD, mode):
    """Gate slabs 1 .. 4, pre NULL / given, tail D = 4 (thread 0 only), 64 (a partial first pass), 1024 (exactly one pass), 1028
    (a second pass of one thread), 2048 (two full passes); c_in aliases c_out as in the rollout; greedy and sample mode."""
    _tail_case(mode, g0n, with_pre, TD, seed=g0n * 7 + TD + int(with_pre))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("TD", [64, 1028])
def test_pick_tail_of_a_row_latched_earlier(TD, mode):
    """t = 1: a row that picked word 0 at t = 0 and prefers a plain word now feeds table row 0 to its cell, in both passes"""
    _tail_case(mode, 2, True, TD, seed=TD + mode, latched=True)


# ------------------------------------------------------------------------------------------- sample mode
def _sample_rows(rng, V, R):
    """R distinct rows: (slabs (3, R, V) integers with -inf / -200 masks in slab 0, bias, allowed (R, V) bool).  Row r's possible
    words by r % 6: one word; words 1 and 2 (what follows in their threads' spans is impossible); the first word and the last
    but one (the last word of the row impossible); every third word without the last; the last word alone; three words in the
    middle.  Impossible words are -inf on even rows and 200 below on odd rows."""
    slabs = rng.integers(-4, 5, size=(3, R, V)).astype(np.float32)
    bias = rng.integers(-4, 5, size=V).astype(np.float32)
    allowed = np.zeros((R, V), bool)
    for r in range(R):
        p = r % 6
        if p == 0:
            allowed[r, (r * 7) % V] = True
        elif p == 1:
            allowed[r, [1, 2]] = True
        elif p == 2:
            allowed[r, [0, V - 2]] = True
        elif p == 3:
            allowed[r, (r % 3)::3] = True
            allowed[r, V - 1] = False
        elif p == 4:
            allowed[r, V - 1] = True
        else:
            allowed[r, V // 2:V // 2 + 3] = True
    mask = np.where((np.arange(R) % 2 == 0)[:, None], -np.inf, -200.0).repeat(V, 1).astype(np.float32)
    slabs[0][~allowed] = mask[~allowed]
    return slabs, bias, allowed


@pytest.mark.parametrize("V,ld", [(5, 8), (5, 7), (1025, 1028), (1025, 1027), (12289, 12292)])
def test_sample_never_draws_an_impossible_word(V, ld):
    """4096 rows (64 distinct ones, repeated: the uniform depends on the row index) x 3 offsets.  Each row's possible words are a
    chosen set; the others are -inf or 200 below (expf underflows to 0).  No draw lands outside the set — the sets leave out the
    last word of the row and the end of a thread's span; a row with one possible word draws it with step_logp == 0 exactly;
    lse and step_logp match float64 within 2e-5 (three integer slabs + bias)."""
    rng = np.random.default_rng(V + ld)
    B, R = 4096, 64
    slabs, bias, allowed = _sample_rows(rng, V, R)
    x = PO.slab_logits(slabs, bias, V)
    xs = np.where(allowed, x, -np.inf)                               # (200 below the rest: e^-200 is nothing in float64 either)
    assert (np.where(allowed, -np.inf, x).max(1) <= xs.max(1) - 150).all()
    m = xs.max(1)
    lse = m + np.log(np.exp(xs - m[:, None]).sum(1))
    row_of = np.arange(B) % R
    single = (allowed.sum(1) == 1)[row_of]
    assert single.sum() > 600
    stride = B * ld + 8
    buf = torch.full((3, stride), float("nan"), device=DEV)
    rows_d = torch.from_numpy(slabs).to(DEV)
    for i in range(3):                                               # (broadcast into place: no second copy of the rows)
        buf[i, :B * ld].view(B // R, R, ld)[:, :, :V] = rows_d[i]
    for offset in (0, 1, 2):
        ro = Rollout(B, 2)
        assert launch(ro, slabs, bias, V, 0, V + 5, ld=ld, mode=1, seed=2024, offset=offset, dev=(buf, buf.data_ptr(), stride)) == 0
        raw, got_lse, got_lp = ro.raw.get(), ro.lse.get(), ro.lp.get()
        assert raw.min() >= 0 and raw.max() < V
        bad = np.nonzero(~allowed[row_of, raw])[0]
        assert len(bad) == 0, ("impossible words drawn", V, ld, offset, bad[:8], raw[bad[:8]])
        assert (got_lp[single] == 0).all()
        e1 = float(np.abs(got_lse - lse[row_of]).max())
        e2 = float(np.abs(got_lp - (x[row_of, raw] - lse[row_of])).max())
        print("sample V %d ld %d offset %d: lse err %.2e step_logp err %.2e" % (V, ld, offset, e1, e2))
        assert e1 <= LOGP_TOL and e2 <= LOGP_TOL
        assert np.array_equal(ro.seq.get()[:, 0], raw) and (ro.seq.get()[:, 1] == FILL).all()
        assert np.array_equal(ro.it.get(), raw) and ro.alive.get()[0] == int((raw > 0).sum())


# ------------------------------------------------------------------------------------------- beam pick
LMAX = 6


def _beam_logits(rng, NI, k, V, ld, end, scores, pick):
    """(NI * k, ld): rows of dead hypotheses are NaN; a live row has one word at 0 (<end> now and then, otherwise one of three
    words, so that two hypotheses of equal score often extend with the SAME word) and the others at -(32 + 0.5 n), n in 0 .. 3 —
    few distinct values, so equal candidates lie in different threads and waves all the time.  Image 0's first pick: the
    second-best value -32 stands ONLY at words 5 + 256 m, i.e. inside one thread's stride (more than 8 of them at V = 4099).
    Image 1: the first pick completes hypothesis 0, the second pick gives every live hypothesis (equal scores) the same best
    word, so the best candidates are equal across hypotheses."""
    lg = np.full((NI * k, ld), np.nan, np.float32)
    for r in range(NI * k):
        if scores[r // k, r % k] == -np.inf:
            continue
        lg[r, :V] = -(32.0 + 0.5 * rng.integers(0, 4, size=V))
        if r == 0 and pick == 0:
            lg[r, :V] = -(32.5 + 0.5 * rng.integers(0, 3, size=V))
            lg[r, 5:V:256] = -32.0
        top = end if rng.random() < 0.2 else (3, 200, V - 2)[int(rng.integers(0, 3))]
        if r // k == 1:                                                  # image 1: its first hypothesis ends at once, the others
            top = end if pick == 0 else 3                                # (equal scores) all go on with word 3
        lg[r, top] = 0.0
    return lg


def _tie_kinds(flags, k, V):
    """which placements of equal candidates occurred among the picks that mattered (a pick against a later pick or against the
    first candidates left out)"""
    kinds = dict(threads=0, waves=0, hyps=0, stride9=0)
    for i, kl, picks, cand in flags["picks"]:
        for r in range(min(k, len(cand))):
            same = [f for nv, f in cand if nv == cand[r][0]]
            if len(same) < 2:
                continue
            f0 = cand[r][1]
            for f in same:
                if f == f0:
                    continue
                ta, tb = (f0 % V) % 256, (f % V) % 256
                kinds["threads"] += ta != tb and ta // 64 == tb // 64
                kinds["waves"] += ta // 64 != tb // 64
                kinds["hyps"] += f // V != f0 // V and f % V == f0 % V
            kinds["stride9"] += sum(1 for f in same if f // V == f0 // V and (f % V) % 256 == (f0 % V) % 256) >= 9
    return kinds


@pytest.mark.parametrize("nbest", [False, True])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("V", [255, 256, 257, 1027, 4099])
def test_beam_pick_exact_with_ties(V, k, nbest):
    """NI = 3, three consecutive picks, ld > V with NaN padding and NaN rows for dead hypotheses.  Every output of every pick
    equals the restatement exactly.  That equal candidates really lay across two threads, two waves and two hypotheses is asserted
    on the restatement for k = 3 and 8, and more than 8 deep inside one thread's stride for V = 4099, k = 8 (the only case with
    room for it).  The k = 1 cases assert no tie placement: a single pick takes its row's one best word, nothing ties there —
    they check the exact outputs at that list depth only."""
    L, lib = _lib()
    assert np.float32(1.0) + np.float32(4099 - 1) * np.exp(np.float32(-32.0)) == np.float32(1.0)       # lse == top logit in fp32
    NI, ld, end, start = 3, V + 5, V - 1, V - 3
    rng = np.random.default_rng(V * 10 + k)
    neg = np.float32(-np.inf)
    h = dict(scores=np.full((NI, k), neg, np.float32), k_left=np.full(NI, k, np.int32), seqs=np.full((NI, k, LMAX), start, np.int64),
             best_score=np.full(NI, neg, np.float32), best_seq=np.zeros((NI, LMAX), np.int64), best_len=np.zeros(NI, np.int32),
             done_score=np.full((NI, k), neg, np.float32), done_seq=np.zeros((NI, k, LMAX), np.int64),
             done_len=np.zeros((NI, k), np.int32), n_done=np.zeros(NI, np.int32))
    h["scores"][:, 0] = 0.0
    g = {n: Guarded(v) for n, v in h.items()}
    g["seqs2"], g["words"], g["rows"] = Guarded(h["seqs"]), Guarded(np.zeros(NI * k, np.int64)), Guarded(np.zeros(NI * k, np.int32))
    flags = dict(picks=[])
    src, dst = "seqs", "seqs2"
    for cur_len in (1, 2, 3):
        lg = _beam_logits(rng, NI, k, V, ld, end, h["scores"], cur_len - 1)
        lg_d = torch.from_numpy(lg).to(DEV)
        head = (L.ptr(lg_d), None, ld, NI, k, V, end, cur_len, LMAX) + tuple(C.c_void_p(g[n].ptr) for n in (
            "scores", "k_left", src, dst, "best_score", "best_seq", "best_len", "words", "rows"))
        if nbest:
            rc = lib.set_beam_pick_nbest_f32(*head, *(C.c_void_p(g[n].ptr) for n in ("done_score", "done_seq", "done_len", "n_done")),
                                             L.stream_of(torch.device(DEV)))
        else:
            rc = lib.set_beam_pick_f32(*head, L.stream_of(torch.device(DEV)))
        assert rc == 0
        torch.cuda.synchronize()
        live_before = h["k_left"].copy()
        done = [h[n] if nbest else None for n in ("done_score", "done_seq", "done_len", "n_done")]
        out, w_np, r_np = PO.beam_pick(lg, h["scores"], h["k_left"], h["seqs"], h["best_score"], h["best_seq"], h["best_len"],
                                       *done, cur_len, flags, k, V, end)
        got_out, want_out = g[dst].get(), g[src].get()                   # (a finished image's sequences are not copied)
        for i in range(NI):
            if live_before[i] > 0:
                want_out[i, :, :cur_len + 1] = out[i, :, :cur_len + 1]
        assert np.array_equal(got_out, want_out), (cur_len, "sequences")
        h["seqs"] = got_out
        src, dst = dst, src
        g[dst] = Guarded(got_out)                                        # (both buffers hold the current sequences, as on the host)
        assert np.array_equal(g["words"].get(), w_np) and np.array_equal(g["rows"].get(), r_np), cur_len
        for name in ("scores", "k_left", "best_score", "best_seq", "best_len", "done_score", "done_seq", "done_len", "n_done"):
            assert np.array_equal(g[name].get(), h[name]), (cur_len, name, g[name].get(), h[name])
    kinds = _tie_kinds(flags, k, V)
    print("beam V %d k %d nbest %s: tie placements" % (V, k, nbest), kinds, "k_left", h["k_left"])
    if k >= 3:                                                           # (k = 1 picks each row's single best word: nothing ties)
        assert kinds["threads"] >= 1 and kinds["waves"] >= 1 and kinds["hyps"] >= 1, kinds
    if V == 4099 and k == 8:
        assert kinds["stride9"] >= 1, kinds


def test_beam_pick_ensemble_ids_exact_values_close():
    """logits2 given: log((softmax + softmax2) / 2) is not exact, so the inputs keep their best k + 1 candidates >= 0.25 apart in
    float64 (asserted); ids exact, values within 2e-5.  k = 3 and 8, V = 1027, ld > V with NaN padding."""
    L, lib = _lib()
    V, NI, end, start = 1027, 3, 1026, 1024
    ld = V + 5
    for k in (3, 8):
        rng = np.random.default_rng(k)
        lg = np.full((2, NI * k, ld), np.nan, np.float32)
        lg[:, :, :V] = 0.05 * rng.standard_normal((2, NI * k, V))
        for r in range(NI * k):
            spikes = rng.choice(V, k + 2, replace=False)
            spikes[2] = end                                              # the third-best word of every row ends it
            lg[:, r, spikes] = (8.0 - 0.6 * np.arange(k + 2))[None] + 0.01 * rng.standard_normal((2, k + 2))
        neg = np.float32(-np.inf)
        h = dict(scores=np.tile(-2.1 * np.arange(k, dtype=np.float32), (NI, 1)), k_left=np.full(NI, k, np.int32),
                 seqs=np.full((NI, k, LMAX), start, np.int64), best_score=np.full(NI, neg, np.float32),
                 best_seq=np.zeros((NI, LMAX), np.int64), best_len=np.zeros(NI, np.int32))
        g = {n: Guarded(v) for n, v in h.items()}
        g["seqs2"], g["words"], g["rows"] = Guarded(h["seqs"]), Guarded(np.zeros(NI * k, np.int64)), Guarded(np.zeros(NI * k, np.int32))
        a_d, b_d = torch.from_numpy(lg[0]).to(DEV), torch.from_numpy(lg[1]).to(DEV)
        rc = lib.set_beam_pick_f32(L.ptr(a_d), L.ptr(b_d), ld, NI, k, V, end, 2, LMAX, *(C.c_void_p(g[n].ptr) for n in (
            "scores", "k_left", "seqs", "seqs2", "best_score", "best_seq", "best_len", "words", "rows")), L.stream_of(torch.device(DEV)))
        assert rc == 0
        torch.cuda.synchronize()
        flags = dict(picks=[])
        out, w_np, r_np = PO.beam_pick(lg[0], h["scores"], h["k_left"], h["seqs"], h["best_score"], h["best_seq"], h["best_len"],
                                       None, None, None, None, 2, flags, k, V, end, logits2=lg[1])
        for i, kl, picks, cand in flags["picks"]:
            gaps = np.diff([nv for nv, f in cand[:k + 1]])
            assert (gaps >= 0.25).all(), ("the inputs do not keep their candidates apart", i, gaps)
        assert np.array_equal(g["words"].get(), w_np) and np.array_equal(g["rows"].get(), r_np)
        assert np.array_equal(g["k_left"].get(), h["k_left"]) and np.array_equal(g["best_len"].get(), h["best_len"])
        assert np.array_equal(g["best_seq"].get(), h["best_seq"]) and (h["k_left"] < k).all()
        assert np.array_equal(g["seqs2"].get()[:, :, :3], out[:, :, :3])
        for name in ("scores", "best_score"):
            got, want = g[name].get(), h[name]
            assert np.array_equal(np.isinf(got), np.isinf(want)), name
            fin = np.isfinite(want)
            assert float(np.abs(got[fin] - want[fin]).max()) <= LOGP_TOL, (name, got, want)
