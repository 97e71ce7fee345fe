"""GPU: the constrained greedy and sampled picks (csrc/epilogue.hip, CONS instantiations) through
set_pick_slabs_constrained_f32, one launch per case on the fixtures of tests/pick_constrained_oracle.py, against the float64
restatement there.  tests/test_pick_constrained_cpu.py has shown on the oracle alone that no fixture row sits near a tie or a CDF /
top-p boundary, so every row is compared: words and bookkeeping exactly, seq_logp / lse / step_logp within the tolerance of
tests/test_hip_pick_epilogues.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import pick_constrained_oracle as PCO
import pick_oracle as PO
import test_hip_pick_epilogues as PE
import trunc_sample_oracle as TS

pytestmark = pytest.mark.gpu
SEED, OFFSET = 2024, 5                       # (the draws tests/test_pick_constrained_cpu.py pinned)
CASES = PCO.pick_cases()
IDS = [c.name for c in CASES]


def rollout_at(B, max_len, hist, unf, t, D=0):
    """a PE.Rollout whose state is that of a rollout about to take step t: seq = hist, the latches, alive[t - 1] = rows alive"""
    ro = PE.Rollout.__new__(PE.Rollout)
    ro.B, ro.max_len, ro.D = B, max_len, D
    st = ro.st = PO.new_state(B, max_len, None, fill=PE.FILL)
    st["seq"][:, :t] = hist[:, :t]
    st["seq_logp"][:, :t] = -1.0
    st["unf"][:] = unf
    if t > 0:
        st["alive"][:t] = max(int(unf.sum()), 1)
        st["it"][:] = np.where(unf != 0, hist[:, t - 1], 0)
    G = PE.Guarded
    ro.seq, ro.seq_logp = G(st["seq"]), G(st["seq_logp"].astype(np.float32))
    ro.it, ro.unf, ro.alive = G(st["it"]), G(st["unf"]), G(st["alive"])
    ro.emb = G(np.full((B, max(D, 1)), -7.0, np.float32))
    ro.emb_want = np.full((B, max(D, 1)), -7.0, np.float32)
    ro.raw, ro.lse, ro.lp = G(np.full(B, -5, np.int64)), G(np.full(B, -5.0, np.float32)), G(np.full(B, -5.0, np.float32))
    return ro


def cons_struct(cons):
    L, _ = PE._lib()
    ids = torch.tensor(list(cons.banned), dtype=torch.long, device=PE.DEV) if cons.banned else None
    return L.BeamConstraintsC(cons.ngram, cons.min_len, 0.0, len(cons.banned), ids.data_ptr() if cons.banned else None), ids


def launch(ro, slabs, bias, V, t, end, cons, *, ld, mode=0, opts=None, E=None, entry="constrained"):
    """one call of set_pick_slabs_constrained_f32 (entry="opts": set_pick_slabs_opts_f32 on the same arguments)"""
    L, lib = PE._lib()
    slabs = np.asarray(slabs, np.float32)
    lt, lp, stride = PE.padded(slabs, ld)
    a = L.PickArgs(logits=lp, ld=ld, stride=stride, end_idx=end, seq=ro.seq.ptr, seq_logp=ro.seq_logp.ptr, it=ro.it.ptr,
                   unfinished=ro.unf.ptr, alive=ro.alive.ptr, seed=SEED, offset=OFFSET, raw_ids=ro.raw.ptr, lse=ro.lse.ptr,
                   step_logp=ro.lp.ptr, n=slabs.shape[0], B=ro.B, V=V, t=t, max_len=ro.max_len, D=ro.D, mode=mode)
    hold = [lt]
    if bias is not None:
        bt, bp, _ = PE.padded(np.asarray(bias, np.float32)[None, None, :], V)
        a.bias = bp
        hold.append(bt)
    if E is not None:
        et = torch.from_numpy(np.ascontiguousarray(E, np.float32)).to(PE.DEV)
        a.table, a.emb_out = et.data_ptr(), ro.emb.ptr
        hold.append(et)
    o = L.SampleOpts(temperature=opts[0], top_k=opts[1], top_p=opts[2]) if opts is not None else None
    st = L.stream_of(torch.device(PE.DEV))
    if entry == "opts":
        rc = lib.set_pick_slabs_opts_f32(C.byref(a), C.byref(o) if o else None, st)
    else:
        cs, ids = cons_struct(cons)
        hold.append(ids)
        rc = lib.set_pick_slabs_constrained_f32(C.byref(a), C.byref(o) if o else None, C.byref(cs), st)
    torch.cuda.synchronize()
    del hold
    return rc


def outputs(ro):
    return [g.get() for g in (ro.seq, ro.seq_logp, ro.it, ro.unf, ro.alive, ro.emb, ro.raw, ro.lse, ro.lp)]


def run_greedy(c, D=8):
    E = np.random.default_rng(c.V).standard_normal((c.V, D)).astype(np.float32)
    ro = rollout_at(c.B, c.max_len, c.hist, c.unf, c.t, D)
    assert launch(ro, c.slabs, c.bias, c.V, c.t, c.end, c.cons, ld=c.ld, E=E) == 0
    words = PCO.greedy_step(PCO.x64_of(c), c.t, c.max_len, c.end, ro.st, c.cons)
    ro.emb_want = PO.relu_embed(E, ro.st["it"]).astype(np.float32)
    ro.check(("constrained greedy", c.name))
    return ro, words


def run_sample(c, opts):
    ro = rollout_at(c.B, c.max_len, c.hist, c.unf, c.t)
    assert launch(ro, c.slabs, c.bias, c.V, c.t, c.end, c.cons, ld=c.ld, mode=1, opts=None if opts == TS.NEUTRAL else opts) == 0
    d, logp, broken = PCO.sample_step(c.x32, opts, SEED, OFFSET, c.t, PCO.case_reg(c), c.max_len, c.end, ro.st, c.cons)
    assert not broken
    what = ("constrained sample", c.name, opts)
    assert np.array_equal(ro.raw.get(), d.ids), (what, ro.raw.get(), d.ids, d.margin)
    assert np.array_equal(ro.seq.get(), ro.st["seq"]) and np.array_equal(ro.it.get(), ro.st["it"]), what
    assert np.array_equal(ro.unf.get(), ro.st["unf"]) and np.array_equal(ro.alive.get(), ro.st["alive"]), what
    e_lp = float(np.abs(ro.lp.get() - logp).max())
    e_lse = float(np.abs(ro.lse.get() - d.lse).max())
    e_seq = float(np.abs(ro.seq_logp.get()[:, c.t] - logp).max())
    print(what, "step_logp err %.2e lse err %.2e" % (e_lp, e_lse))
    assert max(e_lp, e_lse, e_seq) <= PE.LOGP_TOL, (what, e_lp, e_lse, e_seq)
    return ro


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_constrained_greedy(c):
    """arg-max, tie rule, log-softmax of the masked row; seq, it, unfinished, alive and relu(E[it]) exact on every row"""
    ro, words = run_greedy(c)
    live = (c.unf != 0) | (c.t == 0)
    m = PCO.masked(PCO.x64_of(c), c.hist, c.unf, c.t, c.end, c.cons)
    assert np.isfinite(m[np.arange(c.B), words]).all()
    if c.name != "n16_cannot":
        assert (words[live] != np.argmax(PCO.x64_of(c), 1)[live]).any(), "the constraints changed no row"


@pytest.mark.parametrize("opts", PCO.SAMPLE_OPTS, ids=["neutral", "top_k", "top_p", "t_k_p"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_constrained_sample(c, opts):
    """the draw over the masked row under temperature / top-k / top-p equals the oracle's; step_logp, lse under that distribution"""
    run_sample(c, opts)


def test_both_layouts_give_the_same_bits():
    """V = 9490 read with ld = 9490 (scalar) and ld = 9492 (float4): the outputs of every LIVE row — greedy, sampled, sampled under
    truncation — are equal bit for bit (the finished row is the unconstrained pick's, which has one summation order per layout)"""
    a, b = [c for c in CASES if c.name in ("v9490_scalar", "v9490_reg")]
    assert np.array_equal(a.slabs, b.slabs) and not PCO.case_reg(a) and PCO.case_reg(b)
    live = np.flatnonzero(a.unf != 0)
    rows = lambda ro: [x[live].view(np.uint8) for x in outputs(ro) if x.shape[0] == a.B]
    for x, y in zip(rows(run_greedy(a)[0]), rows(run_greedy(b)[0])):
        assert np.array_equal(x, y)
    for opts in PCO.SAMPLE_OPTS:
        for x, y in zip(rows(run_sample(a, opts)), rows(run_sample(b, opts))):
            assert np.array_equal(x, y), opts


@pytest.mark.parametrize("name", ["reg_last_size", "scalar_by_V", "v9490_reg", "n2_far"])
@pytest.mark.parametrize("mode,opts", [(0, None), (1, None), (1, (0.8, 50, 0.9))])
def test_neutral_constraints_are_the_unconstrained_pick_bit_for_bit(name, mode, opts):
    c = [c for c in CASES if c.name == name][0]
    got = []
    for entry in ("opts", "constrained"):
        ro = rollout_at(c.B, c.max_len, c.hist, c.unf, c.t)
        assert launch(ro, c.slabs, c.bias, c.V, c.t, c.end, PCO.Cons(), ld=c.ld, mode=mode, opts=opts, entry=entry) == 0
        got.append(outputs(ro))
    for x, y in zip(*got):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_finished_rows_get_the_unconstrained_pick():
    """the finished row of a fixture, greedy and sampled: its outputs equal those of set_pick_slabs_opts_f32 bit for bit"""
    c = [c for c in CASES if c.name == "reg_last_size"][0]
    r = int(np.flatnonzero(c.unf == 0)[0])
    for mode in (0, 1):
        got = []
        for entry in ("opts", "constrained"):
            ro = rollout_at(c.B, c.max_len, c.hist, c.unf, c.t)
            assert launch(ro, c.slabs, c.bias, c.V, c.t, c.end, c.cons, ld=c.ld, mode=mode, entry=entry) == 0
            got.append((ro.seq_logp.get()[r], ro.raw.get()[r], ro.lse.get()[r], ro.lp.get()[r], ro.it.get()[r]))
        for x, y in zip(*got):
            assert np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8))


TIE_V = {"reg": (1028, 1028), "scalar": (1027, 1029)}


@pytest.mark.parametrize("path", ["reg", "scalar"])
@pytest.mark.parametrize("n", [1, 3])
def test_ties_on_integer_logits(path, n):
    """exact ties (integer logits): row 0's maximum at a banned word AND a later word -> the later word; row 1 all equal ->
    the first word that is not removed; row 2's maximum at <end> under min_len -> the runner-up; row 3 tied at a word rule c
    removes (n-gram 2) and a later one"""
    V, ld = TIE_V[path]
    rng = np.random.default_rng(n)
    B, t, max_len, end = 4, 3, 6, 900
    slabs = PE.int_slabs(rng, n, B, V, -8, 2)
    slabs[:, 0, 40] = slabs[:, 0, 700] = 5
    slabs[:, 1, :] = 1
    slabs[:, 2, end] = 6
    slabs[:, 2, 333] = 4
    slabs[:, 3, 12] = slabs[:, 3, 1020] = 5
    bias = np.zeros(V, np.float32)
    hist = np.zeros((B, max_len), np.int64)
    hist[:, :t] = [[50, 60, 70], [0, 1, 0], [50, 60, 70], [9, 12, 9]]          # row 1: (0, 1) seen, ends in 0 -> 1 removed
    cons = PCO.Cons(2, 4, [40, 2])
    ro = rollout_at(B, max_len, hist, np.ones(B, np.int32), t)
    assert launch(ro, slabs, bias, V, t, end, cons, ld=ld) == 0
    words = PCO.greedy_step(PO.slab_logits(slabs, bias, V), t, max_len, end, ro.st, cons)
    assert words.tolist() == [700, 0, 333, 1020]
    ro.check(("ties", path, n))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("g0n,with_pre,TD", [(1, False, 64), (3, True, 1028)])
def test_pick_tail_under_constraints(monkeypatch, g0n, with_pre, TD, mode):
    """the LstmTail inside the constrained instantiations: the tail cases of tests/test_hip_pick_epilogues.py (V = 6, max_len 3)
    launched through the constrained entry with a word banned that no row of the case prefers (word 1; word 2 in the latched
    case, whose first step picks word 1), so the expected cell is unchanged"""
    L, lib = PE._lib()
    ids = torch.tensor([1, 2], dtype=torch.long, device=PE.DEV)
    for latched in (False, True):
        cs = L.BeamConstraintsC(0, 0, 0.0, 1, ids.data_ptr() + 8 * int(latched))
        monkeypatch.setattr(lib, "set_pick_slabs_f32", lambda a, st, cs=cs: lib.set_pick_slabs_constrained_f32(a, None, C.byref(cs), st))
        PE._tail_case(mode, g0n, with_pre, TD, seed=g0n * 7 + TD + int(latched), latched=latched)
