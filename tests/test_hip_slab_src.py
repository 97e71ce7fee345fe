"""GPU: the six consumers of split-K partials (include/set_hip.h: the *_src_f32 entry points, SrcList::load4 of
csrc/set_common.h) and set_gemm_group_slabs_f32, each ALONE on hand-made partials.

Every consumer is checked twice.  (i) Against float64: the closed form of tests/slab_src_oracle.py (pinned to autograd by
tests/test_slab_src_oracle_cpu.py) applied to the float64 sum of the addends, within the bound of
tests/test_hip_backward_ops.py for fused operators (1e-4 of max|ref| per output + 1e-6 of the largest).  (ii) Bit for bit
against the plain entry point fed the documented fp32 sum ("slab order, then list order") as its gradient: the summation is
the only difference between the two.

Every entry's buffer holds M rows even when it declares fewer; the rows at and beyond `rows` and the padding columns of a
wider row stride are NaN, inside the test's own allocation: a kernel that reads what it must not yields a non-finite output."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import slab_src_oracle as SO
from slab_src_oracle import Entry
from test_hip_backward_ops import FUSED, check, gap_ok, ktol, no_kink, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SHAPES = [(M, D) for M in (1, 5, 70) for D in (4, 8, 260)]          # D = 260: 65 float4 per row, 256-thread blocks straddle rows
SEED, OFFSET = 0x1_2345_6789, (3 << 40) | 5

# ---------------------------------------------------------------------------------------------------------------------
# the lists of addends
# ---------------------------------------------------------------------------------------------------------------------
DEPTHS = (1, 2, 3, 4, 5, 8, 9)                                       # both sides of load4's batches of four
NO_BASE = ["nslab%d" % n for n in DEPTHS] + ["unsplit", "four", "magnitudes", "nothing"]
WITH_BASE = NO_BASE + ["base_only", "base_two"]


def _partials(gen, nslab, M, D, rows=None, ld=None):
    rows, ld = M if rows is None else rows, D if ld is None else ld
    t = torch.full((nslab, M, ld), NAN)
    t[:, :rows, :D] = rnd(gen, nslab, rows, D).float()
    return Entry(t, rows, nslab)


def make_case(case, M, D):
    """-> (base (M, D) fp32 or None, [Entry])"""
    gen = torch.Generator().manual_seed(1000 * M + D + sum(map(ord, case)))
    if case.startswith("nslab"):
        return None, [_partials(gen, int(case[5:]), M, D)]
    if case == "unsplit":                                            # the whole product as one "partial", as the Python loop passes it
        return None, [_partials(gen, 1, M, D)._replace(slab_stride=0)]
    if case == "four":                                               # different depths, an empty entry, rows that have left, a padded stride
        return None, [_partials(gen, 3, M, D), Entry(None, 0, 0), _partials(gen, 5, M, D, rows=max(M - 2, 0), ld=D + 4),
                      _partials(gen, 1, M, D, rows=1)]
    if case == "magnitudes":                                         # 1e4 u - 1e4 u + 1e-3 w: any other order of the adds loses w's bits
        u, w = rnd(gen, M, D).float(), rnd(gen, M, D).float()
        return None, [Entry(torch.stack([1e4 * u, -(1e4 * u), 1e-3 * w]), M, 3)]
    if case == "nothing":
        return None, []
    if case == "base_only":
        return rnd(gen, M, D).float(), []
    if case == "base_two":
        return rnd(gen, M, D).float(), [_partials(gen, 2, M, D), _partials(gen, 6, M, D)]
    raise KeyError(case)


def test_the_cases_are_what_they_claim():
    for M, D in SHAPES:
        _, ent = make_case("four", M, D)
        assert [(e.nslab, e.rows) for e in ent] == [(3, M), (0, 0), (5, max(M - 2, 0)), (1, 1)] and ent[2].t.shape[2] == D + 4
        assert all(e.t is None or e.t.shape[1] == M for e in ent) and ent[1].t is None
        assert bool(torch.isnan(ent[2].t[:, max(M - 2, 0):]).all()) and bool(torch.isnan(ent[2].t[:, :, D:]).all())
        assert M == 1 or bool(torch.isnan(ent[3].t[:, 1:]).all())
        for case in WITH_BASE:
            base, ent = make_case(case, M, D)
            assert bool(torch.isfinite(SO.ordered_sum32(base, ent, M, D)).all()) and len(ent) <= 4
        _, ent = make_case("magnitudes", M, D)
        assert torch.equal(SO.ordered_sum32(None, ent, M, D), ent[0].t[2])
        assert not torch.equal(ent[0].t[0] + ent[0].t[2] + ent[0].t[1], ent[0].t[2])


class Run:
    """one gradient: base + entries on the device, its two sums on the host"""

    def __init__(self, case, M, D):
        self.base, self.entries = make_case(case, M, D)
        self.g32, self.g64 = SO.ordered_sum32(self.base, self.entries, M, D), SO.sum64(self.base, self.entries, M, D)
        self.arr, self.n, self.keep = SO.src_array(self.entries, DEV)
        self.base_d = None if self.base is None else self.base.to(DEV)
        self.g32_d = self.g32.to(DEV)
        self.st = lib_stream()

    @property
    def base_p(self):
        return None if self.base_d is None else self.base_d.data_ptr()


def lib_stream():
    from show_edit_tell_amd import _lib
    return _lib.stream_of(torch.device(DEV))


def lib():
    from show_edit_tell_amd import _lib
    return _lib.load()


def up(t):
    return t.float().to(DEV).contiguous()


def f64(t):
    return t.float().double()


def judge(what, src, plain, ref, bitwise=True):
    """src / plain: {name: device tensor}, ref: {name: float64 tensor}; prints the largest float64 error of each output"""
    torch.cuda.synchronize()
    for name, t in src.items():
        assert bool(torch.isfinite(t).all()), (what, name, "non-finite output")
    named = [(name, src[name], ref[name], None) for name in ref]
    scale = {name: float(r.abs().max()) for name, r in ref.items()}
    worst = max((float((src[n].double().cpu() - ref[n]).abs().max()) / scale[n] for n in ref if scale[n] > 0), default=0.0)
    print("%s: largest float64 error %.3e of max|ref| (bound %.0e)" % (what, worst, FUSED))
    check(named, FUSED, what)
    if bitwise:
        for name in src:
            assert torch.equal(src[name], plain[name]), (what, name, "differs from the plain form fed the ordered fp32 sum",
                                                         float((src[name] - plain[name]).abs().max()))


def rc0(rc, what):
    assert rc == 0, (what, rc)


# ---------------------------------------------------------------------------------------------------------------------
# operator inputs (the saved tensors of the train-mode forward), made once per shape
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cell_inputs(M, D):
    gen = torch.Generator().manual_seed(100 * M + D)
    z = rnd(gen, M, 4 * D, scale=2.0)
    i, f, g, o = z.chunk(4, 1)
    gates = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], 1).float()
    c_prev = rnd(gen, M, D).float()
    g64 = f64(gates)
    c_new = (g64[:, D:2 * D] * c_prev.double() + g64[:, :D] * g64[:, 2 * D:3 * D]).float()
    d = dict(gates=gates, c_prev=c_prev, c_new=c_new, dc=rnd(gen, M, D).float(), do_pre=rnd(gen, M, D).float(),
             adp=rnd(gen, M, D).float(), cg=torch.sigmoid(rnd(gen, M, D, scale=2.0)).float(), cmem=rnd(gen, M, D).float(),
             dadp=rnd(gen, M, D).float(), zt=torch.sigmoid(rnd(gen, M, D, scale=2.0)).float(),
             s=torch.tanh(rnd(gen, M, D, scale=2.0)).float(), t=torch.tanh(rnd(gen, M, D, scale=2.0)).float())
    drop = torch.full((M, D + 4), NAN)                                # ld_drop = D + 4
    drop[:, :D] = rnd(gen, M, D).float()
    d["dh_drop"] = drop
    return d


@pytest.mark.parametrize("M,D", SHAPES)
@pytest.mark.parametrize("case", NO_BASE)
def test_lstm_cell(case, M, D):
    I, R = cell_inputs(M, D), Run(case, M, D)
    for with_dc in (True, False):
        dev = {k: up(I[k]) for k in ("gates", "c_prev", "c_new", "dc")}
        dcp = dev["dc"].data_ptr() if with_dc else None
        outs = []
        for src in (True, False):
            dg, dc_prev = torch.full((M, 4 * D), NAN, device=DEV), torch.full((M, D), NAN, device=DEV)
            tail = (dcp, dev["gates"].data_ptr(), dev["c_prev"].data_ptr(), dev["c_new"].data_ptr(), dg.data_ptr(),
                    dc_prev.data_ptr(), M, D, R.st)
            if src:
                rc0(lib().set_lstm_cell_bwd_src_f32(R.arr, R.n, *tail), "set_lstm_cell_bwd_src_f32")
            else:
                rc0(lib().set_lstm_cell_bwd_f32(R.g32_d.data_ptr(), *tail), "set_lstm_cell_bwd_f32")
            outs.append(dict(dgates=dg, dc_prev=dc_prev))
        r = SO.lstm_cell_bwd(R.g64, f64(I["dc"]) if with_dc else None, f64(I["gates"]), f64(I["c_prev"]), f64(I["c_new"]))
        judge("lstm_cell %s M=%d D=%d dc=%d" % (case, M, D, with_dc), outs[0], outs[1], dict(dgates=r[0], dc_prev=r[1]))


@pytest.mark.parametrize("M,D", SHAPES)
@pytest.mark.parametrize("case", NO_BASE)
def test_copy_gate(case, M, D):
    """the o-gate is read from the (M, 4D) gate block (ld_ogate = 4D); dh_drop has ld_drop = D + 4.  Bit equality where the
    summation is the only difference (no dh_drop, or p = 0 with dh_drop added after the addends); under p > 0 float64 only."""
    I, R = cell_inputs(M, D), Run(case, M, D)
    names = ("gates", "adp", "cg", "cmem", "c_new", "dadp", "dh_drop")
    dev = {k: up(I[k]) for k in names}
    og = dev["gates"][:, 3 * D:]
    for drop, p in ((False, 0.0), (True, 0.0), (True, 0.5)):
        outs = []
        for src in (True, False):
            o = [torch.full((M, D), NAN, device=DEV) for _ in range(4)]
            mid = (dev["dadp"].data_ptr(), og.data_ptr(), 4 * D, dev["adp"].data_ptr(), dev["cg"].data_ptr(), dev["cmem"].data_ptr(),
                   dev["c_new"].data_ptr(), *[x.data_ptr() for x in o], M, D, R.st)
            if src:
                rc0(lib().set_copy_gate_bwd_src_f32(R.arr, R.n, dev["dh_drop"].data_ptr() if drop else None, D + 4, p, SEED, OFFSET,
                                                    *mid), "set_copy_gate_bwd_src_f32")
            else:
                dh = R.g32_d + dev["dh_drop"][:, :D] if drop else R.g32_d      # p = 0: added as it is, after the addends
                rc0(lib().set_copy_gate_bwd_ld_f32(dh.contiguous().data_ptr(), *mid), "set_copy_gate_bwd_ld_f32")
            outs.append(dict(zip(("du", "dcm_direct", "dcn_direct", "do_pre"), o)))
        dh64 = R.g64 + (SO.dropout_bwd(f64(I["dh_drop"][:, :D]), SEED, OFFSET, p) if drop else 0)
        r = SO.copy_gate_bwd(dh64, f64(I["dadp"]), f64(I["gates"][:, 3 * D:]), f64(I["adp"]), f64(I["cg"]), f64(I["cmem"]),
                             f64(I["c_new"]))
        judge("copy_gate %s M=%d D=%d drop=%d p=%.1f" % (case, M, D, drop, p), outs[0], outs[1],
              dict(zip(("du", "dcm_direct", "dcn_direct", "do_pre"), r)), bitwise=p == 0.0)


@pytest.mark.parametrize("M,D", SHAPES)
@pytest.mark.parametrize("case", WITH_BASE)
def test_lstm_gates(case, M, D):
    I, R = cell_inputs(M, D), Run(case, M, D)
    _lstm_gates(I, R, M, D, "lstm_gates %s M=%d D=%d" % (case, M, D))


def _lstm_gates(I, R, M, D, what, arr=None, n=None):
    dev = {k: up(I[k]) for k in ("do_pre", "gates", "c_prev")}
    outs = []
    for src in (True, False):
        dg, dc_prev = torch.full((M, 4 * D), NAN, device=DEV), torch.full((M, D), NAN, device=DEV)
        tail = (dev["do_pre"].data_ptr(), dev["gates"].data_ptr(), dev["c_prev"].data_ptr(), dg.data_ptr(), dc_prev.data_ptr(), M, D, R.st)
        if src:
            rc0(lib().set_lstm_gates_bwd_src_f32(R.base_p, R.arr if arr is None else arr, R.n if n is None else n, *tail),
                "set_lstm_gates_bwd_src_f32")
        else:
            rc0(lib().set_lstm_gates_bwd_f32(R.g32_d.data_ptr(), *tail), "set_lstm_gates_bwd_f32")
        outs.append(dict(dgates=dg, dc_prev=dc_prev))
    r = SO.lstm_gates_bwd(R.g64, f64(I["do_pre"]), f64(I["gates"]), f64(I["c_prev"]))
    judge(what, outs[0], outs[1], dict(dgates=r[0], dc_prev=r[1]))


@pytest.mark.parametrize("M,D", SHAPES)
@pytest.mark.parametrize("case", WITH_BASE)
def test_context_gate(case, M, D):
    """the three outputs are column blocks of one (M, 3D) buffer, ld_out = 3D, in the order xe_sequence.py uses: ds | dz | dt"""
    I, R = cell_inputs(M, D), Run(case, M, D)
    dev = {k: up(I[k]) for k in ("zt", "s", "t")}
    outs = []
    for src in (True, False):
        buf = torch.full((M, 3 * D), NAN, device=DEV)
        tail = (dev["zt"].data_ptr(), dev["s"].data_ptr(), dev["t"].data_ptr(), buf[:, D:].data_ptr(), buf.data_ptr(),
                buf[:, 2 * D:].data_ptr(), 3 * D, M, D, R.st)
        if src:
            rc0(lib().set_context_gate_bwd_src_f32(R.base_p, R.arr, R.n, *tail), "set_context_gate_bwd_src_f32")
        else:
            rc0(lib().set_context_gate_bwd_ld_f32(R.g32_d.data_ptr(), *tail), "set_context_gate_bwd_ld_f32")
        outs.append(dict(ds=buf[:, :D], dz=buf[:, D:2 * D], dt=buf[:, 2 * D:]))
    dz, ds, dt = SO.context_gate_bwd(R.g64, f64(I["zt"]), f64(I["s"]), f64(I["t"]))
    judge("context_gate %s M=%d D=%d" % (case, M, D), outs[0], outs[1], dict(dz=dz, ds=ds, dt=dt))


@functools.lru_cache(maxsize=None)
def select_inputs(M, T, D):
    gen = torch.Generator().manual_seed(M * 10 + T + D)
    Mem = rnd(gen, M, T, D).float()
    alpha = F.softmax(rnd(gen, M, T, scale=3.0), 1).float()
    if T > 1:
        gap_ok(alpha.double())
    return dict(Mem=Mem, alpha=alpha, dM0=rnd(gen, M, T, D).float())


@pytest.mark.parametrize("T", [1, 9])
@pytest.mark.parametrize("M,D", SHAPES)
@pytest.mark.parametrize("case", WITH_BASE)
def test_select(case, M, D, T):
    """dM is prefilled: with acc_dM = 0 all of it is overwritten, with acc_dM = 1 only the selected row may change"""
    I, R = select_inputs(M, T, D), Run(case, M, D)
    dev = {k: up(I[k]) for k in ("Mem", "alpha")}
    sel = I["alpha"].argmax(1)
    for acc in (0, 1):
        outs = []
        for src in (True, False):
            dM, dal = up(I["dM0"]), torch.full((M, T), NAN, device=DEV)
            tail = (dev["Mem"].data_ptr(), dev["alpha"].data_ptr(), dM.data_ptr(), dal.data_ptr(), M, T, D, acc, R.st)
            if src:
                rc0(lib().set_select_bwd_src_f32(R.base_p, R.arr, R.n, *tail), "set_select_bwd_src_f32")
            else:
                rc0(lib().set_select_bwd_acc_f32(R.g32_d.data_ptr(), *tail), "set_select_bwd_acc_f32")
            outs.append(dict(dM=dM, dalpha=dal))
        dM64, dal64 = SO.select_bwd(R.g64, f64(I["Mem"]), f64(I["alpha"]), f64(I["dM0"]) if acc else None)
        judge("select %s M=%d T=%d D=%d acc=%d" % (case, M, T, D, acc), outs[0], outs[1], dict(dM=dM64, dalpha=dal64))
        if acc:
            other = torch.ones(M, T, dtype=torch.bool)
            other[torch.arange(M), sel] = False
            assert torch.equal(outs[0]["dM"].cpu()[other], I["dM0"][other])


ATT_SHAPES = [(M, 1, 4, 4) for M in (1, 5, 70)] + [(M, 7, 64, 32) for M in (1, 5, 70)] + [(M, 36, 2048, 64) for M in (1, 5)]


@functools.lru_cache(maxsize=None)
def attention_inputs(M, L, Dv, A, tanh):
    gen = torch.Generator().manual_seed(M + 10 * L + Dv + A)
    V = rnd(gen, M, L, Dv).float()
    att1, att2 = rnd(gen, M, L, A, scale=2.0).float(), rnd(gen, M, A, scale=2.0).float()
    w = rnd(gen, A, scale=4 / math.sqrt(A)).float()
    pre = f64(att1) + f64(att2).unsqueeze(1)
    if not tanh:
        no_kink(pre, f64(att1), f64(att2).unsqueeze(1).expand_as(pre))
    e = ((torch.tanh(pre) if tanh else torch.relu(pre)) * f64(w)).sum(2)
    alpha = F.softmax(e, 1).float()                          # the kernel's alpha input: the float64 softmax rounded once
    return dict(V=V, att1=att1, att2=att2, w=w, alpha=alpha, dal=rnd(gen, M, L).float(), datt1_0=rnd(gen, M, L, A).float(),
                datt2_0=rnd(gen, M, 2 * A).float())


@pytest.mark.parametrize("tanh", [0, 1], ids=["relu", "tanh"])
@pytest.mark.parametrize("M,L,Dv,A", ATT_SHAPES)
@pytest.mark.parametrize("case", WITH_BASE)
def test_attention(case, M, L, Dv, A, tanh):
    """as xe_sequence.py calls it: the caption form with dalpha_ext and dctx_out, the visual form with neither; acc_datt1 0 and 1
    onto a prefilled datt1; datt2 into the second half of an (M, 2A) buffer (ld_datt2 = 2A) whose first half keeps its prefill.
    dctx_out is the summed gradient itself: the ordered fp32 sum bit for bit."""
    I, R = attention_inputs(M, L, Dv, A, tanh), Run(case, M, Dv)
    dev = {k: up(I[k]) for k in ("V", "att1", "att2", "w", "alpha", "dal")}
    for ext in (False, True):
        r = SO.attention_bwd(R.g64, f64(I["dal"]) if ext else None, f64(I["alpha"]), f64(I["V"]), f64(I["att1"]), f64(I["att2"]),
                             f64(I["w"]), bool(tanh))
        for acc in (0, 1):
            outs = []
            for src in (True, False):
                datt1, datt2 = up(I["datt1_0"]), up(I["datt2_0"])
                dwf, de = torch.full((M, A), NAN, device=DEV), torch.full((M, L), NAN, device=DEV)
                dctx_out = torch.full((M, Dv), NAN, device=DEV) if (ext and src) else None
                ins = (dev["dal"].data_ptr() if ext else None, dev["alpha"].data_ptr(), dev["V"].data_ptr(), dev["att1"].data_ptr(),
                       dev["att2"].data_ptr(), dev["w"].data_ptr(), datt1.data_ptr(), datt2[:, A:].data_ptr(), dwf.data_ptr())
                if src:
                    rc0(lib().set_attention_bwd_src_f32(R.base_p, R.arr, R.n, None if dctx_out is None else dctx_out.data_ptr(), *ins,
                                                        de.data_ptr(), M, L, Dv, A, tanh, acc, 2 * A, R.st), "set_attention_bwd_src_f32")
                else:
                    rc0(lib().set_attention_bwd_acc_f32(R.g32_d.data_ptr(), *ins, None, de.data_ptr(), M, L, Dv, A, tanh, acc, 0, 2 * A,
                                                        R.st), "set_attention_bwd_acc_f32")
                outs.append(dict(datt1=datt1, datt2=datt2[:, A:], dwfull_part=dwf, de=de))
                torch.cuda.synchronize()
                assert torch.equal(datt2[:, :A].cpu(), I["datt2_0"][:, :A])
                if dctx_out is not None:
                    assert torch.equal(dctx_out.cpu(), R.g32), "dctx_out is not the ordered fp32 sum"
            ref = dict(datt1=r[0] + (f64(I["datt1_0"]) if acc else 0), datt2=r[1], dwfull_part=r[2], de=r[3])
            judge("attention %s M=%d L=%d Dv=%d A=%d tanh=%d ext=%d acc=%d" % (case, M, L, Dv, A, tanh, ext, acc), outs[0], outs[1], ref)


# ---------------------------------------------------------------------------------------------------------------------
# set_gemm_group_slabs_f32: the producer of such lists
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = {   # (M, N, K); K = 128 is never split (4 k-tiles); N = 66 cannot be split (no float4 rows) and must land in C
    (0, 1): [[(5, 64, 512)], [(1, 68, 128), (70, 64, 1024)], [(70, 68, 2080), (5, 64, 128), (1, 64, 512)],
             [(5, 68, 1024), (70, 64, 512), (1, 64, 2080), (70, 64, 128)]],
    (0, 0): [[(5, 64, 512), (5, 66, 1024)], [(1, 68, 128), (70, 64, 1024)], [(70, 68, 2080), (5, 64, 128), (1, 66, 512), (1, 64, 512)],
             [(5, 68, 1024), (70, 66, 2080), (1, 64, 2080), (70, 64, 128)]],
}
WS_MODES = ("three", "under_two", "generous")
GEMM_PARAMS = [(lay, gi, mode) for lay in GROUPS for gi in range(len(GROUPS[lay])) for mode in WS_MODES]


def _slab_bytes(M, N):
    return -(-M * N * 4 // 256) * 256


def _can_split(M, N, K):
    return K >= 256 and N % 4 == 0


@functools.lru_cache(maxsize=None)
def gemm_run(layout, gi, mode):
    """-> per problem: dict(shape, out = (p offset in ws, slab_stride, ld, nslab, rows), partials (nslab, M, N) or None,
    C after accumulate = 0 / 1, C of set_gemm_group_f32, the float64 product, the prefilled C)"""
    from show_edit_tell_amd import _lib
    L, st = lib(), lib_stream()
    probs = GROUPS[layout][gi]
    n = len(probs)
    split = [q for q in probs if _can_split(*q)]
    if mode == "three":                                    # exactly 3 slabs of the first problem that can be split
        ws_bytes = 3 * _slab_bytes(*split[0][:2])
    elif mode == "under_two":                              # fewer than 2 slabs of the smallest: everything falls back to C
        ws_bytes = 2 * min(_slab_bytes(M, N) for M, N, _ in split) - 256
    else:
        ws_bytes = 32 << 20
    gen = torch.Generator().manual_seed(1000 * gi + 10 * layout[1] + len(mode))
    As = [rnd(gen, M, K).float() for M, N, K in probs]
    Bs = [(rnd(gen, K, N) if layout[1] else rnd(gen, N, K)).float() / math.sqrt(K) for M, N, K in probs]
    C0 = [rnd(gen, M, N).float() for M, N, K in probs]
    Ad, Bd = [a.to(DEV) for a in As], [b.to(DEV) for b in Bs]

    def call(fn, accumulate, Cd, ws, outs=None):
        descs = (_lib.GemmDesc * n)()
        for i, (M, N, K) in enumerate(probs):
            descs[i] = _lib.GemmDesc(Ad[i].data_ptr(), K, Bd[i].data_ptr(), Bs[i].shape[1], Cd[i].data_ptr(), N, M, N, K, accumulate)
        extra = (outs, st) if outs is not None else (st,)
        rc0(fn(descs, n, layout[0], layout[1], ws.data_ptr(), ws_bytes, *extra), fn.__name__)
        torch.cuda.synchronize()

    res, ws_all, outs_all = [dict(shape=q) for q in probs], [], []
    for accumulate in (0, 1):
        ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)           # (all-ones words are NaN)
        Cd = [c.to(DEV).clone() for c in C0]
        outs = (_lib.SlabSrc * n)()
        call(L.set_gemm_group_slabs_f32, accumulate, Cd, ws, outs)
        ws_all.append(ws)
        outs_all.append([(o.p, o.slab_stride, o.ld, o.nslab, o.rows) for o in outs])
        for i in range(n):
            res[i]["C_acc%d" % accumulate] = Cd[i].cpu()
    assert [o[1:] for o in outs_all[0]] == [o[1:] for o in outs_all[1]]                # (the plan does not depend on `accumulate`)
    wsf = ws_all[0].cpu().view(torch.float32)
    for i, (M, N, K) in enumerate(probs):
        p, stride, ld, nslab, rows = outs_all[0][i]
        off = None if not p else p - ws_all[0].data_ptr()
        res[i].update(out=(off, stride, ld, nslab, rows), p=p, ws_bytes=ws_bytes, C0=C0[i],
                      ref=As[i].double() @ (Bs[i].double() if layout[1] else Bs[i].double().t()))
        res[i]["partials"] = None
        if nslab >= 2 and off is not None and off % 4 == 0 and ld == N and 0 <= off and off + 4 * (nslab - 1) * stride + 4 * M * N <= ws_bytes:
            res[i]["partials"] = torch.stack([wsf[off // 4 + s * stride: off // 4 + s * stride + M * N].view(M, N) for s in range(nslab)])
    # the reduced product of the same descriptors and the same scratch size
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    Cd = [c.to(DEV).clone() for c in C0]
    call(L.set_gemm_group_f32, 0, Cd, ws)
    for i in range(n):
        res[i]["C_full"] = Cd[i].cpu()
    res[0]["keep"] = (ws_all[0], outs_all[0], Ad, Bd)                               # the chained case reads the partials in place
    return res


@pytest.mark.parametrize("layout,gi,mode", GEMM_PARAMS)
def test_gemm_group_slabs(layout, gi, mode):
    res = gemm_run(layout, gi, mode)
    regions = []
    first = next(i for i, q in enumerate(GROUPS[layout][gi]) if _can_split(*q))
    for i, r in enumerate(res):
        M, N, K = r["shape"]
        off, stride, ld, nslab, rows = r["out"]
        what = "gemm_group_slabs %s group %d %s problem %d (M=%d N=%d K=%d) nslab=%d" % (layout, gi, mode, i, M, N, K, nslab)
        print(what)
        assert nslab == 0 or nslab >= 2, what
        assert rows == M, what
        if not _can_split(M, N, K) or mode == "under_two":
            assert nslab == 0, what
        if mode == "three" and i == first:                            # (a later, smaller problem may fit more into what is left)
            assert nslab <= 3, what
        if nslab == 0:
            check([("C", r["C_acc0"], r["ref"], None)], ktol(K), what)
            check([("C accumulate", r["C_acc1"], r["ref"] + r["C0"].double(), None)], ktol(K), what)
        else:
            assert r["p"] % 16 == 0 and 0 <= off and off + 4 * nslab * stride <= r["ws_bytes"], what
            assert ld == N and stride % 4 == 0 and stride >= M * N, what
            regions.append((off, off + 4 * nslab * stride))
            assert torch.equal(r["C_acc0"], r["C0"]) and torch.equal(r["C_acc1"], r["C0"]), what     # the partials stay in ws
            part = r["partials"]
            assert part is not None and bool(torch.isfinite(part).all()), what
            check([("sum of the partials", part.double().sum(0), r["ref"], None)], ktol(K), what)
            e = Entry(part, M, nslab)
            assert torch.equal(SO.ordered_sum32(None, [e], M, N), r["C_full"]), (what, "set_gemm_group_f32 differs from the ordered sum")
        check([("set_gemm_group_f32", r["C_full"], r["ref"], None)], ktol(K), what)
    regions.sort()
    assert all(a[1] <= b[0] for a, b in zip(regions, regions[1:])), (regions, "regions of different problems overlap")


def test_gemm_group_slabs_cases_cover_the_split_depths():
    """the parametrisation above may not silently cover nothing: unsplit, clipped to three, and the planner's own deeper split"""
    seen = sorted({r["out"][3] for prm in GEMM_PARAMS for r in gemm_run(*prm)})
    print("nslab values produced:", seen)
    assert 0 in seen and 3 in seen and any(v >= 5 for v in seen), seen


def test_gemm_group_slabs_output_feeds_a_consumer_unchanged():
    """out[] of a set_gemm_group_slabs_f32 call goes as it is into set_lstm_gates_bwd_src_f32 (D = N = 64, M = 70)"""
    from show_edit_tell_amd import _lib
    res = gemm_run((0, 1), 1, "generous")
    ws, outs, _, _ = res[0]["keep"]
    r = res[1]
    M, D, K = r["shape"]
    p, stride, ld, nslab, rows = outs[1]
    assert nslab >= 2 and (M, D) == (70, 64)
    arr = (_lib.SlabSrc * 1)(_lib.SlabSrc(p, stride, ld, nslab, rows))
    R = Run("base_only", M, D)
    ent = [Entry(r["partials"], rows, nslab)]
    R.g32, R.g64 = SO.ordered_sum32(R.base, ent, M, D), SO.sum64(R.base, ent, M, D)
    R.g32_d = R.g32.to(DEV)
    _lstm_gates(cell_inputs(M, D), R, M, D, "lstm_gates fed by set_gemm_group_slabs_f32 (nslab %d)" % nslab, arr=arr, n=1)
    check([("gradient", R.g64, R.base.double() + r["ref"], None)], ktol(K), "the chained gradient")
