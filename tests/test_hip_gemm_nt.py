"""GPU: the grouped fp32 NT GEMM family of csrc/gemm_f32.hip against a high-precision reference, through its own entry point
(set_gemm_nt_group_f32, autograd_ops.gemm_nt_group), at the tile, slice, segment, task and gate edges of its design.

Exact pass.  A, W and bias hold integers from [-8, 8] stored as fp32.  Every product is an integer of at most 64, every partial
sum in any order an integer of at most K_total * 64 + 8 <= 18 440 < 2^24, so every intermediate of every path — whatever the
tile, the K permutation inside a k-tile, the slab order or the reduction — is exactly representable and the result must equal
the int64 numpy result BIT FOR BIT: no tolerance, no exempt element.  One dropped, duplicated or misplaced term fails.  (The
bound is asserted per problem from its actual K.)  Operands live inside wider tensors whose other columns are NaN (column-slice
views, as the decode step reads W_ih[:, 2D:3D]): a read outside the operand poisons the result.

Guards.  Every C is a view into a larger tensor filled with a NaN of a fixed bit pattern, with ldc > N and guard rows before and
after; the WHOLE tensor is compared with the expected image (sentinel outside [0,M) x [0,N) or outside the listed rows, the
reference bits inside), so a stray or missing store shows wherever it lands.

Rounding pass.  The integers above are exact in bf16 as well, so a path that lost fp32 precision would pass the exact pass;
normal floats against float64 numpy at the bound of the project's other GEMM test (test_gemm_general_layouts) catch that.

Row-tile classes: <= 16 rows gemv_nt_f32, <= 32 rows 32x128, <= 512 rows 64x64 (hand-written k-loop where every K slice lies in
one segment, the compiler-scheduled one otherwise), 128x64 by hint or above 512 rows by the tile model.  K slice ks of a problem
split `ksplit` ways over `kt` k-tiles is [ks * kt // ksplit, (ks + 1) * kt // ksplit)."""
import numpy as np
import pytest
import torch

import parity
from show_edit_tell_amd import _lib
from show_edit_tell_amd._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x7FC12345          # a quiet NaN with a payload: "nobody wrote here"
G = 8                      # guard rows on either side of C (and of A / the row list where indices run out of range)
TAG = {16: "gemv_nt_f32<16,64>", 32: "gemm_nt_f32<32,128>", 64: "gemm_nt_f32<64,64>", 128: "gemm_nt_f32<128,64>"}
TAG_ASM = "gemm_nt_f32_asm<64,64>"
# one shape per row-tile class: (rows, bm_hint, class)
CLASSES = {"gemv": (5, 0, 16), "bm32": (17, 0, 32), "bm64": (65, 0, 64), "bm128": (129, 128, 128)}


def _dev_view(x, rows_guard=0, strided=True):
    """x (rows, K) as a column-slice view of a wider NaN-filled device tensor (and inside NaN guard rows)"""
    rows, K = x.shape
    off, wide = (32, K + 64) if strided else (0, K)
    h = np.full((rows + 2 * rows_guard, wide), np.nan, np.float32)
    h[rows_guard:rows_guard + rows, off:off + K] = x
    t = torch.from_numpy(h).to(DEV)
    return t[rows_guard:rows_guard + rows, off:off + K]


def _straddles(Ks, ksplit):
    """some K slice crosses from one segment into the next (then the compiler-scheduled 64x64 k-loop is taken)"""
    kt = sum(Ks) // 32
    ks = min(max(ksplit, 1), kt)
    ends = np.cumsum([k // 32 for k in Ks])[:-1]
    return any(s * kt // ks < e < (s + 1) * kt // ks for s in range(ks) for e in ends)


class Prob:
    """one problem: integer operands on the device, the exact reference on the host"""

    def __init__(self, rng, M, N, Ks, bias=True, act=ACT_NONE, ksplit=1, strided=True, a_guard=0, shift=None):
        self.M, self.N, self.Ks, self.act, self.ksplit = M, N, tuple(Ks), act, ksplit
        ref = np.zeros((M, N), np.int64)
        self.segs = []
        ktot = sum(Ks)
        assert ktot % 32 == 0 and ktot <= 288 and ktot * 64 + 8 <= 18440 < 2 ** 24
        a_all, w_all = [], []
        for K in Ks:
            a, w = rng.integers(-8, 9, (M, K)), rng.integers(-8, 9, (N, K))
            ref += a @ w.T
            a_all.append(a); w_all.append(w)
        b = rng.integers(-8, 9, N) if bias else None
        if bias:
            ref += b[None, :]
        assert np.abs(ref).max() <= ktot * 64 + 8          # the reference stays in the exact range
        # tanh / sigmoid: A and bias scaled by 2^-shift (exact) so that the exact pre-activation lies in [-4, 4]
        self.shift = 0
        if act in (ACT_TANH, ACT_SIGMOID):
            self.shift = int(np.ceil(np.log2(max(1, np.abs(ref).max()) / 4.0))) if shift is None else shift
            self.shift = max(self.shift, 0)
        sc = 2.0 ** -self.shift
        for a, w in zip(a_all, w_all):
            self.segs.append((_dev_view((a * sc).astype(np.float32), a_guard, strided), _dev_view(w.astype(np.float32), 0, strided)))
        self.bias = None if b is None else torch.from_numpy((b * sc).astype(np.float32)).to(DEV)
        self.pre = ref.astype(np.float64) * sc             # exact in fp32 too
        if act == ACT_RELU:
            ref = np.maximum(ref, 0)
        self.exact = act in (ACT_NONE, ACT_RELU)
        if self.exact:
            self.ref = ref.astype(np.float32)
        else:
            assert np.abs(self.pre).max() <= 4.0
            self.ref = np.tanh(self.pre) if act == ACT_TANH else 1.0 / (1.0 + np.exp(-self.pre))

    @property
    def ktiles(self):
        return sum(self.Ks) // 32

    def straddles(self):
        return _straddles(self.Ks, self.ksplit)


class Canvas:
    """a (M + 2 G, ld) device tensor of sentinels that holds one or more C views, and the image it must hold afterwards"""

    def __init__(self, M, ld):
        self.M, self.ld = M, ld
        self.t = torch.full((M + 2 * G, ld), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
        self.want = np.full((M + 2 * G, ld), SENT, np.uint32)
        self.approx = []

    def view(self, col0, N):
        return self.t[G:G + self.M, col0:col0 + N]

    def expect(self, col0, p, rows=None):
        rows = np.arange(p.M) if rows is None else np.asarray(rows, dtype=np.int64)
        if p.exact:
            self.want[G + rows, col0:col0 + p.N] = p.ref.view(np.uint32)[rows]
        else:
            self.approx.append((col0, p, rows))

    def check(self, what):
        got = self.t.view(torch.int32).cpu().numpy().view(np.uint32)
        for col0, p, rows in self.approx:
            v = got[G + rows, col0:col0 + p.N].view(np.float32)
            assert not np.isnan(v).any(), (what, "NaN inside C")
            err = np.abs(v.astype(np.float64) - p.ref[rows]).max() if len(rows) else 0.0
            assert err <= parity.STATE_TOL, (what, "activation", err)
            self.want[G + rows, col0:col0 + p.N] = v.view(np.uint32)
        bad = np.argwhere(got != self.want)
        if bad.size:
            r, c = bad[0]
            raise AssertionError("%s: %d elements differ; first at row %d (of C: %d), col %d: got %r, want %r" % (
                what, len(bad), r, r - G, c, got[r, c:c + 1].view(np.float32)[0], self.want[r, c:c + 1].view(np.float32)[0]))


def _ld(N, vec):
    ld = (N + 8 + 3) // 4 * 4
    return ld if vec else ld + 1


def run(probs, what, adjacent=False, vec=True, rows=None, written=True, **kw):
    """one launch of `probs` into fresh canvases, checked against the expected image -> (splits, class, kernel tags, canvases).
    adjacent: the outputs are neighbouring column slices of ONE tensor.  rows: the rows a row list selects (None: all)."""
    from show_edit_tell_amd.autograd_ops import gemm_nt_group
    lib = _lib.load()
    canvases, descs, col = [], [], 4
    if adjacent:
        cv = Canvas(probs[0].M, _ld(sum(p.N for p in probs), vec))
    for p in probs:
        if not adjacent:
            cv, col = Canvas(p.M, _ld(p.N, vec)), 4
        descs.append(dict(segs=p.segs, C=cv.view(col, p.N), bias=p.bias, act=p.act, ksplit=p.ksplit))
        if written:
            cv.expect(col, p, rows)
        if cv not in canvases:
            canvases.append(cv)
        col += p.N
    torch.cuda.synchronize()
    lib.set_profile_enable(1)
    try:
        ks, cls = gemm_nt_group(descs, **kw)
        torch.cuda.synchronize()
        tags = sorted(e["tag"] for e in _lib.profile_report() if e["tag"].startswith(("gemm_nt", "gemv_nt")))
    finally:
        lib.set_profile_enable(0)
    for i, cv in enumerate(canvases):
        cv.check("%s [canvas %d]" % (what, i))
    return ks, cls, tags, canvases


def run_both_loops(probs, what, **kw):
    """run(); where the hand-written 64x64 k-loop ran, run again on the compiler-scheduled one: same bits, other kernel"""
    ks, cls, tags, cvs = run(probs, what, **kw)
    if tags == [TAG_ASM]:
        ks2, cls2, tags2, cvs2 = run(probs, what + " (compiler-scheduled loop)", no_asm=True, **kw)
        assert (ks2, cls2, tags2) == (ks, cls, [TAG[64]]), (what, ks2, cls2, tags2)
        for a, b in zip(cvs, cvs2):
            assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), what
    return ks, cls, tags


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


# ------------------------------------------------------------------------------------------------- rows x columns
ROWS = [(1, 0, 16), (5, 0, 16), (16, 0, 16), (17, 0, 32), (32, 0, 32), (33, 0, 64), (64, 0, 64), (65, 0, 64), (129, 0, 64),
        (100, 128, 128), (129, 128, 128), (513, 0, None)]


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 130, 196, 257])
@pytest.mark.parametrize("M,hint,cls", ROWS, ids=["M%d%s" % (m, "_hint128" if h else "") for m, h, _ in ROWS])
def test_exact_rows_cols(M, hint, cls, N):
    """every row-tile class at its row edges (one live row in the last tile: 1, 17, 33, 65, 129, 513) against column tiles with
    N % 64 in {1, 3, 63, 0} and 16-column gemv waves partly filled; bias fused, two k-tiles, unsplit.  N % 4 == 0 runs the
    16-byte epilogue (ldc % 4 == 0) and the scalar one (ldc % 4 == 1); the other N can only take the scalar one."""
    for vec in ((True, False) if N % 4 == 0 else (False,)):
        p = Prob(_rng(1, M, N, vec), M, N, (64,))
        ks, got_cls, tags = run_both_loops([p], "M=%d N=%d hint=%d vec=%d" % (M, N, hint, vec), vec=vec, bm_hint=hint)
        assert ks == [1]
        if cls is None:
            print("M = 513 (tile model, N = %d): row-tile class %d, kernel %s" % (N, got_cls, tags))
            assert got_cls in (64, 128)
        else:
            assert got_cls == cls, (M, N, got_cls)
        assert tags == [TAG_ASM if got_cls == 64 else TAG[got_cls]], tags


# ------------------------------------------------------------------------------------------------- k-tiles x splits
KT_KS = sorted({(kt, ks) for kt in (1, 2, 3, 4, 5, 7, 9) for ks in (1, 2, 3, kt, 8)})


@pytest.mark.parametrize("kt,ksplit", KT_KS, ids=["kt%d_ks%d" % x for x in KT_KS])
@pytest.mark.parametrize("cname", list(CLASSES))
def test_exact_ktiles_splits(cname, kt, ksplit):
    """slices of 1, 2, 3 and 4+ k-tiles, even and uneven (7 tiles over 3 slices, 9 over 8), on every class: the prologue
    branches and loop tails of both 64x64 k-loops, the 4-tile and 1-tile loops of gemv.  N = 132 writes slabs with 16-byte
    stores, N = 67 with scalar ones; split problems come back through the reduction with their bias."""
    M, hint, cls = CLASSES[cname]
    for N in (132, 67):
        p = Prob(_rng(2, M, N, kt, ksplit), M, N, (32 * kt,), ksplit=ksplit, strided=False)
        ks, got_cls, tags = run_both_loops([p], "%s kt=%d ksplit=%d N=%d" % (cname, kt, ksplit, N), bm_hint=hint)
        assert ks == [min(ksplit, kt)] and got_cls == cls
        assert tags == [TAG_ASM if cls == 64 else TAG[cls]], tags          # one segment: always eligible


@pytest.mark.parametrize("M,hint,N,Ks", [(5, 0, 257, (288,)), (65, 0, 196, (96, 96, 96)), (129, 128, 130, (224,))],
                         ids=["gemv", "bm64", "bm128"])
def test_exact_planner_split(M, hint, N, Ks):
    """ksplit = 0: whatever plan_ksplit chooses is served correctly"""
    p = Prob(_rng(3, M, N), M, N, Ks, ksplit=0)
    ks, cls, tags = run_both_loops([p], "planner M=%d N=%d" % (M, N), bm_hint=hint)
    print("planner: M = %d N = %d k-tiles = %d -> ksplit %d on class %d (%s)" % (M, N, p.ktiles, ks[0], cls, tags))
    assert 1 <= ks[0] <= min(8, p.ktiles)


# ------------------------------------------------------------------------------------------------- segments
SEGS = [((32, 64, 32), 1), ((32, 64, 32), 2), ((32, 64, 32), 3), ((32, 64, 32), 4), ((96, 32), 1), ((96, 32), 2), ((96, 32), 4),
        ((64, 64), 2), ((64, 64), 4), ((96, 96, 96), 2), ((96, 96, 96), 3), ((96, 96, 96), 9), ((32, 32, 32), 3), ((64, 96), 5)]


# the grid holds splits that end on the segment ends and splits that cross one, for two and for three segments
assert {(len(k), _straddles(k, s)) for k, s in SEGS} == {(2, False), (2, True), (3, False), (3, True)}


@pytest.mark.parametrize("Ks,ksplit", SEGS, ids=["K%s_ks%d" % ("+".join(map(str, k)), s) for k, s in SEGS])
@pytest.mark.parametrize("cname", list(CLASSES))
def test_exact_segments(cname, Ks, ksplit):
    """two and three (A, W) segments read in place through strided views, split so that slice boundaries coincide with
    segment ends (hand-written loop eligible) or a slice crosses one (seek inside the k-loop; compiler-scheduled loop)"""
    M, hint, cls = CLASSES[cname]
    p = Prob(_rng(4, M, sum(Ks), len(Ks), ksplit), M, 130, Ks, ksplit=ksplit)
    ks, got_cls, tags = run_both_loops([p], "%s K=%s ksplit=%d" % (cname, Ks, ksplit), bm_hint=hint)
    assert ks == [min(ksplit, p.ktiles)] and got_cls == cls
    want = TAG[cls] if cls != 64 or p.straddles() else TAG_ASM
    assert tags == [want], (tags, want)


# ------------------------------------------------------------------------------------------------- tasks
def _six(rng, M):
    return [Prob(rng, M, 192, (64,), ksplit=1),                         # M = 130: 3 row tiles x 3 column tiles, stride 8
            Prob(rng, M, 65, (32, 64, 32), ksplit=2, bias=False),
            Prob(rng, M, 64, (96, 32), ksplit=4),
            Prob(rng, M, 3, (32,), ksplit=1, act=ACT_RELU),
            Prob(rng, M, 257, (96, 96, 96), ksplit=3, act=ACT_RELU),
            Prob(rng, M, 130, (64, 64), ksplit=1, bias=False)]


@pytest.mark.parametrize("n", [2, 3, 6])
@pytest.mark.parametrize("M,hint,cls", [(5, 0, 16), (17, 0, 32), (130, 0, 64), (130, 128, 128)],
                         ids=["gemv", "bm32", "bm64_M130", "bm128_M130"])
def test_exact_tasks(M, hint, cls, n):
    """2, 3 and 6 problems of different N, segment counts and splits in one launch (tasks 2..6 are found through the preloaded
    first-workgroup table), split and unsplit mixed, outputs as separate tensors and as adjacent slices of one.  At M = 130
    the unsplit N = 192 problem has 3 row tiles of 3 workgroups each on a stride rounded up to 8: padding slots."""
    probs = _six(_rng(5, M, n, hint), M)[:n]
    for adjacent in (False, True):
        ks, got_cls, tags = run_both_loops(probs, "tasks n=%d M=%d hint=%d adjacent=%d" % (n, M, hint, adjacent),
                                           adjacent=adjacent, vec=not adjacent, bm_hint=hint)
        assert ks == [min(p.ksplit, p.ktiles) for p in probs] and got_cls == cls
        strad = any(p.straddles() for p in probs)
        assert tags == [TAG[cls] if cls != 64 or strad else TAG_ASM], tags


def test_exact_tasks_all_eligible():
    """six problems whose slices all lie inside one segment: the hand-written loop serves every task slot"""
    rng = _rng(6)
    probs = [Prob(rng, 130, N, Ks, ksplit=ks) for N, Ks, ks in
             [(192, (64,), 1), (65, (32, 64, 32), 4), (64, (96, 32), 4), (3, (32,), 1), (257, (96, 96, 96), 3), (130, (64, 64), 2)]]
    ks, cls, tags = run_both_loops(probs, "six eligible tasks")
    assert cls == 64 and tags == [TAG_ASM] and ks == [1, 4, 4, 1, 3, 2]


MIXED = [((16, 17), 32), ((32, 33), 64), ((5, 130), 64), ((512, 513), 128)]


@pytest.mark.parametrize("Ms,cls", MIXED, ids=["M%d+%d" % m for m, _ in MIXED])
def test_exact_mixed_row_classes(Ms, cls):
    """two problems whose row counts fall into different row-tile classes in ONE launch: the launch runs on the larger class
    (one kernel, one tag), and the problem of the smaller class is served exactly by tiles it only partly fills"""
    rng = _rng(14, *Ms)
    probs = [Prob(rng, M, 65, (64,), ksplit=1) for M in Ms]
    ks, got_cls, tags = run_both_loops(probs, "mixed classes M=%s" % (Ms,))
    assert ks == [1, 1] and got_cls == cls
    assert tags == [TAG_ASM if cls == 64 else TAG[cls]], tags


def test_mixed_row_classes_row_list_refused():
    """(5, 16) rows: both problems in the <= 16-row class, which takes no row list (as test_row_list_refusals: one problem)"""
    from show_edit_tell_amd.autograd_ops import gemm_nt_group
    rng = _rng(15)
    lst_d, _ = _row_list(rng, 16)
    count = torch.tensor([3], dtype=torch.int32, device=DEV)
    probs = [Prob(rng, M, 65, (64,)) for M in (5, 16)]
    cvs = [Canvas(p.M, _ld(65, False)) for p in probs]
    rc, _, _ = gemm_nt_group([dict(segs=p.segs, C=cv.view(4, 65), ksplit=1) for p, cv in zip(probs, cvs)], row_list=lst_d,
                             row_count=count, code=True)
    assert rc == 2                                     # SET_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for cv in cvs:
        cv.check("refused (5 and 16 rows with a row list)")


# ------------------------------------------------------------------------------------------------- epilogue
@pytest.mark.parametrize("ksplit", [1, 3])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID], ids=["none", "relu", "tanh", "sigmoid"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("cname", list(CLASSES))
def test_epilogue(cname, bias, act, ksplit):
    """bias on / off with each activation, fused (unsplit) and through the reduction (split).  None and ReLU are exact; for
    tanh and sigmoid the pre-activation is exact and O(1), so only tanhf / expf error remains: fp64 at parity.STATE_TOL."""
    M, hint, cls = CLASSES[cname]
    for N, vec in ((132, True), (67, False)):
        p = Prob(_rng(7, M, N, bias, act, ksplit), M, N, (128,), bias=bias, act=act, ksplit=ksplit)
        ks, got_cls, _ = run_both_loops([p], "%s bias=%d act=%d ksplit=%d N=%d" % (cname, bias, act, ksplit, N), vec=vec,
                                        bm_hint=hint)
        assert ks == [ksplit] and got_cls == cls


@pytest.mark.parametrize("cname", list(CLASSES))
def test_split_activation_refused_by_launcher(cname):
    """the launcher itself (partials kept, its own epilogue) refuses an activation on a split problem; nothing is written"""
    from show_edit_tell_amd.autograd_ops import gemm_nt_group
    M, hint, _ = CLASSES[cname]
    p = Prob(_rng(8, M), M, 64, (128,), bias=False, act=ACT_TANH, ksplit=2)
    cv = Canvas(M, _ld(64, True))
    rc, _, _ = gemm_nt_group([dict(segs=p.segs, C=cv.view(4, 64), act=p.act, ksplit=2)], bm_hint=hint, keep_slabs=True, code=True)
    assert rc == 1
    torch.cuda.synchronize()
    cv.check("refused launch")


# ------------------------------------------------------------------------------------------------- GATE = 1
@pytest.mark.parametrize("cname", list(CLASSES))
def test_loop_left_gate(cname):
    """alive = 1: the exact result.  alive = 0: not a byte of the poisoned C (unsplit) nor of the poisoned slabs (split,
    partials kept) changes.  With alive = 1 the kept partials add up to the exact result, slab by slab where documented."""
    from show_edit_tell_amd.autograd_ops import gemm_nt_group
    M, hint, cls = CLASSES[cname]
    one, zero = (torch.tensor([v], dtype=torch.int32, device=DEV) for v in (1, 0))
    probs = [Prob(_rng(9, M, 1), M, 132, (96, 32), ksplit=1), Prob(_rng(9, M, 2), M, 67, (64,), ksplit=1, act=ACT_RELU)]
    ks, got_cls, tags = run_both_loops(probs, cname + " alive=1", bm_hint=hint, alive=one)
    assert got_cls == cls and ks == [1, 1]
    run(probs, cname + " alive=0", written=False, bm_hint=hint, alive=zero)
    # split, partials kept in the workspace
    split = [Prob(_rng(9, M, 3), M, 132, (96, 32), bias=False, ksplit=4), Prob(_rng(9, M, 4), M, 67, (96,), bias=False, ksplit=2)]
    nbytes = [(4 * M * 132 * 4 + 255) // 256 * 256, (2 * M * 67 * 4 + 255) // 256 * 256]
    for gate, alive in ((zero, 0), (one, 1)):
        ws = torch.full((sum(nbytes) // 4 + 64,), SENT, dtype=torch.int32, device=DEV)
        cvs = [Canvas(M, _ld(p.N, True)) for p in split]
        descs = [dict(segs=p.segs, C=cv.view(4, p.N), ksplit=p.ksplit) for p, cv in zip(split, cvs)]
        ks, _ = gemm_nt_group(descs, bm_hint=hint, alive=gate, keep_slabs=True, ws=ws.view(torch.uint8))
        torch.cuda.synchronize()
        assert ks == [4, 2]
        for cv in cvs:
            cv.check("kept partials: C is not written")
        h = ws.cpu().numpy().view(np.uint32)
        if not alive:
            assert (h == SENT).all(), "alive = 0 wrote %d words of the slabs" % int((h != SENT).sum())
            continue
        off = 0
        for p, nb in zip(split, nbytes):
            slabs = h[off // 4: off // 4 + p.ksplit * M * p.N].view(np.float32).reshape(p.ksplit, M, p.N)
            assert not np.isnan(slabs).any()
            assert np.array_equal(slabs.astype(np.int64).sum(0), p.pre.astype(np.int64)), cname
            assert (h[off // 4 + p.ksplit * M * p.N: (off + nb) // 4] == SENT).all()
            off += nb
        assert (h[off // 4:] == SENT).all()


# ------------------------------------------------------------------------------------------------- GATE = 2
LIST_CLASSES = {"bm32": (32, 0, 32, False), "bm64_asm": (150, 0, 64, False), "bm64_cxx": (150, 0, 64, True),
                "bm128": (300, 128, 128, False)}


def _row_list(rng, M, bad=False):
    """a shuffled list of all M rows inside a larger int tensor (zeros around it) -> (device view, host list)"""
    lst = rng.permutation(M).astype(np.int32)
    if bad:
        lst[[1, M // 2]] = (-3, M + 5)
    h = np.zeros(M + 2 * 16, np.int32)
    h[16:16 + M] = lst
    return torch.from_numpy(h).to(DEV)[16:16 + M], lst


def _list_probs(rng, M, cxx):
    # (the second problem's first slice crosses a segment end where the compiler-scheduled loop is wanted)
    return [Prob(rng, M, 132, (64,), act=ACT_RELU, a_guard=G), Prob(rng, M, 67, (32, 64) if cxx else (96,), a_guard=G)]


@pytest.mark.parametrize("cname", list(LIST_CLASSES))
def test_row_list(cname):
    """the compacted row list on the three LDS-staged classes (64x64 on both k-loops): two problems share one shuffled,
    unsorted list; only the listed rows are written — with the exact values of those rows — for counts 0, 1, BM - 1, BM,
    BM + 1 and M; a count above M acts as M, a negative one writes nothing."""
    M, hint, bm, cxx = LIST_CLASSES[cname]
    rng = _rng(10, M, hint, cxx)
    probs = _list_probs(rng, M, cxx)
    lst_d, lst = _row_list(rng, M)
    for cnt in sorted({0, 1, bm - 1, bm, bm + 1, M, M + 7, -2}):
        eff = min(max(cnt, 0), M)
        count = torch.tensor([cnt], dtype=torch.int32, device=DEV)
        ks, cls, tags = run_both_loops(probs, "%s count=%d" % (cname, cnt), rows=np.sort(lst[:eff]), bm_hint=hint,
                                       row_list=lst_d, row_count=count)
        assert cls == bm and ks == [1, 1]
        assert tags == [TAG[bm] if bm != 64 or cxx else TAG_ASM], tags


@pytest.mark.parametrize("cname", list(LIST_CLASSES))
def test_row_list_indices_out_of_range(cname):
    """list entries -3 and M + 5 act as rows 0 and M - 1.  A, C and the list lie inside larger tensors with NaN (A, C) or
    zero (list) guards wider than the excursion: a missing clamp shows as NaN in C or as a touched guard row, and stays
    inside the allocations."""
    M, hint, bm, cxx = LIST_CLASSES[cname]
    rng = _rng(11, M, hint, cxx)
    probs = _list_probs(rng, M, cxx)
    lst_d, lst = _row_list(rng, M, bad=True)
    cnt = M // 2 + 1                                   # both bad entries are inside the count
    rows = np.unique(np.clip(lst[:cnt], 0, M - 1))
    assert 0 in rows and M - 1 in rows
    count = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    ks, cls, _ = run_both_loops(probs, cname + " bad indices", rows=rows, bm_hint=hint, row_list=lst_d, row_count=count)
    assert cls == bm


def test_row_list_refusals():
    from show_edit_tell_amd.autograd_ops import gemm_nt_group
    rng = _rng(12)
    lst_d, _ = _row_list(rng, 65)
    count = torch.tensor([3], dtype=torch.int32, device=DEV)
    p = Prob(rng, 65, 64, (96,), ksplit=2)
    cv = Canvas(65, _ld(64, True))
    rc, _, _ = gemm_nt_group([dict(segs=p.segs, C=cv.view(4, 64), ksplit=2)], row_list=lst_d, row_count=count, code=True)
    assert rc == 1                                     # SET_ERR_ARG: a row list takes unsplit problems only
    q = Prob(rng, 16, 64, (96,))
    cq = Canvas(16, _ld(64, True))
    rc, _, _ = gemm_nt_group([dict(segs=q.segs, C=cq.view(4, 64), ksplit=1)], row_list=lst_d, row_count=count, code=True)
    assert rc == 2                                     # SET_ERR_UNSUPPORTED: the <= 16-row class has no row tiles to skip
    torch.cuda.synchronize()
    cv.check("refused (split)")
    cq.check("refused (16-row class)")


# ------------------------------------------------------------------------------------------------- rounding pass
ROUND = [(5, 0, 257, 0), (17, 0, 130, 3), (65, 0, 196, 1), (65, 0, 63, 2), (129, 128, 64, 9), (513, 0, 257, 0)]


@pytest.mark.parametrize("M,hint,N,ksplit", ROUND, ids=["M%d_N%d_ks%d" % (m, n, k) for m, _, n, k in ROUND])
def test_rounding(M, hint, N, ksplit):
    """normal floats, K = 288 in three segments, against float64 numpy at the bound of test_gemm_general_layouts
    (2e-6 sqrt(K) 4 max(1, |ref|max)): fp32 products and sums on every path.  A second run gives the same bits."""
    from show_edit_tell_amd.autograd_ops import gemm_nt_group
    rng = np.random.default_rng([13, M, N, ksplit])
    Ks = (96, 96, 96)
    ref = np.zeros((M, N))
    segs = []
    for K in Ks:
        a, w = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
        ref += a.astype(np.float64) @ w.astype(np.float64).T
        segs.append((_dev_view(a), _dev_view(w)))
    b = rng.standard_normal(N).astype(np.float32)
    ref += b
    tol = 2e-6 * np.sqrt(sum(Ks)) * 4 * max(1.0, np.abs(ref).max())
    outs = []
    for _ in range(2):
        cv = Canvas(M, _ld(N, N % 4 == 0))
        ks, cls = gemm_nt_group([dict(segs=segs, C=cv.view(4, N), bias=torch.from_numpy(b).to(DEV), ksplit=ksplit)], bm_hint=hint)
        torch.cuda.synchronize()
        got = cv.t.cpu().numpy()
        inside = got[G:G + M, 4:4 + N]
        assert not np.isnan(inside).any()
        err = np.abs(inside - ref).max()
        print("rounding M=%d N=%d ksplit=%s class %d: max err %.3e (bound %.3e)" % (M, N, ks, cls, err, tol))
        assert err <= tol, (M, N, err, tol)
        got.view(np.uint32)[G:G + M, 4:4 + N] = SENT
        assert (got.view(np.uint32) == SENT).all(), "stores outside C"
        outs.append(cv.t.view(torch.int32).clone())
    assert torch.equal(outs[0], outs[1])
