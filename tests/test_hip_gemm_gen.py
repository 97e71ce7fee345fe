"""GPU: the general-layout fp32 GEMM of csrc/gemm_gen.hip (gemm_gen_f32, slab_reduce_k, the launcher gemm_gen_group) through
its own entry points — set_gemm_f32, set_gemm_group_f32, set_gemm_group_slabs_f32 — against the exact integer product and
float64, at the tile, slice, alignment, task and load-path edges of its design.  Cases, buffers and reference:
tests/gemm_gen_cases.py (checked without a device by tests/test_gemm_gen_cases_cpu.py).

Exact pass: integer operands inside NaN buffers, every C a view inside a canvas of sentinels, the WHOLE canvas and the WHOLE
split-K scratch compared bit for bit with the expected image: no tolerance, no exempt element.  set_gemm_group_slabs_f32 is the
only window on the split decision: every split assertion goes through the nslab it reports, and every kept partial must be
exactly the product over its k slice [32 floor(s kt / nslab), min(K, 32 floor((s + 1) kt / nslab))).

Rounding pass: integers are exact in bf16 as well, so normal floats against float64 at the bound of the project's other
general-GEMM tests (ktol of tests/test_hip_backward_ops.py) catch a path that lost fp32 precision.

Routes.  SET_EXP_GEN_KPER (k-tiles per slice) is read by the launcher on every call and forces the depth in-process.
SET_GEMM_GEN_HWB (buffer loads / pointer loads), SET_GEMM_GEN_PLAN and SET_GEMM_GEN_BM64_UPTO (row-tile class) are read once
per process: test_forced_routes re-runs the exact and rounding tests of this file in a fresh child per setting.  This module
reads the same variables only to know what it asked for.  The row-tile class is not observable: it is known where the
launcher has no choice (M <= BM64_UPTO: 64 rows; above, with a forced depth or without the cost model: 128 rows)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_gen_cases as GC
import slab_src_oracle as SO
from gemm_gen_cases import G, LAYOUT_NAME, SENT
from show_edit_tell_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _env_int(name, default):
    try:
        return int(os.environ.get(name, default))
    except ValueError:
        return default


HWB = _env_int("SET_GEMM_GEN_HWB", 1) != 0
PLAN = _env_int("SET_GEMM_GEN_PLAN", 1) != 0
BM64_UPTO = _env_int("SET_GEMM_GEN_BM64_UPTO", 512)
SEEN = dict(nslab=set(), layouts=set(), classes=set(), paths=set(), scalar=0, vec=0, launches=0, tests=set())
GRID_TESTS = {"rows_cols", "k_split", "scratch", "groups", "rounding"}


def _note(name, probs, cmodes, kper, nslabs=()):
    cls = {64 if p.M <= BM64_UPTO else 128 for p in probs}
    assert len(cls) == 1
    c = cls.pop()
    SEEN["classes"].add("model" if c == 128 and kper is None and PLAN else c)     # (the cost model may go back to 64 rows)
    SEEN["layouts"].add(LAYOUT_NAME[probs[0].layout])
    SEEN["paths"].add("buffer" if HWB else "pointer")
    SEEN["nslab"].update(int(n) for n in nslabs)
    for p, m in zip(probs, cmodes):
        SEEN["vec" if GC.takes_vec(p.N, m) else "scalar"] += 1
    SEEN["launches"] += 1
    SEEN["tests"].add(name)


def _set_kper(monkeypatch, kper):
    if kper is None:
        monkeypatch.delenv("SET_EXP_GEN_KPER", raising=False)
    else:
        monkeypatch.setenv("SET_EXP_GEN_KPER", str(kper))


def _ptr(op):
    """device address of an operand inside its (cached) NaN-surrounded device buffer"""
    if getattr(op, "dev", None) is None:
        op.dev = torch.from_numpy(op.buf).to(DEV)
    return op.dev.data_ptr() + 4 * op.offset


def _canvas(p, cmode, acc):
    return torch.from_numpy(p.canvas0(cmode, acc).view(np.int32)).to(DEV)


def _same(t, want, what):
    got = t.cpu().numpy().view(want.dtype).reshape(want.shape)
    bad = np.argwhere(got != want)
    if bad.size:
        i = tuple(int(x) for x in bad[0])
        where = "canvas (row, column) %s, C begins at row %d" % (i, G) if len(i) == 2 else "byte %d" % i[0]
        raise AssertionError("%s: %d elements differ; first at %s: got %#x, want %#x" % (what, len(bad), where, int(got[i]), int(want[i])))


def _descs(probs, canvases, cmodes, accs):
    arr = (_lib.GemmDesc * len(probs))()
    for i, p in enumerate(probs):
        off, ldc = p.c_offset(cmodes[i])
        arr[i] = _lib.GemmDesc(_ptr(p.A), p.A.ld, _ptr(p.B), p.B.ld, canvases[i].data_ptr() + 4 * off, ldc, p.M, p.N, p.K, accs[i])
    return arr


def _scratch(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)             # (all-ones words are NaN)


def run_group(name, probs, cmodes, accs, kper, what, ws_bytes=None, expect=None):
    """set_gemm_group_slabs_f32, then set_gemm_group_f32, on the same descriptors and the same scratch size -> nslab per task.
    Checks: the reported regions, every byte of the scratch, every canvas (untouched where the partials are kept)."""
    lib, st = _lib.load(), _lib.stream_of(DEV)
    n, layout = len(probs), probs[0].layout
    ws_bytes = GC.generous_scratch(probs) if ws_bytes is None else ws_bytes
    ws, cvs = _scratch(ws_bytes), [_canvas(p, m, a) for p, m, a in zip(probs, cmodes, accs)]
    outs = (_lib.SlabSrc * n)()
    _lib.check(lib.set_gemm_group_slabs_f32(_descs(probs, cvs, cmodes, accs), n, layout[0], layout[1], ws.data_ptr(), ws_bytes,
                                            outs, st), what)
    torch.cuda.synchronize()
    want = np.full(ws_bytes, 0xFF, np.uint8)
    nslabs, regions = [], []
    for i, (p, o) in enumerate(zip(probs, outs)):
        w = "%s task %d (M=%d N=%d K=%d %s acc=%d) nslab=%d" % (what, i, p.M, p.N, p.K, cmodes[i], accs[i], o.nslab)
        assert o.nslab == 0 or 2 <= o.nslab <= GC.MAX_SLABS, w
        assert o.rows == p.M, w
        if not GC.can_split(p.N, p.K, cmodes[i]):
            assert o.nslab == 0, w                            # fewer than 8 k-tiles (K < 225), or no 16-byte stores
        if expect is not None:
            assert o.nslab == expect[i], (w, expect[i])
        nslabs.append(o.nslab)
        if o.nslab == 0:
            assert not o.p, w
            _same(cvs[i], p.image(cmodes[i], accs[i]), w + ": unsplit, lands in C")
            continue
        off, stride = o.p - ws.data_ptr(), o.slab_stride
        assert o.p % 16 == 0 and o.ld == p.N and 4 * stride == GC.slab_bytes(p.M, p.N), w
        assert 0 <= off and off + 4 * o.nslab * stride <= ws_bytes, w
        regions.append((off, off + 4 * o.nslab * stride))
        _same(cvs[i], p.canvas0(cmodes[i], accs[i]), w + ": the partials stay in the scratch, C is not written")
        for s in range(o.nslab):
            b = off + 4 * s * stride
            want[b:b + 4 * p.M * p.N] = p.partial(o.nslab, s).astype(np.float32).reshape(-1).view(np.uint8)
    regions.sort()
    assert all(a[1] <= b[0] for a, b in zip(regions, regions[1:])), (what, regions, "regions of different problems overlap")
    _same(ws, want, what + " " + str(nslabs) + ": scratch (a partial is not the product over its k slice, or a byte outside the partials changed)")
    # the reduced product
    ws, cvs = _scratch(ws_bytes), [_canvas(p, m, a) for p, m, a in zip(probs, cmodes, accs)]
    _lib.check(lib.set_gemm_group_f32(_descs(probs, cvs, cmodes, accs), n, layout[0], layout[1], ws.data_ptr(), ws_bytes, st), what)
    torch.cuda.synchronize()
    for i, p in enumerate(probs):
        _same(cvs[i], p.image(cmodes[i], accs[i]), "%s task %d (M=%d N=%d K=%d %s acc=%d nslab=%d): set_gemm_group_f32" % (
            what, i, p.M, p.N, p.K, cmodes[i], accs[i], nslabs[i]))
    _note(name, probs, cmodes, kper, nslabs)
    return nslabs


# --------------------------------------------------------------------------------------------------------------------- rows x columns
@pytest.mark.parametrize("M", GC.MS + GC.M_EXTRA)
@pytest.mark.parametrize("layout", GC.LAYOUTS, ids=[LAYOUT_NAME[l] for l in GC.LAYOUTS])
def test_exact_rows_cols(layout, M):
    """set_gemm_f32: every row edge (one live row in the last tile of either class: 65, 129, 513, 577; ragged M under a k-minor
    A: 5, 63, 65, ...) against column tiles with N % 64 in {1, 3, 4, 60, 0} and the clamped last float4 of a k-minor B, two
    k-tiles with a ragged second one; aligned C (16-byte epilogue where N % 4 == 0), C at an odd float offset and ldc % 4 != 0
    (scalar epilogue); accumulate 0 and 1."""
    lib, st = _lib.load(), _lib.stream_of(DEV)
    ws = _scratch(1 << 16)
    ran = 0
    for N in GC.NS:
        if not GC.allowed(layout, M, N):
            continue
        p = GC.Problem(M, N, GC.K_ROWS_COLS, layout, (1,))
        for cmode in GC.C_MODES:
            for acc in (0, 1):
                cv = _canvas(p, cmode, acc)
                off, ldc = p.c_offset(cmode)
                _lib.check(lib.set_gemm_f32(_ptr(p.A), p.A.ld, layout[0], _ptr(p.B), p.B.ld, layout[1], cv.data_ptr() + 4 * off, ldc,
                                            M, N, p.K, acc, ws.data_ptr(), ws.numel(), st), "set_gemm_f32")
                torch.cuda.synchronize()
                _same(cv, p.image(cmode, acc), "%s M=%d N=%d K=%d %s acc=%d" % (LAYOUT_NAME[layout], M, N, p.K, cmode, acc))
                _note("rows_cols", [p], [cmode], None)
                ran += 1
    if not ran:
        assert layout[0] and M < 4                             # (the ABI leaves nothing to run: tests/test_gemm_gen_cases_cpu.py)
    assert bool((ws == 0xFF).all()), "two k-tiles are never split: the scratch is not touched"


# --------------------------------------------------------------------------------------------------------------------- K x split depth
@pytest.mark.parametrize("K", GC.KS)
@pytest.mark.parametrize("layout", GC.LAYOUTS, ids=[LAYOUT_NAME[l] for l in GC.LAYOUTS])
def test_exact_k_split(layout, K, monkeypatch):
    """every contraction length — one k-tile, ragged ones (K % 32 != 0; K % 4 != 0 with the zero padding of k-major operands),
    7 k-tiles (never split), 8 and 9 (the first that are), 65 and 257 (the cap of 64 slices, uneven) — under the planner's own
    depth and under 4, 5 and 1000 k-tiles per slice, on 1 x 2, 2 x 3 and 3 x 1 tiles and on 513 rows (the 128-row class under
    a forced depth); the partials, the reduction with and without accumulate, and the outputs that cannot split (scalar
    epilogue: nslab == 0)."""
    for M, N, cmodes in GC.K_SHAPES:
        if not GC.allowed(layout, M, N):
            continue
        p = GC.Problem(M, N, K, layout, (2,))
        for kper in GC.KPERS:
            _set_kper(monkeypatch, kper)
            for cmode in cmodes:
                for acc in (0, 1):
                    expect = None if kper is None else [GC.expected_nslab(K, N, cmode, kper)]
                    run_group("k_split", [p], [cmode], [acc], kper, "%s kper=%s" % (LAYOUT_NAME[layout], kper), expect=expect)


# --------------------------------------------------------------------------------------------------------------------- scratch size
@pytest.mark.parametrize("mode", ["three", "under_two"])
@pytest.mark.parametrize("layout", [(1, 1), (1, 0)], ids=["tn", "tt"])
def test_exact_scratch_clips_the_split(layout, mode, monkeypatch):
    """the two k-minor-A layouts (tests/test_hip_slab_src.py has the other two): a scratch of exactly three slabs of the first
    splittable problem clips it to three and leaves nothing for the later ones; one of less than two slabs of the smallest
    sends everything to C"""
    spec = [(64, 68, 2080), (5, 64, 128), (33, 64, 512)]
    probs = [GC.Problem(M, N, K, layout, (5, i)) for i, (M, N, K) in enumerate(spec)]
    ws_bytes = 3 * GC.slab_bytes(64, 68) if mode == "three" else 2 * min(GC.slab_bytes(M, N) for M, N, _ in spec) - 256
    for kper in (None, 4):
        _set_kper(monkeypatch, kper)
        for acc in (0, 1):
            expect = [0, 0, 0] if mode == "under_two" else ([3, 0, 0] if kper else None)
            ns = run_group("scratch", probs, ["aligned"] * 3, [acc] * 3, kper, "%s %s kper=%s" % (LAYOUT_NAME[layout], mode, kper),
                           ws_bytes=ws_bytes, expect=expect)
            assert ns[0] <= 3 and ns[1] == 0


# --------------------------------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("n", GC.GROUP_SIZES + ("shared_a",))
@pytest.mark.parametrize("pool", list(GC.POOLS))
@pytest.mark.parametrize("layout", GC.LAYOUTS, ids=[LAYOUT_NAME[l] for l in GC.LAYOUTS])
def test_exact_groups(layout, pool, n, monkeypatch):
    """2, 3 and 6 tasks of different (M, N, K) in one launch and one grouped reduction (red_begin per task): a task that cannot
    split between tasks that do, accumulating tasks beside plain ones, three tasks sharing one A; row pools of one class each:
    <= 64 rows, 65..200 rows (several row tiles with overhang; the 128-row class when it is forced above 64 rows), 513 / 577
    rows (the 128-row class)."""
    shared = n == "shared_a"
    spec = GC.shared_a_spec(pool) if shared else GC.group_spec(layout, pool, n)
    probs = GC.make_group(layout, spec, (6,), share_a=shared)
    accs = [s[3] for s in spec]
    for kper in (None, 4):
        _set_kper(monkeypatch, kper)
        expect = None if kper is None else [GC.expected_nslab(K, N, "aligned", kper) for _, N, K, _ in spec]
        ns = run_group("groups", probs, ["aligned"] * len(probs), accs, kper,
                       "%s %s group of %s kper=%s" % (LAYOUT_NAME[layout], pool, n, kper), expect=expect)
        if kper and not shared:
            assert ns[0] >= 2 and ns[1] == 0 and (len(ns) < 3 or ns[2] >= 2)


def test_exact_mixed_row_classes_refused():
    """a group whose row counts fall on both sides of the 64-row class's limit (512 rows; 64 when forced) is SET_ERR_ARG;
    nothing is written"""
    lib, st = _lib.load(), _lib.stream_of(DEV)
    for layout in GC.LAYOUTS:
        for Ms in ((BM64_UPTO, BM64_UPTO + 1), (BM64_UPTO + 1, 4)):
            probs = [GC.Problem(M, 64, 32, layout, (7, i)) for i, M in enumerate(Ms)]
            cvs, ws = [_canvas(p, "aligned", 0) for p in probs], _scratch(4096)
            d = _descs(probs, cvs, ["aligned"] * 2, [0, 0])
            outs = (_lib.SlabSrc * 2)()
            assert lib.set_gemm_group_f32(d, 2, layout[0], layout[1], ws.data_ptr(), 4096, st) == GC.ARG
            assert lib.set_gemm_group_slabs_f32(d, 2, layout[0], layout[1], ws.data_ptr(), 4096, outs, st) == GC.ARG
            torch.cuda.synchronize()
            for p, cv in zip(probs, cvs):
                _same(cv, p.canvas0("aligned", 0), "refused group")


# --------------------------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("kper", GC.ROUND_KPERS, ids=["unsplit", "split"])
@pytest.mark.parametrize("M,N,K", GC.ROUND_SHAPES, ids=["bm64", "bm128"])
@pytest.mark.parametrize("layout", GC.LAYOUTS, ids=[LAYOUT_NAME[l] for l in GC.LAYOUTS])
def test_rounding(layout, M, N, K, kper, monkeypatch):
    """normal floats against float64 numpy at 2e-6 sqrt(K) 4 max(1, max|ref|) — ktol of tests/test_hip_backward_ops.py, the
    bound of test_gemm_general_layouts — per layout x row class x {unsplit, split 8 ways}; two calls give the same bits; the
    reduced C is slab_src_oracle.ordered_sum32 of the kept partials (slab 0 first, starting from +0)."""
    lib, st = _lib.load(), _lib.stream_of(DEV)
    _set_kper(monkeypatch, kper)
    p = GC.FloatProblem(M, N, K, layout, (8,))
    col0, ldc = GC.c_geometry(N, "aligned")
    ws_bytes = GC.generous_scratch([p])
    outs = []

    def call(fn, *extra):
        cv = torch.full((M + 2 * G, ldc), SENT, dtype=torch.int32, device=DEV)
        ws = _scratch(ws_bytes)
        d = (_lib.GemmDesc * 1)(_lib.GemmDesc(_ptr(p.A), p.A.ld, _ptr(p.B), p.B.ld, cv.data_ptr() + 4 * (G * ldc + col0), ldc, M, N, K, 0))
        _lib.check(fn(d, 1, layout[0], layout[1], ws.data_ptr(), ws_bytes, *extra, st), fn.__name__)
        torch.cuda.synchronize()
        return cv, ws

    for _ in range(2):
        cv, _ws = call(lib.set_gemm_group_f32)
        got = cv.cpu().numpy().view(np.uint32)
        inside = got[G:G + M, col0:col0 + N].view(np.float32).copy()
        assert not np.isnan(inside).any()
        err = np.abs(inside - p.ref).max()
        print("rounding %s M=%d N=%d K=%d kper=%d: max err %.3e (bound %.3e)" % (LAYOUT_NAME[layout], M, N, K, kper, err, p.tol))
        assert err <= p.tol, (err, p.tol)
        got[G:G + M, col0:col0 + N] = SENT
        assert (got == SENT).all(), "stores outside C"
        outs.append(inside)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "two identical calls differ"
    so = (_lib.SlabSrc * 1)()
    cv, ws = call(lib.set_gemm_group_slabs_f32, so)
    nslab = so[0].nslab
    assert nslab == GC.expected_nslab(K, N, "aligned", kper)
    if nslab:
        assert bool((cv == SENT).all())
        off, stride = (so[0].p - ws.data_ptr()) // 4, so[0].slab_stride
        wsf = ws.cpu().view(torch.float32)
        part = torch.stack([wsf[off + s * stride: off + s * stride + M * N].view(M, N) for s in range(nslab)])
        assert bool(torch.isfinite(part).all())
        assert torch.equal(SO.ordered_sum32(None, [SO.Entry(part, M, nslab)], M, N), torch.from_numpy(outs[0])), \
            "set_gemm_group_f32 differs from the ordered sum of its partials"
    _note("rounding", [p], ["aligned"], kper, [nslab])


# --------------------------------------------------------------------------------------------------------------------- summary
def test_exact_route_summary():
    """what the tests above ran in this process, as one line (test_forced_routes reads it from its children); where the whole
    grid ran, it may not have silently covered nothing"""
    s = dict(SEEN, nslab=sorted(SEEN["nslab"]), layouts=sorted(SEEN["layouts"]), classes=sorted(map(str, SEEN["classes"])),
             paths=sorted(SEEN["paths"]), tests=sorted(SEEN["tests"]), hwb=int(HWB), plan=int(PLAN), bm64_upto=BM64_UPTO)
    print("\nGEMM_GEN_ROUTES " + json.dumps(s))
    if not GRID_TESTS <= SEEN["tests"]:
        return                                                 # (a selection of tests: nothing to conclude)
    assert s["layouts"] == sorted(LAYOUT_NAME.values())
    assert 0 in s["nslab"] and 64 in s["nslab"] and any(2 <= v < 64 for v in s["nslab"]), s["nslab"]
    assert s["scalar"] > 0 and s["vec"] > 0
    assert {"64", "128"} <= set(s["classes"]), s["classes"]
    assert s["paths"] == ["buffer" if HWB else "pointer"]


# --------------------------------------------------------------------------------------------------------------------- forced routes
FORCED = {"pointer": {"SET_GEMM_GEN_HWB": "0"},
          "bm128": {"SET_GEMM_GEN_PLAN": "0", "SET_GEMM_GEN_BM64_UPTO": "64"},
          "pointer_bm128": {"SET_GEMM_GEN_HWB": "0", "SET_GEMM_GEN_PLAN": "0", "SET_GEMM_GEN_BM64_UPTO": "64"}}


@pytest.mark.parametrize("setting", list(FORCED))
def test_forced_routes(setting):
    """the exact and rounding tests of this file on the pointer-load kernels, on the 128 x 64 class for every M > 64 (M = 65,
    129, 130 and 200 then overhang it) and on both: the switches are read once per process, hence a fresh child each"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **FORCED[setting])
    env.pop("SET_EXP_GEN_KPER", None)
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(root, "tests", "test_hip_gemm_gen.py"), "-k", "test_exact or test_rounding"]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout
    line = [l for l in out.stdout.splitlines() if l.startswith("GEMM_GEN_ROUTES ")]
    assert len(line) == 1, out.stdout[-2000:]
    s = json.loads(line[0].split(" ", 1)[1])
    print(setting, line[0])
    assert GRID_TESTS <= set(s["tests"])
    assert 0 in s["nslab"] and 64 in s["nslab"] and any(2 <= v < 64 for v in s["nslab"]), s["nslab"]
    assert s["paths"] == (["pointer"] if "SET_GEMM_GEN_HWB" in FORCED[setting] else ["buffer"])
    assert s["bm64_upto"] == int(FORCED[setting].get("SET_GEMM_GEN_BM64_UPTO", 512))
    assert {"64", "128"} <= set(s["classes"]) and s["scalar"] > 0 and len(s["layouts"]) == 4
    if "SET_GEMM_GEN_PLAN" in FORCED[setting]:
        assert "model" not in s["classes"]                     # every launch ran on a class the test knows


# --------------------------------------------------------------------------------------------------------------------- 2^31
def test_31_bit_switch():
    """layout (1, 1), M = N = 64, K = 520 (17 k-tiles): A is a column-slice view of a (520, lda) NaN tensor whose furthest load
    offset 4 ((17 32 + 64) lda + 64) lies just below 2^31 - 1 (buffer loads) and just above (the launcher's switch to pointer
    loads).  Which path ran cannot be seen; both must be exact, with nothing written outside C."""
    lib, st = _lib.load(), _lib.stream_of(DEV)
    M = N = 64
    K = 520
    kt = GC.ktiles(K)
    far = lambda lda: 4 * ((kt * 32 + 64) * lda + GC.up4(M))
    ldas = (883008, 883012)
    assert far(ldas[0]) < 2 ** 31 - 1 <= far(ldas[1]) and far(ldas[1]) - far(ldas[0]) == 4 * 4 * (kt * 32 + 64)
    assert 4 * ((K - 1) * ldas[1] + M) < 2 ** 31 - 1           # (the operand itself stays addressable with 31 bits)
    p = GC.Problem(M, N, K, (1, 1), (9,))
    flat = torch.full((K * ldas[1] + 64,), float("nan"), dtype=torch.float32, device=DEV)       # about 1.9 GB
    vals = torch.from_numpy(np.ascontiguousarray(p.a.T.astype(np.float32))).to(DEV)             # (K, M)
    try:
        for lda in ldas:
            for acc in (0, 1):
                view = flat.as_strided((K, M), (lda, 1), 32)
                view.copy_(vals)
                cv, ws = _canvas(p, "aligned", acc), _scratch(GC.generous_scratch([p]))
                off, ldc = p.c_offset("aligned")
                _lib.check(lib.set_gemm_f32(flat.data_ptr() + 4 * 32, lda, 1, _ptr(p.B), p.B.ld, 1, cv.data_ptr() + 4 * off, ldc,
                                            M, N, K, acc, ws.data_ptr(), ws.numel(), st), "set_gemm_f32")
                torch.cuda.synchronize()
                _same(cv, p.image("aligned", acc), "lda=%d (furthest offset %d, 2^31 - 1 = %d) acc=%d" % (lda, far(lda), 2 ** 31 - 1, acc))
                view.fill_(float("nan"))
    finally:
        del flat
        torch.cuda.empty_cache()
