"""No device: the case tables and the host reference of tests/gemm_gen_cases.py judged against themselves, the K-slice
formula of csrc/gemm_gen.hip against a brute-force partition, and the host refusals of gemm_gen_group through the raw ABI
(host memory stands in for the device buffers: every call made here returns before any launch and touches nothing)."""
import ctypes as C

import numpy as np
import pytest

import gemm_gen_cases as GC
from gemm_gen_cases import ARG, UNSUPPORTED


# --------------------------------------------------------------------------------------------------------------------- table
def _check(p):
    assert 64 * p.K + 8 < 2 ** 24 and np.abs(p.ref).max() + 8 <= 64 * p.K + 8
    assert np.array_equal(p.ref, p.a @ p.b.T)                                   # (numpy's own int64 product)
    for cmode in GC.C_MODES:
        for acc in (0, 1):
            assert np.array_equal(GC.reference(p, cmode, acc), p.image(cmode, acc)), (p.M, p.N, p.K, p.layout, cmode, acc)


def test_rows_cols_table():
    """the exactness bound holds and the reference alone (the ABI's index formulas over the flat NaN-surrounded buffers)
    reproduces the expected canvas image, for every problem of the rows x columns grid"""
    n = 0
    for layout, M, N, K in GC.rows_cols_cases():
        _check(GC.Problem(M, N, K, layout, (1,)))
        n += 1
    assert n == sum(GC.allowed(l, M, N) for l in GC.LAYOUTS for M in GC.MS + GC.M_EXTRA for N in GC.NS) > 300


def test_k_table():
    for layout, M, N, K, cmodes in GC.k_cases():
        p = GC.Problem(M, N, K, layout, (2,))
        if K <= 288 or M == 5:
            _check(p)
        for nslab in (2, 3, 64):                                                 # the slices add up to the product
            if GC.ktiles(K) >= nslab:
                assert np.array_equal(sum(p.partial(nslab, s) for s in range(nslab)), p.ref)


def test_group_table():
    for layout in GC.LAYOUTS:
        for pool, Ms in GC.POOLS.items():
            assert all(m <= 64 for m in Ms) or all(64 < m <= 512 for m in Ms) or all(m > 512 for m in Ms)
            for n in GC.GROUP_SIZES:
                spec = GC.group_spec(layout, pool, n)
                assert len(spec) == n and len(set(s[:3] for s in spec)) == n and n <= GC.MAX_TASKS
                assert {s[3] for s in spec} == {0, 1}                          # one task accumulates beside one that does not
                assert GC.can_split(*spec[0][1:3]) and not GC.can_split(*spec[1][1:3])
                if n >= 3:
                    assert GC.can_split(*spec[2][1:3])                          # the unsplittable task lies between split ones
                for q in GC.make_group(layout, spec, (3,)):
                    assert 64 * q.K + 8 < 2 ** 24
            sh = GC.make_group(layout, GC.shared_a_spec(pool), (4,), share_a=True)
            assert all(q.A is sh[0].A for q in sh) and len({q.N for q in sh}) == len(sh)
    _check(GC.make_group((1, 1), GC.group_spec((1, 1), "mid", 3), (3,))[2])


def test_operand_buffers():
    """NaN everywhere around an operand except the zero padding of a k-major one; the readable padding of a k-minor A is NaN"""
    v = np.arange(1, 5 * 37 + 1).reshape(5, 37) % 17 - 8
    kmaj, kmin = GC.Operand(v, 0), GC.Operand(v, 1)
    assert np.array_equal(kmaj.read(), v) and np.array_equal(kmin.read(), v)
    b = kmaj.buf
    assert (b[GC.G:GC.G + 5, GC.OFF + 37:GC.OFF + 40] == 0).all() and np.isnan(b[GC.G:GC.G + 5, GC.OFF + 40:]).all()
    assert np.isnan(b[:GC.G]).all() and np.isnan(b[GC.G + 5:]).all() and np.isnan(b[:, :GC.OFF]).all()
    b = kmin.buf
    assert np.isnan(b[GC.G:GC.G + 37, GC.OFF + 5:]).all() and np.isnan(b[GC.G + 37:]).all() and np.isnan(b[:GC.G]).all()
    assert kmin.ld >= GC.up4(5) and kmaj.ld >= GC.up4(37) and b.shape[0] >= GC.G + 37 + GC.G


def test_the_tables_hit_every_edge():
    rc = list(GC.rows_cols_cases())
    kc = list(GC.k_cases())
    assert {c[0] for c in rc} == {c[0] for c in kc} == set(GC.LAYOUTS)
    for layout in GC.LAYOUTS:
        ns = {c[2] for c in rc if c[0] == layout}
        assert {n % 4 == 0 for n in ns} == ({True} if layout[1] else {True, False})
        assert {n % 64 for n in ns} >= {0, 4, 60}                              # whole, nearly empty and nearly full column tiles
        ms = {c[1] for c in rc if c[0] == layout}
        assert ms >= {4, 5, 63, 64, 65, 127, 128, 129, 130, 200, 513, 577} and ((1 in ms) != bool(layout[0]))
        ks = {c[3] for c in kc if c[0] == layout}
        assert ks == set(GC.KS)
        assert any(k & 3 for k in ks) and any(k & 31 and not k & 3 for k in ks)
        kts = {GC.ktiles(k) for k in ks}
        assert 7 in kts and 8 in kts and 9 in kts and 257 in kts and min(kts) == 1
        assert {m for c in kc if c[0] == layout for m in c[4]} == set(GC.C_MODES)
    assert {1, 3} <= {c[2] % 4 for c in rc}                                    # N % 4 in {1, 3}: k-major B only
    assert GC.K_ROWS_COLS & 31 and GC.ktiles(GC.K_ROWS_COLS) == 2
    assert max(GC.KS) == 8224 and 64 * 8224 + 8 < 2 ** 24
    assert set(GC.GROUP_SIZES) == {2, 3, 6}
    # the forced depths reach: no split, 2..63 and the cap of 64 with uneven slices
    seen = {GC.expected_nslab(K, 132, "aligned", kp) for K in GC.KS for kp in GC.KPERS if kp}
    assert 0 in seen and 64 in seen and any(2 <= s < 64 for s in seen), seen
    assert GC.expected_nslab(8224, 132, "aligned", 4) == 64 and 257 % 64 != 0
    assert GC.expected_nslab(224, 132, "aligned", 4) == 0 and GC.expected_nslab(256, 132, "aligned", 4) == 2
    assert GC.expected_nslab(8224, 132, "odd_col", 4) == GC.expected_nslab(8224, 132, "odd_ld", 4) == 0
    assert GC.expected_nslab(8224, 130, "aligned", 4) == 0 and GC.expected_nslab(2080, 132, "aligned", 1000) == 0
    for N in GC.NS:
        geo = {m: GC.c_geometry(N, m) for m in GC.C_MODES}
        assert all(ld > N + col0 for col0, ld in geo.values())
        assert geo["aligned"][0] % 4 == 0 and geo["aligned"][1] % 4 == 0
        assert geo["odd_col"][0] % 2 == 1 and geo["odd_col"][1] % 4 == 0 and geo["odd_ld"][1] % 4 != 0


# --------------------------------------------------------------------------------------------------------------------- slices
def test_slice_formula_partitions_the_k_tiles():
    """[s kt / n, (s + 1) kt / n) for all kt <= 300, n <= min(64, kt): every k-tile in exactly one slice, no slice empty,
    slices in order, sizes within one of each other"""
    for kt in range(1, 301):
        for n in range(1, min(64, kt) + 1):
            owner = np.zeros(kt, np.int64)
            sizes = []
            for s in range(n):
                lo, hi = GC.slice_tiles(kt, n, s)
                assert 0 <= lo < hi <= kt, (kt, n, s)
                owner[lo:hi] += 1
                sizes.append(hi - lo)
            assert (owner == 1).all(), (kt, n)
            assert GC.slice_tiles(kt, n, 0)[0] == 0 and GC.slice_tiles(kt, n, n - 1)[1] == kt
            assert max(sizes) - min(sizes) <= 1
    assert GC.slice_k(8224, 64, 63) == (32 * (63 * 257 // 64), 8224) and GC.slice_k(100, 2, 1) == (64, 100)


# --------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import build
    build.build()
    from show_edit_tell_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def mem():
    block = np.full(1 << 16, 0xA5, np.uint8)
    base = block.ctypes.data + (-block.ctypes.data) % 256
    yield base
    assert (block == 0xA5).all()


def _desc(mem, **o):
    from show_edit_tell_amd._lib import GemmDesc
    d = dict(A=mem + 4096, lda=64, B=mem + 8192, ldb=64, C=mem + 12288, ldc=64, M=8, N=8, K=8, accumulate=0)
    d.update(o)
    return GemmDesc(d["A"], d["lda"], d["B"], d["ldb"], d["C"], d["ldc"], d["M"], d["N"], d["K"], d["accumulate"])


def _group(lib, mem, descs, layout, slabs=False):
    from show_edit_tell_amd._lib import GemmDesc, SlabSrc
    arr = (GemmDesc * max(len(descs), 1))(*descs)
    ws, nb = mem + 32768, 1 << 14
    if slabs:
        out = (SlabSrc * max(len(descs), 1))()
        return lib.set_gemm_group_slabs_f32(arr, len(descs), layout[0], layout[1], ws, nb, out, None)
    return lib.set_gemm_group_f32(arr, len(descs), layout[0], layout[1], ws, nb, None)


@pytest.mark.parametrize("slabs", [False, True], ids=["group", "group_slabs"])
def test_host_refusals(lib, mem, slabs):
    one = lambda layout, **o: _group(lib, mem, [_desc(mem, **o)], layout, slabs)
    for layout in GC.LAYOUTS:
        assert one(layout, lda=66) == ARG and one(layout, ldb=62) == ARG and one(layout, lda=65) == ARG
        for bad in (4, 8, 12):
            assert one(layout, A=mem + 4096 + bad) == ARG and one(layout, B=mem + 8192 + bad) == ARG
        for key in "ABC":
            assert one(layout, **{key: None}) == ARG
        for key in "MNK":
            assert one(layout, **{key: 0}) == ARG and one(layout, **{key: -3}) == ARG
        # seven tasks; no descriptor array
        assert _group(lib, mem, [_desc(mem)] * 7, layout, slabs) == ARG
        from show_edit_tell_amd._lib import SlabSrc
        if slabs:
            assert lib.set_gemm_group_slabs_f32(None, 1, layout[0], layout[1], mem + 32768, 1 << 14, (SlabSrc * 1)(), None) == ARG
        else:
            assert lib.set_gemm_group_f32(None, 1, layout[0], layout[1], mem + 32768, 1 << 14, None) == ARG
        # mixed row classes (64-row class up to 512 rows by default), in either order and behind valid tasks
        small, big = _desc(mem, M=64, lda=608), _desc(mem, M=600, lda=608)
        assert _group(lib, mem, [small, big], layout, slabs) == ARG
        assert _group(lib, mem, [big, big, small], layout, slabs) == ARG
    # a ragged contraction length wants k-major rows readable (and zero) up to round_up(K, 4)
    assert one((0, 0), K=9, lda=8) == UNSUPPORTED and one((0, 0), K=9, ldb=8) == UNSUPPORTED
    assert one((0, 1), K=9, lda=8) == UNSUPPORTED and one((1, 0), K=9, ldb=8) == UNSUPPORTED
    assert one((0, 0), K=70, lda=68, ldb=72) == UNSUPPORTED
    # a k-minor A: at least 4 rows; a ragged M wants lda >= round_up(M, 4)
    for layout in ((1, 1), (1, 0)):
        for M in (1, 2, 3):
            assert one(layout, M=M) == UNSUPPORTED
        assert one(layout, M=6, lda=4) == UNSUPPORTED and one(layout, M=69, lda=68) == UNSUPPORTED
    # a k-minor B: N a multiple of 4
    for layout in ((0, 1), (1, 1)):
        for N in (1, 2, 3, 6, 66):
            assert one(layout, N=N) == UNSUPPORTED
    # every task is looked at, not the first
    assert _group(lib, mem, [_desc(mem), _desc(mem), _desc(mem, N=6)], (0, 1), slabs) == UNSUPPORTED
    assert _group(lib, mem, [_desc(mem), _desc(mem, lda=66)], (0, 0), slabs) == ARG


def test_host_refusals_single(lib, mem):
    """set_gemm_f32: the same refusals; M <= 0 or N <= 0 is an empty product (SET_OK, csrc/gemm_gen.hip gemm_gen), K <= 0 is not"""
    def one(layout=(0, 0), **o):
        d = _desc(mem, **o)
        return lib.set_gemm_f32(d.A, d.lda, layout[0], d.B, d.ldb, layout[1], d.C, d.ldc, d.M, d.N, d.K, 0, mem + 32768, 1 << 14, None)
    assert one(M=0) == 0 and one(N=0) == 0 and one(M=-1) == 0
    assert one(K=0) == ARG and one(K=-4) == ARG
    assert one(lda=66) == ARG and one(A=mem + 4096 + 4) == ARG and one(B=None) == ARG
    assert one(K=9, lda=8) == UNSUPPORTED and one((1, 1), M=3) == UNSUPPORTED and one((1, 1), M=6, lda=4) == UNSUPPORTED
    assert one((0, 1), N=6) == UNSUPPORTED


def test_slabs_entry_needs_its_output_array(lib, mem):
    from show_edit_tell_amd._lib import GemmDesc
    arr = (GemmDesc * 1)(_desc(mem))
    assert lib.set_gemm_group_slabs_f32(arr, 1, 1, 1, mem + 32768, 1 << 14, None, None) == ARG
