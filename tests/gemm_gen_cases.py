"""Case tables and host reference (test infrastructure) for the general-layout fp32 GEMM of csrc/gemm_gen.hip
(set_gemm_f32, set_gemm_group_f32, set_gemm_group_slabs_f32).  Importable without a device: numpy only.
tests/test_gemm_gen_cases_cpu.py checks this module against itself; tests/test_hip_gemm_gen.py lets it judge the kernel.

Exact pass.  A and B hold integers from [-8, 8] stored as fp32.  Every product is an integer of at most 64 and every partial
sum in any order one of at most 64 K (+ 8 for a prefilled C) < 2^24, so whatever the tile, the slice or the order of the
reduction the result must equal the integer product BIT FOR BIT.  (The integer product is formed by float64 BLAS, which is exact
below 2^53, and converted to int64.)  The bound is asserted per problem from its actual K.

Operands.  Each operand lies inside a wider NaN-filled buffer, at a column offset that is a multiple of 4 floats, with NaN
guard rows above and below (for a k-minor operand the rows below are the rows k >= K, which are never read).  Two kinds of
padding differ: the columns K .. round_up(K, 4) - 1 of a k-major operand hold the ZEROS the ABI demands of the caller; the
columns M .. round_up(M, 4) - 1 of a k-minor A hold NaN: they may be read and must not reach a stored element.

Outputs.  Every C is a view into a canvas of sentinels (a NaN with a payload) with ldc > N, guard rows above and below and
guard columns on both sides; the whole canvas is compared with the expected bit image."""
import numpy as np

SENT = 0x7FC12345          # tests/test_hip_gemm_nt.py: a quiet NaN with a payload, "nobody wrote here"
G = 8                      # guard rows on either side of C and of every operand
OFF = 8                    # column offset of an operand inside its buffer (floats; the ABI wants a multiple of 4)
ARG, UNSUPPORTED = 1, 2    # include/set_hip.h SET_ERR_ARG, SET_ERR_UNSUPPORTED

LAYOUTS = ((0, 0), (0, 1), (1, 1), (1, 0))                   # (a_kminor, b_kminor)
LAYOUT_NAME = {(0, 0): "nt", (0, 1): "nn", (1, 1): "tn", (1, 0): "tt"}      # the kernel's profile tags
C_MODES = ("aligned", "odd_col", "odd_ld")                   # the last two can only take the scalar epilogue

MS = (1, 4, 5, 63, 64, 65, 127, 128, 129, 130, 513, 577)
M_EXTRA = (200,)           # overhangs the 128-row class when it is forced for every M > 64
NS = (1, 3, 4, 60, 64, 68, 130, 132)
KS = (4, 32, 36, 100, 33, 37, 224, 256, 288, 2080, 8224)
K_ROWS_COLS = 36           # two k-tiles, the second ragged
KPERS = (None, 4, 5, 1000)                                   # None: the planner's own choice; else SET_EXP_GEN_KPER
K_SHAPES = ((5, 68, ("aligned",)), (65, 132, C_MODES), (130, 60, ("aligned",)), (130, 130, ("aligned",)), (513, 68, ("aligned",)))
MAX_SLABS, MIN_SPLIT_KT, MAX_TASKS = 64, 8, 6


def up4(x):
    return (x + 3) & ~3


def ktiles(K):
    return (K + 31) // 32


def allowed(layout, M, N):
    """the ABI: a k-minor A needs M >= 4, a k-minor B needs N % 4 == 0 and N >= 4"""
    return (not layout[0] or M >= 4) and (not layout[1] or (N % 4 == 0 and N >= 4))


def slice_tiles(kt, nslab, s):
    """k-tiles [lo, hi) of slice s of a problem of kt k-tiles split nslab ways (csrc/gemm_gen.hip: kt0, kt1)"""
    return s * kt // nslab, (s + 1) * kt // nslab


def slice_k(K, nslab, s):
    lo, hi = slice_tiles(ktiles(K), nslab, s)
    return 32 * lo, min(K, 32 * hi)


def c_geometry(N, cmode):
    """-> (first column of the C view inside its canvas, ldc)"""
    ld = up4(N) + 12
    return {"aligned": (4, ld), "odd_col": (5, ld), "odd_ld": (4, ld + 1)}[cmode]


def takes_vec(N, cmode):
    """whether the output can take 16-byte stores: N % 4 == 0, ldc % 4 == 0, C 16-byte aligned"""
    return N % 4 == 0 and cmode == "aligned"


def expected_nslab(K, N, cmode, kper):
    """what set_gemm_group_slabs_f32 must report under SET_EXP_GEN_KPER = kper and a generous scratch: no split below 8
    k-tiles or without 16-byte stores, else min(64, ceil(kt / kper)) — where a "split" into one slice is no split (0)"""
    kt = ktiles(K)
    if kt < MIN_SPLIT_KT or not takes_vec(N, cmode):
        return 0
    n = min(MAX_SLABS, -(-kt // kper))
    return n if n >= 2 else 0


def slab_bytes(M, N):
    return -(-M * N * 4 // 256) * 256


def generous_scratch(probs):
    """room for the deepest split of every problem that can split at all (and for one slab of the others), + slack"""
    return sum((MAX_SLABS if ktiles(p.K) >= MIN_SPLIT_KT and p.N % 4 == 0 else 1) * slab_bytes(p.M, p.N) for p in probs) + 4096


class Operand:
    """vals (X, K) — X = M or N — as the ABI reads it, inside a wider NaN buffer.  Element (x, k) is buf.flat[offset + x ld + k]
    (k-major) or buf.flat[offset + k ld + x] (k-minor)."""

    def __init__(self, vals, kminor):
        X, K = vals.shape
        self.X, self.K, self.kminor = X, K, bool(kminor)
        if kminor:
            self.ld = up4(X) + OFF + 8
            self.buf = np.full((G + K + G, self.ld), np.nan, np.float32)
            self.buf[G:G + K, OFF:OFF + X] = vals.T            # (columns X .. up4(X) - 1 stay NaN: readable padding)
        else:
            self.ld = up4(K) + OFF + 8
            self.buf = np.full((G + X + G, self.ld), np.nan, np.float32)
            self.buf[G:G + X, OFF:OFF + K] = vals
            self.buf[G:G + X, OFF + K:OFF + up4(K)] = 0.0      # the zero padding the ABI demands when K % 4 != 0
        self.offset = G * self.ld + OFF
        assert self.ld % 4 == 0 and self.offset % 4 == 0

    def read(self):
        """the (X, K) matrix the ABI's index formula reads from the flat buffer (float64)"""
        x, k = np.arange(self.X)[:, None], np.arange(self.K)[None, :]
        idx = self.offset + (k * self.ld + x if self.kminor else x * self.ld + k)
        return self.buf.reshape(-1)[idx].astype(np.float64)


def _product(a, b):
    """exact integer product a (M, K) . b (N, K)^T"""
    if a.shape[1] == 0:
        return np.zeros((a.shape[0], b.shape[0]), np.int64)
    p = a.astype(np.float64) @ b.astype(np.float64).T          # exact: |sum| <= 64 K < 2^53
    out = p.astype(np.int64)
    assert np.array_equal(out.astype(np.float64), p)
    return out


class Problem:
    """one exact problem: integer operands in their buffers, the integer product, an integer prefill for accumulate = 1"""

    def __init__(self, M, N, K, layout, seed, share_a=None):
        assert allowed(layout, M, N), (layout, M, N)
        self.M, self.N, self.K, self.layout = M, N, K, tuple(layout)
        assert 64 * K + 8 < 2 ** 24, K                         # every partial sum in any order is exact in fp32
        rng = np.random.default_rng([int(s) for s in seed] + [M, N, K, 2 * layout[0] + layout[1]])
        if share_a is None:
            self.a = rng.integers(-8, 9, (M, K))
            self.A = Operand(self.a, layout[0])
        else:
            assert (share_a.M, share_a.K) == (M, K)
            self.a, self.A = share_a.a, share_a.A
        self.b = rng.integers(-8, 9, (N, K))
        self.B = Operand(self.b, layout[1])
        self.c0 = rng.integers(-8, 9, (M, N))
        self._parts = {}
        self.ref = _product(self.a, self.b)
        assert np.abs(self.ref).max() + 8 <= 64 * K + 8 < 2 ** 24

    def partial(self, nslab, s):
        """the exact product over the k range of slice s of nslab (computed once)"""
        if (nslab, s) not in self._parts:
            lo, hi = slice_k(self.K, nslab, s)
            self._parts[nslab, s] = _product(self.a[:, lo:hi], self.b[:, lo:hi])
        return self._parts[nslab, s]

    def canvas0(self, cmode, accumulate):
        """the canvas before the launch: sentinels; the integer prefill inside the view when the launch accumulates"""
        col0, ld = c_geometry(self.N, cmode)
        img = np.full((self.M + 2 * G, ld), SENT, np.uint32)
        if accumulate:
            img[G:G + self.M, col0:col0 + self.N] = self.c0.astype(np.float32).view(np.uint32)
        return img

    def image(self, cmode, accumulate, values=None):
        """the canvas after the launch (values: what the view must hold; default the product, + the prefill)"""
        col0, _ = c_geometry(self.N, cmode)
        img = self.canvas0(cmode, accumulate)
        v = (self.ref + (self.c0 if accumulate else 0)) if values is None else values
        img[G:G + self.M, col0:col0 + self.N] = v.astype(np.float32).view(np.uint32)
        return img

    def c_offset(self, cmode):
        col0, ld = c_geometry(self.N, cmode)
        return G * ld + col0, ld


def reference(p, cmode, accumulate):
    """the host reference: the ABI's own index formulas over the flat buffers, float64, stored into the canvas"""
    a, b = p.A.read(), p.B.read()
    assert not np.isnan(a).any() and not np.isnan(b).any()
    c = a @ b.T
    img = p.canvas0(cmode, accumulate)
    off, ld = p.c_offset(cmode)
    flat = img.reshape(-1)
    idx = off + np.arange(p.M)[:, None] * ld + np.arange(p.N)[None, :]
    if accumulate:
        c = c + flat[idx].view(np.float32).astype(np.float64)
    flat[idx] = c.astype(np.float32).view(np.uint32)
    return img


# --------------------------------------------------------------------------------------------------------------------- the grid
def rows_cols_cases():
    """every M against every N, two k-tiles (the second ragged), every C alignment, both accumulate modes"""
    for layout in LAYOUTS:
        for M in MS + M_EXTRA:
            for N in NS:
                if allowed(layout, M, N):
                    yield layout, M, N, K_ROWS_COLS


def k_cases():
    """every K on shapes of 1 x 2, 2 x 3 and 3 x 1 tiles (64-row class), one that cannot split (N = 130, k-major B only) and
    one of 513 rows (the 128-row class whenever the depth is forced: 5 row tiles, one live row in the last)"""
    for layout in LAYOUTS:
        for K in KS:
            for M, N, cmodes in K_SHAPES:
                if allowed(layout, M, N):
                    yield layout, M, N, K, cmodes


# row pools of ONE row-tile class each, whatever SET_GEMM_GEN_BM64_UPTO (512, or 64 in the forced-route runs) says
POOLS = {"small": (5, 33, 64), "mid": (65, 129, 130, 200), "big": (513, 577)}
# (N, K, accumulate) of the tasks of a group; task 1 cannot split (N = 66: no 16-byte rows; K = 128: 4 k-tiles) and lies
# between tasks that do.  A k-minor B cannot have N = 66.
GROUP_TASKS = ((64, 256, 0), (66, 1024, 1), (132, 2080, 1), (68, 288, 0), (4, 100, 1), (60, 520, 0))
GROUP_TASKS_BKMINOR = ((64, 256, 0), (64, 128, 1), (132, 2080, 1), (68, 288, 0), (4, 100, 1), (60, 520, 0))
GROUP_SIZES = (2, 3, 6)


def group_spec(layout, pool, n):
    """-> [(M, N, K, accumulate)] of a group of n tasks with different shapes in one row class"""
    tasks = GROUP_TASKS_BKMINOR if layout[1] else GROUP_TASKS
    Ms = POOLS[pool]
    return [(Ms[(i + 1) % len(Ms)],) + tasks[i] for i in range(n)]


def shared_a_spec(pool):
    """three tasks that share one A (same M, K), as the dX products of one module's backward share dY"""
    M = POOLS[pool][-1]
    return [(M, N, 288, acc) for N, acc in ((64, 0), (132, 1), (68, 0))]


def make_group(layout, spec, seed, share_a=False):
    probs = []
    for i, (M, N, K, _) in enumerate(spec):
        probs.append(Problem(M, N, K, layout, list(seed) + [i], share_a=probs[0] if share_a and i else None))
    return probs


def can_split(N, K, cmode="aligned"):
    return ktiles(K) >= MIN_SPLIT_KT and takes_vec(N, cmode)


# the float problems of the rounding pass: (M, N, K); M = 130: the 64-row class, 577: the 128-row one (forced depth)
ROUND_SHAPES = ((130, 132, 1000), (577, 68, 1000))
ROUND_KPERS = (1000, 4)                                      # unsplit, split 8 ways


class FloatProblem:
    """normal floats in the same buffers; the float64 product"""

    def __init__(self, M, N, K, layout, seed):
        rng = np.random.default_rng([int(s) for s in seed] + [M, N, K, 2 * layout[0] + layout[1]])
        self.M, self.N, self.K, self.layout = M, N, K, tuple(layout)
        a = rng.standard_normal((M, K)).astype(np.float32)
        b = rng.standard_normal((N, K)).astype(np.float32)
        self.A, self.B = Operand(a, layout[0]), Operand(b, layout[1])
        self.ref = a.astype(np.float64) @ b.astype(np.float64).T
        self.tol = 2e-6 * np.sqrt(K) * 4 * max(1.0, np.abs(self.ref).max())     # ktol of tests/test_hip_backward_ops.py
