// ---------------------------------------------------------------------------------------------
// gemm_nt_split_bf16 (included by gemm_f32.hip): the grouped GEMM of gemm_nt_f32<128,64> on the bf16 matrix pipe, with every
// fp32 operand split EXACTLY into three bf16 values
//      x = hi + mid + lo        (8 + 8 + 8 significand bits, round-to-nearest conversions and exact fp32 subtractions, split3.h)
// and six of the nine partial products accumulated in fp32 (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid; the
// dropped ones are <= 2^-24 relative, i.e. at the level of one fp32 rounding).  v_mfma_f32_32x32x16_bf16 has 16x
// the rate of v_mfma_f32_32x32x2_f32, so six of them cost 2.67x less matrix-pipe time than the fp32 chain.
// Splitting happens on the fly when a k-tile is staged into LDS (weights stay fp32 in HBM, nothing is
// repacked); LDS holds three bf16 planes per operand, 64-B rows, 16-B chunks XOR-swizzled by (row>>2)&3 so
// that the ds_write_b64 of the staging and the ds_read_b128 of the fragments are bank-conflict-free.
// Same task descriptors, K segments, split-K slabs, leading preloaded arguments, loop gate (GATE = 1) and compacted row list
// (GATE = 2, unsplit problems only) as gemm_nt_f32<128,64>.  Who runs on it: the launcher's word (gemm_group, SET_GEMM_SPLIT).
// GATE = 2 has gemm_nt_f32's contract: the grid of the full launch, row tile m0 covers the list entries [m0, m0 + 128), a tile at
// or beyond the clamped count returns at once, the list is read (and every index clamped to [0, M)) where the A-row pointers are
// formed and where the C rows are stored.  Staging, split, k-loop and MFMA order are those of the full launch, so every computed
// element has the bits the full split launch gives it.
//
// Values the planes cannot carry.  The split of +-inf is (inf, NaN, NaN) and a finite |x| >= 2^128 - 2^119 rounds its hi plane
// to inf, so the six products of such an operand give NaN where the fp32 chain gives +-inf (or a finite number).  Finite
// operands with a finite result never produce a non-finite accumulator, so the epilogue takes every non-finite accumulator
// as the sign of such an operand and recomputes THAT element as a plain fp32 FMA chain over the workgroup's K slice: the
// result is the fp32 path's +-inf / NaN / finite value, the other elements keep the split product.  At the small end the lo
// plane of |x| < 2^-109 falls below bf16's normal range; operands scaled by 2^-100 and by 2^100 keep the error of the unscaled
// ones digit for digit (tests/test_hip_gemm_split.py).
// ---------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int SPLIT_LDS_BYTES = 2 * 3 * (128 + 64) * 64;      // two stages of three bf16 planes per operand: 72 KB, two workgroups per CU

template <int GATE>
__global__ void __launch_bounds__(256) gemm_nt_split_bf16(const int ntasks, const int wb1, const int wb2, const int wb3,
                                                          const int wb4, const int wb5, const int* const gate_alive,
        const int* const gate_nrows, const GemmLaunch L) {
    constexpr int BM = 128, BN = 64, TM = 2, LA = 4, LW = 2;
    constexpr int ROWB = 64;                              // bytes per LDS row (32 bf16)
    constexpr int PLANE_A = BM * ROWB, PLANE_W = BN * ROWB;
    constexpr int BUF = 3 * (PLANE_A + PLANE_W);          // 36 KB per stage
    static_assert(2 * BUF == SPLIT_LDS_BYTES, "launcher's dynamic LDS size");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;

    static_assert(GEMM_MAX_TASKS == 6, "five leading wg_begin arguments");
    int ti = 0;
    {
        const int bid = (int)blockIdx.x;
        if (1 < ntasks && bid >= wb1) ti = 1;
        if (2 < ntasks && bid >= wb2) ti = 2;
        if (3 < ntasks && bid >= wb3) ti = 3;
        if (4 < ntasks && bid >= wb4) ti = 4;
        if (5 < ntasks && bid >= wb5) ti = 5;
    }
    const GemmTask& T = L.t[ti];
    // workgroup -> (row tile tm, column tile tn, k-slice ks).  Row tiles of the same (tn, ks) read the same
    // weight block; their block ids differ by tm_stride, a multiple of 8, so they land on the SAME XCD (blocks
    // go round-robin over the 8 XCDs) and the second reader finds the block in that XCD's L2.
    const int local = (int)blockIdx.x - T.wg_begin;
    const int tm = local / T.tm_stride;
    const int rem = local - tm * T.tm_stride;
    if (rem >= T.tiles_n * T.ksplit) return;          // padding slot
    // row gate of the decode loops (set_common.h), as in gemm_nt_f32: nothing to do once the reference has left its loop
    if constexpr (GATE == 1) {
        if (gate_alive && *gate_alive == 0) return;
    }
    const int ks = rem % T.ksplit;
    const int tn = rem / T.ksplit;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kt0 = (int)(((long long)ks * T.ktiles) / T.ksplit);
    const int kt1 = (int)(((long long)(ks + 1) * T.ktiles) / T.ksplit);
    // compacted row list, as in gemm_nt_f32: gate_nrows is the length of L.row_list (else an unused slot)
    int epi_m = T.M;
    const int* const rlist = L.row_list;
    if constexpr (GATE == 2) {
        const int cnt = *gate_nrows;
        epi_m = cnt < 0 ? 0 : (cnt < T.M ? cnt : T.M);
        if (m0 >= epi_m) return;                      // (uniform over the workgroup, before its first barrier)
    } else {
        (void)gate_nrows;
    }
    auto epi_row = [&](int row) {                     // tile row (< epi_m) -> row of A and of C
        if constexpr (GATE == 2) { const int i = rlist[row]; return i < 0 ? 0 : (i < T.M ? i : T.M - 1); }
        else return row;
    };

    const int srow = tid >> 3, kc = tid & 7, scol = kc * 4;
    // byte offset of this thread's 8-byte store inside a plane row
    const int soff = srow * ROWB + (((kc >> 1) ^ ((srow >> 2) & 3)) << 4) + ((kc & 1) << 3);
    int arow[LA], wrow[LW];
#pragma unroll
    for (int i = 0; i < LA; ++i) { int r = m0 + srow + 32 * i; r = r < epi_m ? r : epi_m - 1; arow[i] = epi_row(r); }
#pragma unroll
    for (int i = 0; i < LW; ++i) { int r = n0 + srow + 32 * i; wrow[i] = r < T.N ? r : T.N - 1; }

    f32x4 ra0[LA], rw0[LW], ra1[LA], rw1[LW];
    const float* pa[LA];
    const float* pw[LW];
    int seg_end = 0;
#define SPL_SEEK(KT)                                                                                    \
    {                                                                                                   \
        const int kt_ = (KT);                                                                           \
        int s_ = 0, kbase_ = 0;                                                                         \
        _Pragma("unroll") for (int i = 0; i < GEMM_MAX_SEG - 1; ++i)                                    \
            if (i + 1 < T.nseg && kt_ >= T.kt_end[i]) { s_ = i + 1; kbase_ = T.kt_end[i]; }             \
        const float* Ab_ = T.A[0];                                                                      \
        const float* Wb_ = T.W[0];                                                                      \
        long long lda_ = T.lda[0], ldw_ = T.ldw[0];                                                     \
        seg_end = T.kt_end[0];                                                                          \
        _Pragma("unroll") for (int i = 1; i < GEMM_MAX_SEG; ++i)                                        \
            if (s_ == i) { Ab_ = T.A[i]; Wb_ = T.W[i]; lda_ = T.lda[i]; ldw_ = T.ldw[i]; seg_end = T.kt_end[i]; } \
        const long long koff_ = (long long)(kt_ - kbase_) * GEMM_BK + scol;                             \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) pa[i] = Ab_ + arow[i] * lda_ + koff_;            \
        _Pragma("unroll") for (int i = 0; i < LW; ++i) pw[i] = Wb_ + wrow[i] * ldw_ + koff_;            \
    }
#define SPL_GLOAD(RA, RW)                                                                           \
    {                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) { RA[i] = *(gptr4)(pa[i]); pa[i] += GEMM_BK; } \
        _Pragma("unroll") for (int i = 0; i < LW; ++i) { RW[i] = *(gptr4)(pw[i]); pw[i] += GEMM_BK; } \
    }
#ifdef SPL_EXP_NOGLOAD        /* diagnostic: only the prologue's tiles are ever requested */
#define SPL_STAGE(KT, RA, RW) if ((KT) < kt0 + 3 && (KT) < kt1) { if ((KT) == seg_end) SPL_SEEK(KT); SPL_GLOAD(RA, RW); }
#else
#define SPL_STAGE(KT, RA, RW)                                                                       \
    if ((KT) < kt1) {                                                                                   \
        if ((KT) == seg_end) SPL_SEEK(KT);                                                              \
        SPL_GLOAD(RA, RW);                                                                          \
    }
#endif
#ifdef SPL_EXP_NOSPLIT        /* diagnostic: no split arithmetic, the planes get raw bits */
#define SPL_SPLIT3(X, H, M, L) { const u32x4 b_ = __builtin_bit_cast(u32x4, X); H = (u32x2){b_.x, b_.y}; M = (u32x2){b_.z, b_.w}; L = (u32x2){b_.y, b_.z}; }
#else
#define SPL_SPLIT3(X, H, M, L) split3(X, H, M, L)
#endif
    // registers (fp32) -> three bf16 planes in LDS
#define SPL_LSTORE(B, RA, RW)                                                                       \
    {                                                                                                   \
        char* sA_ = smem + (B) * BUF + soff;                                                            \
        char* sW_ = smem + (B) * BUF + 3 * PLANE_A + soff;                                              \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) {                                                \
            u32x2 h_, m_, l_;                                                                           \
            SPL_SPLIT3(RA[i], h_, m_, l_);                                                              \
            *reinterpret_cast<u32x2*>(sA_ + i * 32 * ROWB) = h_;                                        \
            *reinterpret_cast<u32x2*>(sA_ + i * 32 * ROWB + PLANE_A) = m_;                              \
            *reinterpret_cast<u32x2*>(sA_ + i * 32 * ROWB + 2 * PLANE_A) = l_;                          \
        }                                                                                               \
        _Pragma("unroll") for (int i = 0; i < LW; ++i) {                                                \
            u32x2 h_, m_, l_;                                                                           \
            SPL_SPLIT3(RW[i], h_, m_, l_);                                                              \
            *reinterpret_cast<u32x2*>(sW_ + i * 32 * ROWB) = h_;                                        \
            *reinterpret_cast<u32x2*>(sW_ + i * 32 * ROWB + PLANE_W) = m_;                              \
            *reinterpret_cast<u32x2*>(sW_ + i * 32 * ROWB + 2 * PLANE_W) = l_;                          \
        }                                                                                               \
    }

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    const int frow = lane & 31;
    const int fsw = (frow >> 2) & 3;
    // byte offsets of this lane's fragment rows (A: 2 sub-tiles, W: 1) and of its chunk in k16-step 0 / 1
    const int fa0 = (wm * 64 + frow) * ROWB, fw0 = (wn * 32 + frow) * ROWB;
    const int fc[2] = {(((lane >> 5)) ^ fsw) << 4, ((2 + (lane >> 5)) ^ fsw) << 4};
#define SPL_FRAG(S, FA, FW)                                                                             \
    {                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                  \
            _Pragma("unroll") for (int p = 0; p < 3; ++p)                                               \
                FA[i][p] = *reinterpret_cast<const u32x4*>(sA + p * PLANE_A + fa0 + i * 32 * ROWB + fc[S]); \
        _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                   \
            FW[p] = *reinterpret_cast<const u32x4*>(sW + p * PLANE_W + fw0 + fc[S]);                    \
    }
#ifdef SPL_EXP_NOMFMA         /* diagnostic: the fragments are consumed by one VALU add instead of an MFMA */
#define SPL_MM(I, PA, PW) acc[I][(PA) * 3 + (PW)] += __uint_as_float(fa_[I][PA].x ^ fw_[PW].y)
#else
#define SPL_MM(I, PA, PW) acc[I] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                             \
        __builtin_bit_cast(bf16x8, fa_[I][PA]), __builtin_bit_cast(bf16x8, fw_[PW]), acc[I], 0, 0, 0)
#endif
    // six products per sub-tile, smallest first; the two sub-tiles alternate so consecutive MFMAs are independent
#define SPL_MFMA(FA, FW)                                                                                \
    {                                                                                                   \
        auto& fa_ = FA; auto& fw_ = FW;                                                                 \
        SPL_MM(0, 0, 2); SPL_MM(1, 0, 2);                                                               \
        SPL_MM(0, 2, 0); SPL_MM(1, 2, 0);                                                               \
        SPL_MM(0, 1, 1); SPL_MM(1, 1, 1);                                                               \
        SPL_MM(0, 0, 1); SPL_MM(1, 0, 1);                                                               \
        SPL_MM(0, 1, 0); SPL_MM(1, 1, 0);                                                               \
        SPL_MM(0, 0, 0); SPL_MM(1, 0, 0);                                                               \
    }
    // One k-tile.  The split of tile kt+1 (VALU) and its LDS stores are issued IN BETWEEN the 24 MFMAs of tile kt
    // (sched_group_barrier pins the interleave: the matrix pipe runs 32 cycles per MFMA, enough for ~7 VALU
    // issues), so the conversion work hides under the matrix pipe instead of alternating with it.  The store
    // is unconditional: on the last tile it writes stale registers into the buffer nobody reads again.
#define SPL_ITER(KT, B, RA, RW)                                                                     \
    {                                                                                                   \
        const char* sA = smem + (B) * BUF;                                                              \
        const char* sW = smem + (B) * BUF + 3 * PLANE_A;                                                \
        u32x4 fA0[TM][3], fW0[3], fA1[TM][3], fW1[3];                                                   \
        SPL_FRAG(0, fA0, fW0);                                                                          \
        SPL_FRAG(1, fA1, fW1);                                                                          \
        SPL_LSTORE((B) ^ 1, RA, RW);                                                                \
        SPL_MFMA(fA0, fW0);                                                                             \
        SPL_MFMA(fA1, fW1);                                                                             \
        _Pragma("unroll") for (int q_ = 0; q_ < 24; ++q_) {                                             \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
            __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);                                          \
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                                          \
        }                                                                                               \
        SPL_STAGE((KT) + 3, RA, RW);                                                                \
        __syncthreads();                                                                                \
    }
    if (kt0 < kt1) {
        SPL_SEEK(kt0);
        SPL_GLOAD(ra0, rw0);
        SPL_STAGE(kt0 + 1, ra1, rw1);
        SPL_LSTORE(0, ra0, rw0);
        SPL_STAGE(kt0 + 2, ra0, rw0);
        __syncthreads();
    }
    for (int kt = kt0; kt < kt1; kt += 2) {
        SPL_ITER(kt, 0, ra1, rw1);
        if (kt + 1 < kt1) SPL_ITER(kt + 1, 1, ra0, rw0);
    }
#undef SPL_ITER
#undef SPL_MFMA
#undef SPL_MM
#undef SPL_FRAG
#undef SPL_LSTORE
#undef SPL_SPLIT3
#undef SPL_STAGE
#undef SPL_GLOAD
#undef SPL_SEEK

    // element (row, col) of this workgroup's K slice as a plain fp32 FMA chain (operands the planes cannot carry: see the top)
    auto dot_f32 = [&](int row, int col) {
        float s = 0.f;
        int sb = 0;
        for (int sg = 0; sg < T.nseg; ++sg) {
            const int se = T.kt_end[sg];
            const int a = kt0 > sb ? kt0 : sb, b = kt1 < se ? kt1 : se;
            if (a < b) {
                const float* xa = T.A[sg] + (long long)row * T.lda[sg] + (long long)(a - sb) * GEMM_BK;
                const float* xw = T.W[sg] + (long long)col * T.ldw[sg] + (long long)(a - sb) * GEMM_BK;
                const int nk = (b - a) * GEMM_BK;
                for (int k = 0; k < nk; ++k) s = fmaf(xa[k], xw[k], s);
            }
            sb = se;
        }
        return s;
    };
    float* Cs = T.C + (long long)ks * T.slab_stride;
    const bool fused = (T.ksplit == 1);
    const int crow0 = m0 + wm * 64 + 4 * (lane >> 5);
    const int col = n0 + wn * 32 + (lane & 31);
    if (col < T.N) {
        const float bv = (fused && T.bias) ? T.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = crow0 + i * 32 + (r & 3) + 8 * (r >> 2);
                if (row < epi_m) {
                    const int crow = epi_row(row);
                    float v = acc[i][r];
                    if (!(fabsf(v) <= 3.402823466e+38f)) v = dot_f32(crow, col);     // inf or NaN
                    if (fused) v = apply_act(v + bv, T.act);
                    Cs[(long long)crow * T.ldc + col] = v;
                }
            }
        }
    }
}
