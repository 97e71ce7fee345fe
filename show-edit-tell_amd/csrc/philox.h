// Philox4x32-10 counter-based generator (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), shared
// by the sampling epilogue (epilogue.hip) and the dropout kernels (train_seq.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace set {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// ---- Gumbel noise of the Gumbel-max sampler (include/set_hip.h, "Gumbel-max draw"): ONE definition for the per-step pick
// (epilogue.hip), the persistent launch (decode_persistent_wide.hip), set_gumbel_fill_f32 and the float64 restatement
// tests/gumbel_oracle.py.  Vocabulary word v of (row, t) takes output word e = v & 3 of
//   Philox4x32-10(key = (seed_lo, seed_hi), counter = (row, t + 256 (j + 1), offset_lo, offset_hi)),   j = v >> 2.
// The inverse-CDF sampler's uniform uses counter word 1 = t < 256, so with t <= 255 and j + 1 < 2^24 the two streams never
// share a counter (the host refuses max_len > 255 and V > GUMBEL_MAX_V).
// From the 32-bit word r: u = (r + 1/2) 2^-32 in (0, 1), E = -log(u) formed without cancellation at either end
// (r < 2^31: -logf of the product; otherwise -log1pf(-(1 - u)) with 1 - u = (2^32 - r) 2^-32 - 2^-33 from the exact integer),
// g = -logf(E).  E lies in [2^-33, 22.9], never 0 or infinite; g in about [-3.2, 22.9].
constexpr int GUMBEL_MAX_V = (1 << 26) - 4;      // j + 1 <= 2^24 - 1 for every word: 256 (j + 1) + t stays below 2^32
constexpr int GUMBEL_MAX_LEN = 255;

__device__ __forceinline__ float gumbel_of_word(uint32_t r) {
    float E;
    if (r < 0x80000000u) {
        E = -logf(((float)r + 0.5f) * 2.3283064365386963e-10f);
    } else {
        const float vv = (float)(0u - r) * 2.3283064365386963e-10f - 1.1641532182693481e-10f;
        E = -log1pf(-vv);
    }
    return -logf(E);
}
// the four Philox words behind vocabulary words 4 j .. 4 j + 3 of (row, t)
__device__ __forceinline__ void gumbel_quad_words(unsigned long long seed, unsigned long long offset, int row, int t, int j,
                                                  uint32_t (&c)[4]) {
    c[0] = (uint32_t)row; c[1] = (uint32_t)t + 256u * ((uint32_t)j + 1u); c[2] = (uint32_t)offset; c[3] = (uint32_t)(offset >> 32);
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// noise of ONE word (a caller that owns a whole quad calls gumbel_quad_words once and gumbel_of_word four times)
__device__ __forceinline__ float gumbel_at(unsigned long long seed, unsigned long long offset, int row, int t, int v) {
    uint32_t c[4];
    gumbel_quad_words(seed, offset, row, t, v >> 2, c);
    const int e = v & 3;
    return gumbel_of_word(e == 0 ? c[0] : e == 1 ? c[1] : e == 2 ? c[2] : c[3]);
}

}  // namespace set
