// Edit trace (set_editnet_edit_trace, host loop in editnet.hip): the record of one forced decode timestep, taken from what
// the step left in the workspace — alpha_c, alpha, cmem_pre, the logits partials — plus the one contraction the fused route
// never materialises, gate_cnew(c_new), which arrives as split-K partials of a grouped GEMM.
//
// One launch per timestep, one 256-thread workgroup per row.  Every reduction has a fixed order: per-thread
// partials in ascending index order, a xor-shuffle tree inside the wave, the four wave results combined in index order; slab
// partials are added in slab order.  No atomics.  Every element of the row's record is written by this launch (zeros and
// select = -1 for t >= n_steps[b]), so the outputs need no fill.
#include <math.h>
#include "set_common.h"

namespace set {

typedef float tr_f32x4 __attribute__((ext_vector_type(4)));

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;

// value (m, v) of a slab set, partials added in slab order (+ bias last, as the pick kernels add it)
__device__ __forceinline__ float tr_slab_at(const Slabs& s, const float* bias, long long m, int v) {
    const float* p = s.p + m * s.ld + v;
    float x = p[0];
    for (int i = 1; i < s.n; ++i) x += p[(long long)i * s.stride];
    return bias ? x + bias[v] : x;
}

// (max, sum exp(x - max)) of two disjoint sets
__device__ __forceinline__ void tr_lse_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    if (nm == -INFINITY) { m = nm; s = 0.f; return; }           // both sets empty
    s = s * expf(m - nm) + os * expf(om - nm);
    m = nm;
}

__global__ void __launch_bounds__(TR_THREADS) edit_trace_k(const EditTraceStep a) {
    __shared__ float s_f[TR_WAVES];
    __shared__ float s_m[TR_WAVES];
    __shared__ int s_i[TR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, R = a.R, D = a.D, V = a.V, t = a.t;
    const long long row = (long long)b * a.S + t;
    float* o_ac = a.out.alpha_c + row * T;
    float* o_av = a.out.alpha_v ? a.out.alpha_v + row * R : nullptr;
    float* o_gf = a.out.gate_full ? a.out.gate_full + row * D : nullptr;
    const tr_f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

    if (t >= a.n_steps[b]) {                                    // (workgroup-uniform) not recorded: zeros, select = -1
        for (int j = tid; j < T; j += TR_THREADS) o_ac[j] = 0.f;
        if (o_av) for (int r = tid; r < R; r += TR_THREADS) o_av[r] = 0.f;
        if (o_gf) for (int d = tid * 4; d < D; d += TR_THREADS * 4) *reinterpret_cast<tr_f32x4*>(o_gf + d) = z4;
        if (tid == 0) { a.out.select[row] = -1; a.out.copy_gate[row] = 0.f; a.out.logp[row] = 0.f; }
        return;
    }

    // ---- attention rows + SelectC's hard choice: first index of the largest alpha_c (editnet.py:409-415)
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = tid; j < T; j += TR_THREADS) {                 // ascending index per thread: `>` keeps the first
        const float v = a.alpha_c[(long long)b * T + j];
        o_ac[j] = v;
        if (v > best) { best = v; bi = j; }
    }
    if (o_av) for (int r = tid; r < R; r += TR_THREADS) o_av[r] = a.alpha_v[(long long)b * R + r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_m[wave] = best; s_i[wave] = bi; }

    // ---- copy gate (editnet.py:281): sigmoid((gate_cnew(c_new) + b) + (gate_cmem(sel) + b)), operand order of copy_gate_k
    float gsum = 0.f;
    for (int d = tid * 4; d < D; d += TR_THREADS * 4) {
        const long long off = (long long)b * D + d;
        const tr_f32x4 x = slab_sum4_at(a.gn, (long long)b * a.gn.ld + d) + *reinterpret_cast<const tr_f32x4*>(a.bn + d);
        const tr_f32x4 y = *reinterpret_cast<const tr_f32x4*>(a.cmem_pre + off) + *reinterpret_cast<const tr_f32x4*>(a.bm + d);
        tr_f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            g[e] = 1.f / (1.f + expf(-(x[e] + y[e])));
            gsum += g[e];
        }
        if (o_gf) *reinterpret_cast<tr_f32x4*>(o_gf + d) = g;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o);
    if (lane == 0) s_f[wave] = gsum;
    __syncthreads();
    if (tid == 0) {
        float bv = s_m[0];
        int bj = s_i[0];
#pragma unroll
        for (int w = 1; w < TR_WAVES; ++w)
            if (s_m[w] > bv || (s_m[w] == bv && s_i[w] < bj)) { bv = s_m[w]; bj = s_i[w]; }
        a.out.select[row] = bj == 0x7fffffff ? 0 : bj;          // (all-NaN alpha: stay in range, as select_rows_k does)
        a.out.copy_gate[row] = ((s_f[0] + s_f[1]) + (s_f[2] + s_f[3])) / (float)D;
    }
    __syncthreads();                                            // s_m / s_f are reused below

    // ---- log-sum-exp of the step's logits in one pass: running (max, sum exp(x - max)) per thread
    float m = -INFINITY, s = 0.f;
    const bool vec = !(a.logits.ld & 3) && !(a.logits.stride & 3) && ((reinterpret_cast<uintptr_t>(a.logits.p) & 15u) == 0) &&
                     (!a.fc_bias || (reinterpret_cast<uintptr_t>(a.fc_bias) & 15u) == 0);
    const int V4 = vec ? (V & ~3) : 0;
    for (int v = tid * 4; v < V4; v += TR_THREADS * 4) {
        tr_f32x4 x = slab_sum4_at(a.logits, (long long)b * a.logits.ld + v);
        if (a.fc_bias) x += *reinterpret_cast<const tr_f32x4*>(a.fc_bias + v);
        const float xm = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        if (xm > m) { s *= expf(m - xm); m = xm; }              // (m == -inf: s == 0, exp(-inf) == 0)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += expf(x[e] - m);
    }
    for (int v = V4 + tid; v < V; v += TR_THREADS) {             // last V % 4 columns (or every column when unaligned)
        const float x = tr_slab_at(a.logits, a.fc_bias, b, v);
        if (x > m) { s *= expf(m - x); m = x; }
        s += expf(x - m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o);
        const float os = __shfl_xor(s, o);
        tr_lse_merge(m, s, om, os);
    }
    if (lane == 0) { s_m[wave] = m; s_f[wave] = s; }
    __syncthreads();
    if (tid == 0) {
        float m01 = s_m[0], s01 = s_f[0], m23 = s_m[2], s23 = s_f[2];
        tr_lse_merge(m01, s01, s_m[1], s_f[1]);
        tr_lse_merge(m23, s23, s_m[3], s_f[3]);
        tr_lse_merge(m01, s01, m23, s23);
        long long tok = a.tokens[(long long)b * a.ld_tokens + t + 1];
        tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);            // clamped like every token gather (RowGather::row)
        const float x = tr_slab_at(a.logits, a.fc_bias, b, (int)tok);
        a.out.logp[row] = (x - m01) - logf(s01);
    }
}

int edit_trace_record(const EditTraceStep& a, int B, hipStream_t s) {
    if (B <= 0) return SET_OK;
    if ((a.D & 3) || a.gn.n <= 0 || a.logits.n <= 0) return SET_ERR_UNSUPPORTED;
    if (!a.out.alpha_c || !a.out.select || !a.out.copy_gate || !a.out.logp || a.t < 0 || a.t >= a.S) return SET_ERR_ARG;
    ProfScope ps("edit_trace", s, 0.0,
                 4.0 * B * ((double)a.V * a.logits.n + (double)a.D * (a.gn.n + 4.0) + 2.0 * (a.T + a.R)));
    hipLaunchKernelGGL(edit_trace_k, dim3(B), dim3(TR_THREADS), 0, s, a);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

}  // namespace set
