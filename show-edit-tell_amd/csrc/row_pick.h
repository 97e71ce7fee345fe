// The leaf pieces greedy_pick_k and gumbel_pick_k (epilogue.hip) share: the fixed-order block sum and the serial bookkeeping once
// the word is known, and the ban list of the constrained picks (PickCons).  Workgroups are 256 threads = 4 waves.  Nothing here
// owns LDS: the kernels declare it and pass it in.
#pragma once
#include "set_common.h"

namespace set {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the xor tree 32 .. 1 over the wave, lane 0 of every wave leaves its value in slot[wave], ONE barrier, then (s0 + s1) + (s2 + s3)
__device__ __forceinline__ float block_sum(float v, float* slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

// the order of beam candidates (beam.hip, beam_constrained.hip): value descending, flat index ascending among equals
__device__ __forceinline__ bool beam_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// ---- the constrained picks (set_common.h PickCons; include/set_hip.h "Constrained greedy and sampled picks"): the words REMOVED
// from row b at timestep t, as a list in LDS built the way bc_rows_k (beam_constrained.hip) builds a hypothesis's: the banned ids,
// <end> while t < min_len, and every word rule c yields from the row's own tokens s[1 .. t] = hist[0 .. t-1] (s[0] = <start> never
// takes part, so it is not stored).  Entries are words of [0, V) or -1 (matches nothing).  Block-uniform; ends with a barrier.
struct PickBanLds {
    long long seq[PC_MAXLEN + 1];              // s[0 .. L-1], L = t + 1 <= 256; seq[0] is never read
    int ban[PC_MAXBAN + 1 + PC_MAXLEN];
    int wcnt[4];
};
__device__ __forceinline__ int pick_ban_build(const PickCons& c, const long long* hist, int t, int V, long long end_idx,
                                              PickBanLds& s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = t + 1, n = c.ngram;
    if (tid >= 1 && tid < L) s.seq[tid] = hist[tid - 1];
    int nfix = c.n_banned;
    if (tid < c.n_banned) {
        const long long w = c.banned[tid];
        s.ban[tid] = (w >= 0 && w < V) ? (int)w : -1;
    }
    if (t < c.min_len) {                                 // rule b
        if (tid == 0) s.ban[nfix] = (end_idx >= 0 && end_idx < V) ? (int)end_idx : -1;
        ++nfix;
    }
    __syncthreads();
    // rule c: thread i - 1 owns position i in 1 .. L - n; the hits are compacted behind the fixed entries in position order
    bool hit = false;
    int hw = -1;
    if (n >= 1 && tid + 1 <= L - n) {
        const int i = tid + 1;
        hit = true;
        for (int q = 0; q + 1 < n; ++q) hit = hit && s.seq[i + q] == s.seq[L - n + 1 + q];
        const long long w = s.seq[i + n - 1];
        hit = hit && w >= 0 && w < V;
        hw = (int)w;
    }
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) s.wcnt[wave] = __popcll(votes);
    __syncthreads();
    int at = nfix, nban = nfix;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) at += s.wcnt[w]; nban += s.wcnt[w]; }
    if (hit) s.ban[at + __popcll(votes & ((1ull << lane) - 1ull))] = hw;
    __syncthreads();
    return nban;
}
// the register path: the thread that holds word w = ((tid + 256 q) * 4 + e) sets it to -inf (static register indices only)
__device__ __forceinline__ void pick_ban_regs(f32x4 (&x)[ROW_MAXQ], const int* ban, int nban) {
    for (int i = 0; i < nban; ++i) {
        const int w = ban[i];
        if (w >= 0 && ((w >> 2) & 255) == (int)threadIdx.x) {
            const int wq = w >> 10, we = w & 3;
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (q == wq && e == we) x[q][e] = -INFINITY;
        }
    }
}
// The scalar path of a MASKED row visits a thread's words as the register path does — quads (tid + 256 q) * 4 + e, q then e — so
// that every order-dependent sum, and the draw's enumeration, are the register path's: the outputs of a constrained pick do not
// depend on the row layout.  (A row that is not masked keeps the unconstrained kernels' order tid + 256 i and with it their bits.)
// f(v) returns true to stop.
template <class F>
__device__ __forceinline__ void pick_scalar_quads(int V, F&& f) {
    for (int q = 0; (((int)threadIdx.x + 256 * q) << 2) < V; ++q)
        for (int e = 0; e < 4; ++e) {
            const int v = (((int)threadIdx.x + 256 * q) << 2) + e;
            if (v < V && f(v)) return;
        }
}
// the scalar path: is word v on the list
__device__ __forceinline__ bool pick_banned(const int* ban, int nban, int v) {
    bool r = false;
    for (int i = 0; i < nban; ++i) r = r || ban[i] == v;
    return r;
}

// ---- the bookkeeping once the row's word is known (editnet_rl.py:529-547)
struct SampleOut {
    long long* raw_ids;   // (B) sampled word BEFORE the <end> -> 0 rewriting; -1 once the loop has been left
    float* lse;           // (B) log-sum-exp of the row (for the backward of the gathered log-prob)
    float* step_logp;     // (B) this step's log-prob (0 once the loop has been left)
    uint32_t* kept_key;   // (B) or NULL: thr of the kept set {order_key(y) >= thr} the row was drawn from (0: every word)
};

// <end> -> 0 and the `unfinished` latch: the next input word of a row that picked `pick`; unf = the row's latch after the step
__device__ __forceinline__ long long pick_latch(long long pick, long long end_idx, int t, int unf_prev, int& unf) {
    long long it = pick;
    if (it == end_idx) it = 0;
    unf = (t == 0) ? (it > 0) : (unf_prev && it > 0);
    return unf ? it : 0;
}

// ONE thread of row b.  unf_prev / alive_prev = unfinished[b] / alive[t - 1] as they stood before the step (not read at t == 0).
// Once alive[t - 1] == 0 the reference has left its loop (`break`, editnet_rl.py:546): nothing more goes to seq / seq_logp.
__device__ __forceinline__ void pick_commit(int b, int t, int max_len, long long end_idx, int pick, float logp, float lse,
                                            int unf_prev, int alive_prev, long long* seq, float* seq_logp,
                                            long long* it_buf, int* unfinished, int* alive, const SampleOut& so, long long* s_tok) {
    int unf;
    const long long it = pick_latch(pick, end_idx, t, unf_prev, unf);
    const bool broken = (t > 0) && (alive_prev == 0);
    if (t < max_len && !broken) {
        seq[(long long)b * max_len + t] = it;
        if (seq_logp) seq_logp[(long long)b * max_len + t] = logp;
    }
    if (so.raw_ids) so.raw_ids[b] = broken ? -1 : (long long)pick;
    if (so.lse) so.lse[b] = lse;
    if (so.step_logp) so.step_logp[b] = broken ? 0.f : logp;
    unfinished[b] = unf;
    if (unf) atomicAdd(&alive[t], 1);
    it_buf[b] = it;
    *s_tok = it;
}

// the NEXT step's embedding gather emb_out[b] = relu(table[tok]) (editnet.py:300-304), by the whole workgroup
__device__ __forceinline__ void pick_embed(const float* table, float* emb_out, int b, long long tok, int D) {
    for (int d = threadIdx.x * 4; d < D; d += 1024) {
        f32x4 v = *reinterpret_cast<const f32x4*>(table + tok * D + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        *reinterpret_cast<f32x4*>(emb_out + (long long)b * D + d) = v;
    }
}

}  // namespace set
