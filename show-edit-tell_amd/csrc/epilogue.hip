// Step epilogues on the vocabulary row (one workgroup per batch row, HBM/L2-bound reduction):
//   greedy (editnet_rl.py:514-543, dcnet_rl.py:313-340): log_softmax, first arg-max, <end> -> 0,
//   `unfinished` latch, seq / seqLogprobs stores, early-break emulation, and the NEXT step's
//   embedding gather relu(E[it]) (editnet.py:300-304) fused in so the loop needs no extra launch.
// The sampled and Gumbel-max picks follow.  What greedy_pick_k and gumbel_pick_k have in common — the fixed-order block sum and the
// bookkeeping after the word — is row_pick.h (sample_pick_k spells its own out: through the helpers it measured up to 2 % slower); the kernels here differ in how the word is chosen.
#include "row_pick.h"
#include "philox.h"

namespace set {

__device__ __forceinline__ float logit_at(const Slabs& s, const float* bias, long long row, int v) {
    const float* p = s.p + row * s.ld + v;
    float x = p[0];
    for (int i = 1; i < s.n; ++i) x += p[(long long)i * s.stride];
    return bias ? x + bias[v] : x;
}

// ---- LstmTail (set_common.h): the next timestep's attention-LSTM cell of this row, finished by the workgroup that chose
// the row's word.  Arithmetic and operand order are lstm_pointwise_k's (slab 0, 1, ..., pre, table row; c' = f c + i g,
// h' = o tanh c').  tail_fetch requests everything that does not depend on the word (the first two slabs, pre, c) so the
// latency sits under the logits fetch; tail_finish adds the table row and stores.
__device__ __forceinline__ float tail_sigm(float x) { return 1.f / (1.f + expf(-x)); }
struct TailRegs {
    f32x4 s0[4], s1[4], pre[4], c;
};
__device__ __forceinline__ void tail_fetch(const LstmTail& L, int b, int j, TailRegs& r) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const float* p = L.g0.p + (long long)b * L.g0.ld + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        r.s0[q] = L.g0.n > 0 ? *reinterpret_cast<const f32x4*>(p + q * L.D) : z;
        r.s1[q] = L.g0.n > 1 ? *reinterpret_cast<const f32x4*>(p + L.g0.stride + q * L.D) : z;
        r.pre[q] = L.pre ? *reinterpret_cast<const f32x4*>(L.pre + (long long)b * L.ldpre + q * L.D + j) : z;
    }
    r.c = *reinterpret_cast<const f32x4*>(L.c_in + (long long)b * L.D + j);
}
struct TailRow {
    f32x4 xt[4];
};
__device__ __forceinline__ void tail_row_fetch(const LstmTail& L, int j, const float* trow, TailRow& w) {
#pragma unroll
    for (int q = 0; q < 4; ++q) w.xt[q] = *reinterpret_cast<const f32x4*>(trow + q * L.D + j);
}
__device__ __forceinline__ void tail_finish(const LstmTail& L, int b, int j, const TailRow& w, const TailRegs& r) {
    f32x4 g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        g[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (L.g0.n > 0) g[q] += r.s0[q];
        if (L.g0.n > 1) g[q] += r.s1[q];
    }
    for (int i = 2; i < L.g0.n; i += 2) {            // the remaining partials two at a time (requested together, added in order)
        const float* p = L.g0.p + (long long)i * L.g0.stride + (long long)b * L.g0.ld + j;
        const bool two = i + 1 < L.g0.n;
        f32x4 v0[4], v1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v0[q] = *reinterpret_cast<const f32x4*>(p + q * L.D);
            if (two) v1[q] = *reinterpret_cast<const f32x4*>(p + L.g0.stride + q * L.D);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { g[q] += v0[q]; if (two) g[q] += v1[q]; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (L.pre) g[q] += r.pre[q];
        g[q] += w.xt[q];
    }
    f32x4 cn, hn;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ig = tail_sigm(g[0][e]), fg = tail_sigm(g[1][e]), gg = tanhf(g[2][e]);
        const float og = tail_sigm(g[3][e]);
        cn[e] = fg * r.c[e] + ig * gg;
        hn[e] = og * tanhf(cn[e]);
    }
    *reinterpret_cast<f32x4*>(L.c_out + (long long)b * L.D + j) = cn;
    *reinterpret_cast<f32x4*>(L.h_out + (long long)b * L.D + j) = hn;
}
__device__ __forceinline__ const float* tail_row(const LstmTail& L, long long tok) {
    tok = tok < 0 ? 0 : (tok >= L.nrows ? L.nrows - 1 : tok);       // clamped like RowGather::row
    return L.tab + tok * L.ld_tab + L.col0;
}
// the whole cell of row b for word tok, by the whole workgroup, from column j0 = 4 tid (+ 1024 when the first piece is done)
__device__ __forceinline__ void pick_tail_rows(const LstmTail& L, int b, long long tok, int j0) {
    const float* trow = tail_row(L, tok);
    for (int j = j0; j < L.D; j += 1024) {
        TailRegs r;
        TailRow w;
        tail_fetch(L, b, j, r);
        tail_row_fetch(L, j, trow, w);
        tail_finish(L, b, j, w, r);
    }
}

static bool tail_ok(const LstmTail& L) {
    return L.D > 0 && !(L.D & 3) && L.g0.p && L.g0.n >= 1 && !(L.g0.ld & 3) && !(L.g0.stride & 3) && aligned16(L.g0.p) &&
           L.tab && !(L.ld_tab & 3) && !(L.col0 & 3) && aligned16(L.tab) && L.nrows > 0 && L.c_in && L.c_out && L.h_out &&
           aligned16(L.c_in) && aligned16(L.c_out) && aligned16(L.h_out) && (!L.pre || (aligned16(L.pre) && !(L.ldpre & 3)));
}

// grid = B rows.  alive[t] counts rows still unfinished after step t (zeroed by the caller);
// once alive[t-1] == 0 the reference has left its loop (`break`, editnet_rl.py:546) and nothing
// more is written to seq / seq_logp.
// REG = true: the row (<= 4*256*ROW_MAXQ logits) is read ONCE as float4 (all K-slabs + bias summed
// in registers), max / first-argmax and sum-exp are reduced from registers.
// CONS = true: the constrained pick (set_common.h PickCons).  A live row's removed words (row_pick.h pick_ban_build) are -inf from
// the moment the row is read: arg-max, tie rule and log-sum-exp are those of the masked row; a row that has finished is read
// unmasked.  CONS = false is the kernel as it was: nothing below runs, no LDS is added.

template <bool REG, bool TAIL, bool CONS>
__global__ void SET_VGPR_CAP __launch_bounds__(256) greedy_pick_k(Slabs logits, const float* bias, int V, int t, int max_len,
                                                     long long end_idx, long long* seq, float* seq_logp,
                                                     long long* it_buf, int* unfinished, int* alive,
                                                     const float* table, float* emb_out, int D, const LstmTail tail,
                                                     const int* row_limit, const PickCons cons) {
    __shared__ PickBanLds s_cb;              // (CONS only)
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    __shared__ float s_sum[4];
    __shared__ long long s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // bookkeeping words of the serial tail (thread 0): requested now, under the row fetch, instead of as a dependent round
    // trip after the reductions.  (The loop-left test of set_common.h RowGate is NOT made here: a dependent load at the top of
    // every 10-us kernel of the chain costs more — 2 % of a single-stream decode when all seven kernels of a timestep make
    // it — than these short kernels cost after the break; the three GEMM launches and the attention launch make it.)
    int unf_prev = 1, alive_prev = 1;
    if (t > 0) {
        if (TAIL || CONS || tid == 0) unf_prev = unfinished[b];  // (TAIL: every thread derives the word right after the arg-max)
        if (tid == 0) alive_prev = alive[t - 1];
    }
    TailRegs tr;
    const bool tail0 = TAIL && tid * 4 < tail.D;
    if (TAIL) { if (tail0) tail_fetch(tail, b, tid * 4, tr); }
    int nban = 0;
    bool masked = false;                     // CONS: a live row of a launch whose constraints are not neutral
    if (CONS) {
        masked = unf_prev && (cons.ngram | cons.min_len | cons.n_banned);
        if (masked) nban = pick_ban_build(cons, seq + (long long)b * max_len, t, V, end_idx, s_cb);
    }
    float best = -INFINITY;
    int bi = 0x7fffffff;
    f32x4 x[ROW_MAXQ];
    if (REG) {
        const float* row = logits.p + (long long)b * logits.ld;
        // slab 0 (+ bias), then the remaining K-slabs in index order; ROW_MAXQ independent float4 loads
        // are in flight per pass
        const bool bias4 = bias && !(V & 3) && ((reinterpret_cast<uintptr_t>(bias) & 15u) == 0);
        // the bias does not depend on the slabs: request it first (added last, as before)
        f32x4 bq[ROW_MAXQ];
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
            bq[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (v < V) {
                if (bias4) {
                    bq[q] = *reinterpret_cast<const f32x4*>(bias + v);
                } else if (bias) {
                    bq[q][0] = bias[v];
                    if (v + 1 < V) bq[q][1] = bias[v + 1];
                    if (v + 2 < V) bq[q][2] = bias[v + 2];
                    if (v + 3 < V) bq[q][3] = bias[v + 3];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
            x[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (v < V) x[q] = *reinterpret_cast<const f32x4*>(row + v);
        }
        int i = 1;
        for (; i + 2 <= logits.n; i += 2) {          // two slabs (2 x ROW_MAXQ loads) in flight, added in slab order
            f32x4 y[ROW_MAXQ], z[ROW_MAXQ];
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) {
                const int v = (tid + 256 * q) * 4;
                y[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                z[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (v < V) {
                    y[q] = *reinterpret_cast<const f32x4*>(row + (long long)i * logits.stride + v);
                    z[q] = *reinterpret_cast<const f32x4*>(row + (long long)(i + 1) * logits.stride + v);
                }
            }
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) { x[q] += y[q]; x[q] += z[q]; }
        }
        for (; i < logits.n; ++i) {
            f32x4 y[ROW_MAXQ];
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) {
                const int v = (tid + 256 * q) * 4;
                y[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (v < V) y[q] = *reinterpret_cast<const f32x4*>(row + (long long)i * logits.stride + v);
            }
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) x[q] += y[q];
        }
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
            if (bias) x[q] += bq[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) if (v + e >= V) x[q][e] = -INFINITY;     // padding columns / rows past V
        }
        if (CONS) pick_ban_regs(x, s_cb.ban, nban);
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x[q][e] > best) { best = x[q][e]; bi = (tid + 256 * q) * 4 + e; }   // ascending index per thread
    } else {
        if (CONS && masked) {                // (row_pick.h pick_scalar_quads: the register path's order)
            pick_scalar_quads(V, [&](int v) {
                float xv = logit_at(logits, bias, b, v);
                if (pick_banned(s_cb.ban, nban, v)) xv = -INFINITY;
                if (xv > best) { best = xv; bi = v; }
                return false;
            });
        } else {
            for (int v = tid; v < V; v += 256) {
                const float xv = logit_at(logits, bias, b, v);
                if (xv > best) { best = xv; bi = v; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; }
    __syncthreads();
    best = s_val[0]; bi = s_idx[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_val[w] > best || (s_val[w] == best && s_idx[w] < bi)) { best = s_val[w]; bi = s_idx[w]; }
    if (bi == 0x7fffffff) { bi = 0; best = __builtin_nanf(""); }   // no comparison succeeded: the row is all NaN.  Word 0 and a NaN log-prob, never an out-of-range gather
    // set_decode_row_limits: row b's caption is at most row_limit[b] words long — at that timestep the loop ends it (<end> is
    // taken whatever the scores say; the recorded log-prob stays the arg-max's)
    if (row_limit && t + 1 >= row_limit[b]) bi = (int)end_idx;
    // the word follows from the arg-max and the row's latch alone: with a tail, every thread requests its piece of the
    // token-table row NOW, so that round trip runs under the sum-exp pass instead of after the serial bookkeeping
    TailRow tw;
    if (TAIL) {
        int unf;
        const long long it = pick_latch(bi, end_idx, t, unf_prev, unf);
        if (tail0) tail_row_fetch(tail, tid * 4, tail_row(tail, it), tw);
    }
    float sum = 0.f;
    if (REG) {
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += expf(x[q][e] - best);               // exp(-inf) == 0 for padding
    } else {
        if (CONS && masked) {
            pick_scalar_quads(V, [&](int v) {
                float xv = logit_at(logits, bias, b, v);
                if (pick_banned(s_cb.ban, nban, v)) xv = -INFINITY;
                sum += expf(xv - best);
                return false;
            });
        } else {
            for (int v = tid; v < V; v += 256) sum += expf(logit_at(logits, bias, b, v) - best);
        }
    }
    const float total = block_sum(sum, s_sum);
    if (tid == 0) {
        const float logp = (best - best) - logf(total);         // log_softmax at the arg-max
        pick_commit(b, t, max_len, end_idx, bi, logp, 0.f, unf_prev, alive_prev, seq, seq_logp, it_buf, unfinished, alive,
                    SampleOut{nullptr, nullptr, nullptr, nullptr}, &s_tok);
    }
    __syncthreads();
    if (emb_out && table) pick_embed(table, emb_out, b, s_tok, D);
    if (TAIL) {
        if (tail0) tail_finish(tail, b, tid * 4, tw, tr);
        pick_tail_rows(tail, b, s_tok, tid * 4 + 1024);
    }
}

// ---- host side of the three picks.  pick_args_check: the refusals they share after `B <= 0`, in their order.  SET_PICK_ROWS: one
// workgroup per row on the arguments every pick function has under these names (B, s, logits .. D), followed by the kernel's own.
// SET_PICK_DISPATCH: LAUNCH(REG, TAIL) by the row layout (pick_reg_ok) and the presence of a tail.  #undef'd after gumbel_pick.
static int pick_args_check(int D, const LstmTail* tail) {
    if (D & 3) return SET_ERR_UNSUPPORTED;
    return tail && !tail_ok(*tail) ? SET_ERR_ARG : SET_OK;
}
#define SET_PICK_ROWS(KERNEL, ...)                                                                                         \
    hipLaunchKernelGGL(KERNEL, dim3(B), dim3(256), 0, s, logits, bias, V, t, max_len, end_idx, seq, seq_logp, it, unfinished, \
                       alive, table, emb_out, D, __VA_ARGS__)
#define SET_PICK_DISPATCH(LAUNCH)                                                 \
    do {                                                                          \
        if (pick_reg_ok(logits, V)) { if (tail) LAUNCH(true, true); else LAUNCH(true, false); } \
        else { if (tail) LAUNCH(false, true); else LAUNCH(false, false); }        \
    } while (0)

int greedy_pick(Slabs logits, const float* bias, int V, int t, int max_len, long long end_idx, long long* seq,
                float* seq_logp, long long* it, int* unfinished, int* alive, const float* table, float* emb_out,
                int D, int B, hipStream_t s, const LstmTail* tail, const PickCons* cons) {
#if defined(SET_EXP_SKIP_POINTWISE) || defined(SET_EXP_SKIP_PICK)      // diagnostic build (EXPERIMENTS 5.7): the launch is dropped, results are garbage
    return SET_OK;
#endif
    if (B <= 0) return SET_OK;
    SET_TRY(pick_args_check(D, tail));
    const LstmTail tl = tail ? *tail : LstmTail();
    const PickCons pc = cons ? *cons : PickCons();
    ProfScope ps(cons ? "greedy_pick_cons" : "greedy_pick", s, 0.0,
                 4.0 * B * (2.0 * V * logits.n + 2.0 * D + (tail ? tl.D * (4.0 * (tl.g0.n + 2) + 3.0) : 0.0)));
#define SET_PICK_LAUNCH(REG, TAIL)                                                                         \
    do {                                                                                                   \
        if (cons) SET_PICK_ROWS((greedy_pick_k<REG, TAIL, true>), tl, g_row_limit, pc);                    \
        else SET_PICK_ROWS((greedy_pick_k<REG, TAIL, false>), tl, g_row_limit, pc);                        \
    } while (0)
    SET_PICK_DISPATCH(SET_PICK_LAUNCH);
#undef SET_PICK_LAUNCH
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// ---------------------------------------------------------------------------------------------
// Multinomial sampling epilogue (editnet_rl.py:521-543, dcnet_rl.py:320-340): the sampling twin of
// greedy_pick_k.  prob = exp(log_softmax(logits)); it ~ Categorical(prob); seqLogprobs = logprobs[it];
// then the same <end> -> 0 / `unfinished` latch / early-break bookkeeping and next-embedding gather.
//
// Device RNG: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), counter
// = (row, timestep, offset_lo, offset_hi), key = (seed_lo, seed_hi): one independent 24-bit uniform per
// (seed, offset, row, timestep), reproducible and independent of launch geometry.
// Draw: inverse CDF over a FIXED enumeration of the vocabulary (thread-major: thread tid owns the words
// (tid + 256 q) * 4 + e, q = 0.., e = 0..3, in that order; any fixed enumeration samples the same categorical
// distribution).  One block-wide inclusive scan of the per-thread probability mass locates the owning
// thread, which then walks its <= 48 words.  u = (r >> 8) * 2^-24 lies in [0, 1 - 2^-24], so u * total
// rounds strictly below total and exactly one thread owns the target.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned long long offset, int row, int t) {
    uint32_t c[4] = {(uint32_t)row, (uint32_t)t, (uint32_t)offset, (uint32_t)(offset >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(c[0] >> 8) * (1.0f / 16777216.0f);
}

__global__ void __launch_bounds__(64) philox_fill_k(uint32_t* out, int n, unsigned long long seed,
                                                    unsigned long long offset) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // element i -> counter (i, 0, offset): 4 words each
    if (i >= n) return;
    uint32_t c[4] = {(uint32_t)i, 0u, (uint32_t)offset, (uint32_t)(offset >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    out[4 * i] = c[0]; out[4 * i + 1] = c[1]; out[4 * i + 2] = c[2]; out[4 * i + 3] = c[3];
}

int philox_fill(uint32_t* out, int n, unsigned long long seed, unsigned long long offset, hipStream_t s) {
    if (n <= 0) return SET_OK;
    hipLaunchKernelGGL(philox_fill_k, dim3(cdiv(n, 64)), dim3(64), 0, s, out, n, seed, offset);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// ---- truncated sampling (include/set_hip.h SetSampleOpts): y = x * inv_t, then top-k, then top-p over what top-k kept.
// Both thresholds are found by a bitwise descent over the order-preserving 32-bit key of the float (at most 32 block
// reductions each: an integer count for top-k, a fixed-order mass for top-p), so the kept set {key >= thr} is exact,
// takes every tie at its boundary and does not depend on the launch.  Words outside it are masked to -inf, after which the
// draw below is the untruncated one.  (sbs.hip sbs_rows_k spells the same descent out over its own enumeration.)
struct SampleTrunc {
    float inv_t = 1.f;
    int top_k = 0;        // 0: off (the host maps top_k >= V to 0)
    float top_p = 1.f;    // 1: off
};

// CONS = true: the constrained pick, as in greedy_pick_k — the removed words of a live row are -inf before the maximum, so
// temperature, the kept set, the draw, lse and the log-prob are those of the masked row.  CONS = false: the kernel as it was.
template <bool REG, bool TAIL, bool TRUNC, bool CONS>
__global__ void __launch_bounds__(256) sample_pick_k(Slabs logits, const float* bias, int V, int t, int max_len,
                                                     long long end_idx, long long* seq, float* seq_logp,
                                                     long long* it_buf, int* unfinished, int* alive,
                                                     const float* table, float* emb_out, int D,
                                                     unsigned long long seed, unsigned long long offset,
                                                     SampleOut so, const LstmTail tail, const SampleTrunc trunc,
                                                     const PickCons cons) {
    __shared__ PickBanLds s_cb;          // (CONS only)
    __shared__ float s_red[4];
    __shared__ int s_cnt[2][4];          // TRUNC: per-wave partials of one descent pass, double-buffered (one barrier a pass)
    __shared__ float s_mass[2][4];
    __shared__ float s_scan[4];
    __shared__ float s_max;
    __shared__ long long s_tok;
    __shared__ int s_pick;
    __shared__ float s_pick_x;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    f32x4 x[ROW_MAXQ];
    float best = -INFINITY;
    uint32_t thr = 0;                                    // TRUNC: the kept set is {order_key(y) >= thr}
    int nban = 0;
    bool masked = false;                                 // CONS: a live row of a launch whose constraints are not neutral
    if (CONS) {
        masked = (t == 0 || unfinished[b]) && (cons.ngram | cons.min_len | cons.n_banned);
        if (masked) nban = pick_ban_build(cons, seq + (long long)b * max_len, t, V, end_idx, s_cb);
    }
    // the generic path's logit, re-read (CONS: -inf when removed; TRUNC: scaled, and -inf outside the kept set once thr stands)
    auto val = [&](int v) -> float {
        float xv = logit_at(logits, bias, b, v);
        if (CONS) { if (pick_banned(s_cb.ban, nban, v)) xv = -INFINITY; }
        if (TRUNC) {
            xv *= trunc.inv_t;
            if (order_key(xv) < thr) xv = -INFINITY;
        }
        return xv;
    };
    if (REG) {
        const float* row = logits.p + (long long)b * logits.ld;
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
            x[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (v < V) x[q] = *reinterpret_cast<const f32x4*>(row + v);
        }
        for (int i = 1; i < logits.n; ++i) {             // K-slabs in index order, as greedy_pick_k
            f32x4 y[ROW_MAXQ];
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) {
                const int v = (tid + 256 * q) * 4;
                y[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (v < V) y[q] = *reinterpret_cast<const f32x4*>(row + (long long)i * logits.stride + v);
            }
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) x[q] += y[q];
        }
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (v + e < V) { if (bias) x[q][e] += bias[v + e]; if (TRUNC) x[q][e] *= trunc.inv_t; }
                else x[q][e] = -INFINITY;
                best = fmaxf(best, x[q][e]);
            }
        }
        if (CONS) {                                      // the maximum of the masked row
            pick_ban_regs(x, s_cb.ban, nban);
            best = -INFINITY;
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) best = fmaxf(best, x[q][e]);
        }
    } else {
        for (int v = tid; v < V; v += 256) best = fmaxf(best, val(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o));
    if (lane == 0) s_red[wave] = best;
    if (tid == 0) s_pick = -1;
    __syncthreads();
    best = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    if (TRUNC && (trunc.top_k > 0 || trunc.top_p < 1.f)) {
        // Every pass is block-uniform: each wave leaves one partial in LDS, one barrier, every thread adds the four in the
        // same order.  Padding columns (-inf) never change a decision: they lie below every threshold that matters.
        uint32_t key[ROW_MAXQ][4];
        if (REG) {
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) key[q][e] = order_key(x[q][e]);
        }
        int pass = 0;
        uint32_t lo = 0;
        if (trunc.top_k > 0) {           // lo = key of the top_k-th largest value: the largest lo with |{key >= lo}| >= top_k
            for (int bit = 31; bit >= 0; --bit, ++pass) {
                const uint32_t cand = lo | (1u << bit);
                int c = 0;               // wave-uniform
                if (REG) {
#pragma unroll
                    for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) c += __popcll(__ballot(key[q][e] >= cand));
                } else {
                    for (int v0 = 0; v0 < V; v0 += 256) {
                        const int v = v0 + tid;
                        c += __popcll(__ballot(v < V && order_key(val(v)) >= cand));
                    }
                }
                if (lane == 0) s_cnt[pass & 1][wave] = c;
                __syncthreads();
                const int* sc = s_cnt[pass & 1];
                if ((sc[0] + sc[1]) + (sc[2] + sc[3]) >= trunc.top_k) lo = cand;
            }
            thr = lo;                    // (the generic path's val() masks with it from here on)
        }
        if (trunc.top_p < 1.f) {
            // mass of {kept by top-k, key >= cand}: per thread in enumeration order, xor tree over the wave, waves in index
            // order — one fixed order for every cand, so the sum of these non-negative terms is monotone in cand
            float m[ROW_MAXQ][4];
            if (REG) {
#pragma unroll
                for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) m[q][e] = key[q][e] >= lo ? expf(x[q][e] - best) : 0.f;
            }
            auto mass_ge = [&](uint32_t cand) -> float {
                float sm = 0.f;
                if (REG) {
#pragma unroll
                    for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) sm += key[q][e] >= cand ? m[q][e] : 0.f;
                } else if (CONS && masked) {             // (row_pick.h pick_scalar_quads: the register path's order)
                    pick_scalar_quads(V, [&](int v) {
                        const float yv = val(v);
                        sm += order_key(yv) >= cand ? expf(yv - best) : 0.f;
                        return false;
                    });
                } else {
                    for (int v = tid; v < V; v += 256) {
                        const float yv = val(v);
                        sm += order_key(yv) >= cand ? expf(yv - best) : 0.f;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
                if (lane == 0) s_mass[pass & 1][wave] = sm;
                __syncthreads();
                const float* sp = s_mass[pass & 1];
                ++pass;
                return (sp[0] + sp[1]) + (sp[2] + sp[3]);
            };
            const float need = trunc.top_p * mass_ge(lo);
            uint32_t hi = 0;             // the largest hi with mass_ge(hi) >= need; hi >= lo as mass_ge(lo) >= need
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = hi | (1u << bit);
                if (mass_ge(cand) >= need) hi = cand;
            }
            thr = hi;
        }
        const uint32_t kbest = order_key(best);
        if (thr > kbest) thr = kbest;    // the arg-max is always kept
        if (REG) {
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) if (key[q][e] < thr) x[q][e] = -INFINITY;
        }
    }
    // per-thread probability mass (unnormalised), then inclusive scan over the threads
    float mass = 0.f;
    if (REG) {
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) mass += expf(x[q][e] - best);                  // exp(-inf) == 0
    } else if (CONS && masked) {
        pick_scalar_quads(V, [&](int v) { mass += expf(val(v) - best); return false; });
    } else {
        for (int v = tid; v < V; v += 256) mass += expf(val(v) - best);
    }
    float incl = mass;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_scan[wave] = incl;
    __syncthreads();
    float wave_base = 0.f;
#pragma unroll
    for (int w = 0; w < 3; ++w) if (w < wave) wave_base += s_scan[w];
    incl += wave_base;
    const float total = ((s_scan[0] + s_scan[1]) + s_scan[2]) + s_scan[3];
    const float target = sample_uniform(seed, offset, b, t) * total;
    // the owner is the first thread whose inclusive mass exceeds the target (monotone scan; `excl` of a thread
    // is recomputed from its own incl, so neighbours may disagree by an ulp: ownership is decided on incl only)
    float prev_incl = __shfl_up(incl, 1);
    if (lane == 0) prev_incl = wave_base;
    const bool owner = (target < incl) && !(target < prev_incl);
    if (owner) {
        float c = prev_incl;
        int pick = -1;
        float pick_x = 0.f;
        if (REG) {
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = expf(x[q][e] - best);
                    c += pe;
                    if (pick < 0 && pe > 0.f && target < c) { pick = (tid + 256 * q) * 4 + e; pick_x = x[q][e]; }
                }
            if (pick < 0) {                      // rounding left the target at the very end of this thread's span
#pragma unroll
                for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x[q][e] > -INFINITY && expf(x[q][e] - best) > 0.f) { pick = (tid + 256 * q) * 4 + e; pick_x = x[q][e]; }
            }
        } else {
            int last = -1;
            float last_x = 0.f;
            if (CONS && masked) {
                pick_scalar_quads(V, [&](int v) {
                    const float xv = val(v);
                    const float pe = expf(xv - best);
                    if (pe > 0.f) { last = v; last_x = xv; }
                    c += pe;
                    if (pe > 0.f && target < c) { pick = v; pick_x = xv; return true; }
                    return false;
                });
            } else {
                for (int v = tid; v < V; v += 256) {
                    const float xv = val(v);
                    const float pe = expf(xv - best);
                    if (pe > 0.f) { last = v; last_x = xv; }
                    c += pe;
                    if (pe > 0.f && target < c) { pick = v; pick_x = xv; break; }
                }
            }
            if (pick < 0) { pick = last; pick_x = last_x; }
        }
        s_pick = pick;
        s_pick_x = pick_x;
    }
    __syncthreads();
    if (tid == 0) {
        int pick = s_pick;
        float px = s_pick_x;
        if (pick < 0) {                          // cannot happen for finite logits; keep the row well defined
            pick = 0;
            px = REG ? best : val(0);
        }
        const float lse = best + logf(total);
        const float logp = (px - best) - logf(total);
        long long it = pick;
        if (it == end_idx) it = 0;
        int unf = (t == 0) ? (it > 0) : (unfinished[b] && it > 0);
        it = unf ? it : 0;
        const bool broken = (t > 0) && (alive[t - 1] == 0);
        if (t < max_len && !broken) {
            seq[(long long)b * max_len + t] = it;
            if (seq_logp) seq_logp[(long long)b * max_len + t] = logp;
        }
        if (so.raw_ids) so.raw_ids[b] = broken ? -1 : (long long)pick;
        if (so.lse) so.lse[b] = lse;
        if (so.step_logp) so.step_logp[b] = broken ? 0.f : logp;
        if (so.kept_key) so.kept_key[b] = thr;
        unfinished[b] = unf;
        if (unf) atomicAdd(&alive[t], 1);
        it_buf[b] = it;
        s_tok = it;
    }
    __syncthreads();
    if (emb_out && table) {
        const long long tok = s_tok;
        for (int d = tid * 4; d < D; d += 1024) {
            f32x4 v = *reinterpret_cast<const f32x4*>(table + tok * D + d);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
            *reinterpret_cast<f32x4*>(emb_out + (long long)b * D + d) = v;
        }
    }
    if (TAIL) {
        const float* trow = tail_row(tail, s_tok);
        for (int j = tid * 4; j < tail.D; j += 1024) {
            TailRegs r2;
            TailRow w2;
            tail_fetch(tail, b, j, r2);
            tail_row_fetch(tail, j, trow, w2);
            tail_finish(tail, b, j, w2, r2);
        }
    }
}

int sample_pick(Slabs logits, const float* bias, int V, int t, int max_len, long long end_idx, long long* seq,
                float* seq_logp, long long* it, int* unfinished, int* alive, const float* table, float* emb_out, int D,
                int B, unsigned long long seed, unsigned long long offset, long long* raw_ids, float* lse,
                float* step_logp, hipStream_t s, const LstmTail* tail, const SetSampleOpts* opts, uint32_t* kept_key,
                const PickCons* cons) {
    if (B <= 0) return SET_OK;
    SET_TRY(pick_args_check(D, tail));
    if (sample_opts_check(opts) != SET_OK) return SET_ERR_ARG;
    const LstmTail tl = tail ? *tail : LstmTail();
    SampleTrunc tc;
    if (opts) {
        tc.inv_t = 1.0f / opts->temperature;
        tc.top_k = opts->top_k >= V ? 0 : opts->top_k;
        tc.top_p = opts->top_p;
    }
    // nothing to scale and nothing to cut: the untruncated instantiation, as before there were options
    const bool trunc = tc.inv_t != 1.f || tc.top_k > 0 || tc.top_p < 1.f;
    const PickCons pc = cons ? *cons : PickCons();
    static const char* const scope[2][2] = {{"sample_pick", "sample_pick_trunc"}, {"sample_pick_cons", "sample_pick_trunc_cons"}};
    ProfScope ps(scope[cons != nullptr][trunc], s, 0.0,
                 4.0 * B * (1.0 * V * logits.n + 2.0 * D + (tail ? tl.D * (4.0 * (tl.g0.n + 2) + 3.0) : 0.0)));
    SampleOut so{raw_ids, lse, step_logp, kept_key};
#define SET_PICK_LAUNCH(REG, TAIL)                                                                         \
    do {                                                                                                   \
        if (cons) {                                                                                        \
            if (trunc) SET_PICK_ROWS((sample_pick_k<REG, TAIL, true, true>), seed, offset, so, tl, tc, pc);    \
            else SET_PICK_ROWS((sample_pick_k<REG, TAIL, false, true>), seed, offset, so, tl, tc, pc);         \
        } else if (trunc) SET_PICK_ROWS((sample_pick_k<REG, TAIL, true, false>), seed, offset, so, tl, tc, pc); \
        else SET_PICK_ROWS((sample_pick_k<REG, TAIL, false, false>), seed, offset, so, tl, tc, pc);        \
    } while (0)
    SET_PICK_DISPATCH(SET_PICK_LAUNCH);
#undef SET_PICK_LAUNCH
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// ---------------------------------------------------------------------------------------------
// Gumbel-max pick (include/set_hip.h "Gumbel-max draw"): the word of row b at timestep t is the FIRST maximum of
// s[v] = y[v] + g[v], y = (logits + bias) * inv_t, g = the noise of philox.h keyed by (seed, offset, b, t, v) — exactly a draw
// from softmax(y), and an arg-max, so it does not depend on how the vocabulary is cut over threads or workgroups: the
// persistent launch (decode_persistent_wide.hip, SAMPLE) draws the same word from the same seed.  step_logp / lse are over
// the unperturbed y, as in the untruncated sampled pick; the bookkeeping after the draw is row_pick.h's.
// One workgroup per row; a thread owns whole quads of the vocabulary (one Philox call serves four words).
// ---------------------------------------------------------------------------------------------
template <bool REG, bool TAIL>
__global__ void __launch_bounds__(256) gumbel_pick_k(Slabs logits, const float* bias, int V, int t, int max_len,
                                                     long long end_idx, long long* seq, float* seq_logp,
                                                     long long* it_buf, int* unfinished, int* alive,
                                                     const float* table, float* emb_out, int D,
                                                     unsigned long long seed, unsigned long long offset,
                                                     SampleOut so, const LstmTail tail, float inv_t) {
    __shared__ float s_my[4], s_bs[4], s_by[4], s_sum[4];
    __shared__ int s_bi[4];
    __shared__ long long s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    f32x4 x[ROW_MAXQ];
    float my = -INFINITY;                    // max y
    float bs = -INFINITY, by = 0.f;          // max s, y at its first arg-max
    int bi = 0x7fffffff;
    // one quad: y of its words (-inf past V), the running max y and (max s, first arg-max, y there) in ascending word order
    auto quad = [&](int j, f32x4& y) {
        uint32_t c[4];
        gumbel_quad_words(seed, offset, b, t, j, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 4 * j + e;
            if (v < V) {
                const float s = y[e] + gumbel_of_word(c[e]);
                my = fmaxf(my, y[e]);
                if (s > bs) { bs = s; bi = v; by = y[e]; }
            } else {
                y[e] = -INFINITY;
            }
        }
    };
    if (REG) {
        const float* row = logits.p + (long long)b * logits.ld;
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
            x[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (v < V) x[q] = *reinterpret_cast<const f32x4*>(row + v);
        }
        for (int i = 1; i < logits.n; ++i) {             // K-slabs in index order, as sample_pick_k
            f32x4 y[ROW_MAXQ];
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) {
                const int v = (tid + 256 * q) * 4;
                y[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (v < V) y[q] = *reinterpret_cast<const f32x4*>(row + (long long)i * logits.stride + v);
            }
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q) x[q] += y[q];
        }
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v + e < V) { if (bias) x[q][e] += bias[v + e]; x[q][e] = __fmul_rn(x[q][e], inv_t); }   // (rounded: never an fma with the noise)
            if (v < V) quad(tid + 256 * q, x[q]);
            else x[q] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
    } else {
        for (int j = tid; 4 * j < V; j += 256) {
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = 4 * j + e < V ? __fmul_rn(logit_at(logits, bias, b, 4 * j + e), inv_t) : -INFINITY;
            quad(j, y);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        my = fmaxf(my, __shfl_xor(my, o));
        const float os = __shfl_xor(bs, o), oy = __shfl_xor(by, o);
        const int oi = __shfl_xor(bi, o);
        if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; by = oy; }
    }
    if (lane == 0) { s_my[wave] = my; s_bs[wave] = bs; s_bi[wave] = bi; s_by[wave] = by; }
    __syncthreads();
    my = fmaxf(fmaxf(s_my[0], s_my[1]), fmaxf(s_my[2], s_my[3]));
    bs = s_bs[0]; bi = s_bi[0]; by = s_by[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_bs[w] > bs || (s_bs[w] == bs && s_bi[w] < bi)) { bs = s_bs[w]; bi = s_bi[w]; by = s_by[w]; }
    float sum = 0.f;
    if (REG) {
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += expf(x[q][e] - my);                    // exp(-inf) == 0 past V
    } else {
        for (int v = tid; v < V; v += 256) sum += expf(__fmul_rn(logit_at(logits, bias, b, v), inv_t) - my);
    }
    const float total = block_sum(sum, s_sum);
    if (tid == 0) {
        const float lse = my + logf(total);
        float logp = (by - my) - logf(total);
        int pick = bi;
        if (pick == 0x7fffffff) { pick = 0; logp = __builtin_nanf(""); }       // no comparison succeeded: the row is all NaN
        pick_commit(b, t, max_len, end_idx, pick, logp, lse, t > 0 ? unfinished[b] : 1, t > 0 ? alive[t - 1] : 1, seq,
                    seq_logp, it_buf, unfinished, alive, so, &s_tok);
    }
    __syncthreads();
    if (emb_out && table) pick_embed(table, emb_out, b, s_tok, D);
    if (TAIL) pick_tail_rows(tail, b, s_tok, tid * 4);
}

int pick_cons_check(const SetBeamConstraints* c, int V, int max_len, PickCons* out) {
    if (!c) return SET_ERR_ARG;
    if (c->no_repeat_ngram < 0 || c->no_repeat_ngram > PC_MAXNGRAM || c->min_len < 0) return SET_ERR_ARG;
    if (!(c->length_alpha == 0.f)) return SET_ERR_ARG;                                  // nothing is ranked here (NaN refused too)
    if (c->n_banned < 0 || c->n_banned > PC_MAXBAN || (c->n_banned == 0) != (c->banned == nullptr)) return SET_ERR_ARG;
    if (max_len > PC_MAXLEN) return SET_ERR_ARG;                                        // the row's history lives in LDS
    if ((long long)V <= (long long)c->n_banned + 1 + max_len) return SET_ERR_ARG;       // by counting, every row keeps a word
    out->ngram = c->no_repeat_ngram; out->min_len = c->min_len; out->n_banned = c->n_banned;
    out->banned = (const long long*)c->banned;
    return SET_OK;
}

int gumbel_opts_check(const SetSampleOpts* opts, int V, int max_len) {
    if (sample_opts_check(opts) != SET_OK) return SET_ERR_ARG;
    if (opts && (opts->top_k != 0 || opts->top_p != 1.f)) return SET_ERR_ARG;       // the arg-max draw has no truncation
    if (max_len > GUMBEL_MAX_LEN || V > GUMBEL_MAX_V) return SET_ERR_ARG;            // the noise counters (philox.h)
    return SET_OK;
}

int gumbel_pick(Slabs logits, const float* bias, int V, int t, int max_len, long long end_idx, long long* seq,
                float* seq_logp, long long* it, int* unfinished, int* alive, const float* table, float* emb_out, int D,
                int B, unsigned long long seed, unsigned long long offset, long long* raw_ids, float* lse,
                float* step_logp, hipStream_t s, const LstmTail* tail, const SetSampleOpts* opts) {
    if (gumbel_opts_check(opts, V, max_len) != SET_OK || t > GUMBEL_MAX_LEN) return SET_ERR_ARG;
    if (B <= 0) return SET_OK;
    SET_TRY(pick_args_check(D, tail));
    const LstmTail tl = tail ? *tail : LstmTail();
    const float inv_t = opts ? 1.0f / opts->temperature : 1.f;
    ProfScope ps("gumbel_pick", s, 0.0,
                 4.0 * B * (1.0 * V * logits.n + 2.0 * D + (tail ? tl.D * (4.0 * (tl.g0.n + 2) + 3.0) : 0.0)));
    SampleOut so{raw_ids, lse, step_logp, nullptr};
#define SET_PICK_LAUNCH(REG, TAIL) SET_PICK_ROWS((gumbel_pick_k<REG, TAIL>), seed, offset, so, tl, inv_t)
    SET_PICK_DISPATCH(SET_PICK_LAUNCH);
#undef SET_PICK_LAUNCH
    SET_LAUNCH_CHECK();
    return SET_OK;
}

#undef SET_PICK_DISPATCH
#undef SET_PICK_ROWS

// out (rows, V) = the noise g of (seed, offset, row, t, v): the test hook of the definition in philox.h
__global__ void __launch_bounds__(256) gumbel_fill_k(float* out, int rows, int V, int t, unsigned long long seed,
                                                     unsigned long long offset) {
    const int nq = (V + 3) >> 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // (row, quad)
    if (i >= (long long)rows * nq) return;
    const int row = (int)(i / nq), j = (int)(i % nq);
    uint32_t c[4];
    gumbel_quad_words(seed, offset, row, t, j, c);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * j + e < V) out[(long long)row * V + 4 * j + e] = gumbel_of_word(c[e]);
}

int gumbel_fill(float* out, int rows, int V, int t, unsigned long long seed, unsigned long long offset, hipStream_t s) {
    const long long n = (long long)rows * ((V + 3) >> 2);
    hipLaunchKernelGGL(gumbel_fill_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, rows, V, t, seed, offset);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// d logits[b, v] = g[b] * (1[v == id_b] - softmax(logits[b])[v])   (gradient of the gathered log-softmax;
// rows with id < 0 — steps after the loop was left — get zeros)
__global__ void __launch_bounds__(256) sample_logp_bwd_k(const float* logits, long long ld, const float* lse,
                                                         const long long* ids, const float* g, float* dlogits,
                                                         long long ldd, int V) {
    const int b = blockIdx.x;
    const long long id = ids[b];
    const float gb = g[b], l = lse[b];
    for (int v = threadIdx.x; v < V; v += 256) {
        float d = 0.f;
        if (id >= 0) d = gb * ((v == id ? 1.f : 0.f) - expf(logits[(long long)b * ld + v] - l));
        dlogits[(long long)b * ldd + v] = d;
    }
}

int sample_logp_bwd(const float* logits, long long ld, const float* lse, const long long* ids, const float* g,
                    float* dlogits, long long ldd, int B, int V, hipStream_t s) {
    if (B <= 0) return SET_OK;
    hipLaunchKernelGGL(sample_logp_bwd_k, dim3(B), dim3(256), 0, s, logits, ld, lse, ids, g, dlogits, ldd, V);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// The same gradient under SetSampleOpts, over any number of rows (the sequence nodes: all T * B rows of a rollout at once):
//   d logits[r, v] = g[r] * inv_t * (1[v == id_r] - (order_key(y) >= key_r ? exp(y - lse_r) : 0)),   y = fl32(logits[r, v] * inv_t)
// key_r is the threshold sample_pick_k left in SampleOut::kept_key (NULL: 0, every word kept); the kept set is piecewise constant
// in the logits and is held constant.  y is the rounded product the forward compared (no fma with the subtraction of lse), so
// the set is the forward's bit for bit; with inv_t == 1 and key 0 the values are sample_logp_bwd_k's.  One workgroup per row;
// VEC: rows read and written as float4 (ld, ldd multiples of 4, bases 16-byte aligned), the V % 4 tail by scalar accesses —
// columns V .. ldd-1 are never written.
template <bool VEC>
__global__ void __launch_bounds__(256) sample_logp_bwd_opts_k(const float* logits, long long ld, const float* lse,
                                                              const long long* ids, const uint32_t* kept_key, const float* g,
                                                              float* dlogits, long long ldd, int V, float inv_t) {
    const long long r = blockIdx.x;
    const int tid = threadIdx.x;
    const long long id = ids[r];
    const float gb = g[r] * inv_t, l = lse[r];
    const uint32_t thr = kept_key ? kept_key[r] : 0u;
    const float* x = logits + r * ld;
    float* d = dlogits + r * ldd;
    auto grad = [&](float xv, int v) -> float {
        if (id < 0) return 0.f;
        const float y = __fmul_rn(xv, inv_t);
        const float p = order_key(y) >= thr ? expf(y - l) : 0.f;
        return gb * ((v == id ? 1.f : 0.f) - p);
    };
    if (VEC) {
        const int V4 = V & ~3;
        for (int v = tid * 4; v < V4; v += 1024) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + v);
            f32x4 dv;
#pragma unroll
            for (int e = 0; e < 4; ++e) dv[e] = grad(xv[e], v + e);
            *reinterpret_cast<f32x4*>(d + v) = dv;
        }
        if (V4 + tid < V) d[V4 + tid] = grad(x[V4 + tid], V4 + tid);
    } else {
        for (int v = tid; v < V; v += 256) d[v] = grad(x[v], v);
    }
}

int sample_logp_bwd_opts(const float* logits, long long ld, const float* lse, const long long* ids, const uint32_t* kept_key,
                         const float* g, float* dlogits, long long ldd, int rows, int V, const SetSampleOpts* opts,
                         hipStream_t s) {
    if (rows <= 0) return SET_OK;
    if (sample_opts_check(opts) != SET_OK) return SET_ERR_ARG;
    const float inv_t = opts ? 1.0f / opts->temperature : 1.f;
    ProfScope ps("sample_logp_bwd_opts", s, 0.0, 8.0 * rows * V);
    const bool vec = !(ld & 3) && !(ldd & 3) && aligned16(logits) && aligned16(dlogits);
    if (vec)
        hipLaunchKernelGGL(sample_logp_bwd_opts_k<true>, dim3(rows), dim3(256), 0, s, logits, ld, lse, ids, kept_key, g, dlogits,
                           ldd, V, inv_t);
    else
        hipLaunchKernelGGL(sample_logp_bwd_opts_k<false>, dim3(rows), dim3(256), 0, s, logits, ld, lse, ids, kept_key, g, dlogits,
                           ldd, V, inv_t);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// it[:] = value; unfinished[:] = 1; alive[0..n_alive) = 0
__global__ void __launch_bounds__(256) set_tokens_k(long long* it, long long value, int* unfinished, int* alive,
                                                    int n_alive, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { it[i] = value; unfinished[i] = 1; }
    if (i < n_alive) alive[i] = 0;
}

int set_tokens(long long* it, long long value, int* unfinished, int* alive, int n_alive, int B, hipStream_t s) {
    const int n = B > n_alive ? B : n_alive;
    hipLaunchKernelGGL(set_tokens_k, dim3(cdiv(n, 256)), dim3(256), 0, s, it, value, unfinished, alive, n_alive, B);
    SET_LAUNCH_CHECK();
    return SET_OK;
}


__global__ void __launch_bounds__(256) iota_i64_k(long long* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}

int iota_i64(long long* p, int n, hipStream_t s) {
    hipLaunchKernelGGL(iota_i64_k, dim3(cdiv(n, 256)), dim3(256), 0, s, p, n);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

}  // namespace set
