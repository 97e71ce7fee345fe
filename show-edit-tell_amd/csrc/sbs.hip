// Stochastic beam search (Kool, van Hoof, Welling, "Stochastic Beams and Where to Find Them", ICML 2019): the pick of one
// timestep for NI images x k slots (include/set_hip.h "Stochastic beam search pick").  The k slots of an image end up holding
// k DISTINCT prefixes that are an exact sample without replacement from the model's sequence distribution, in draw order.
//
// Two launches:
//   sbs_rows_k    one workgroup per (image, slot) row — the V-sized work: the row read, log-sum-exp of y, the Gumbel noise of
//                 philox.h, g[v] = phi'[v] + noise, and the row's k best (g, v) with phi' there.  The conditioned score g~ is
//                 increasing in g for a fixed parent, so a parent can only place its own k best g among the image's k picks:
//                 the transform is applied to k values per parent, never to V.
//   sbs_merge_k   one wave per image: the transform of the k x k candidates, finished slots as one candidate each, the flat
//                 top-k (ties: lowest flat index j V + v), and the bookkeeping.
// Both row-read paths (float4 into registers / scalar re-reads) give every thread the same quads in the same order and
// feed one set of lambdas, so the outputs do not depend on the path.  No floating-point atomics, no scratch.
//
// The two-model pick (set_sbs_pick_ensemble_f32, the EditNet + DCNet ensemble) is sbs_rows_k<.., 2>: a second logits row per
// slot, both tempered and normalised on their own, the word's log-probability that of the averaged distributions.  The merge
// sees only candidates and is shared.  The register path HOLDS BOTH ROWS (2 x 12 float4 per thread): no scratch on gfx950, and
// one workgroup per row leaves at most one workgroup per CU, so the registers cost no occupancy that a launch of <= 128 rows
// could use; re-reading the second row was therefore not needed.
//
// Truncation (set_sbs_pick_opts_f32 / set_sbs_pick_ensemble_opts_f32, sbs_rows_k<.., .., true>): top-k and top-p cut the WORD
// distribution of every step to a kept set S, by the rules and the bitwise descent of sample_pick_k (epilogue.hip), and the log-
// sum-exp is taken over S: phi is the log-probability under the truncated, renormalised model, of which the search is then the
// exact sample without replacement.  One model: S on y.  Two models: S on l, the log of the averaged distributions.  The noise,
// the candidates' selection and the merge are untouched.
#include "set_common.h"
#include "philox.h"

namespace set {

typedef float sbs_f32x4 __attribute__((ext_vector_type(4)));
constexpr int SBS_KMAX = 8;
constexpr int SBS_NONE = 0x7fffffff;

struct SbsRowArgs {
    const float* logits; const float* logits2; long long ld;     // logits2: the second model's rows (NM == 2), same V and ld
    int k, V, t;
    float inv_t;
    unsigned long long seed, offset;
    const float* phi; const float* G; const int* fin; const int* n_open;
    float* cand_g; float* cand_phi; int* cand_v;         // (NI * k, SBS_KMAX)
};

// top_k / top_p of a truncated pick.  A kernel argument of its own: SbsRowArgs, and with it every argument offset of the untruncated
// instantiations, stays as it was.
struct SbsTrunc {
    int top_k;                                   // 0: off (the host maps top_k >= V to 0)
    float top_p;                                 // 1: off
};

// log(0.5 (exp(p) + exp(q))) = hi + log1p(exp(lo - hi)) - ln 2 with hi / lo the larger / smaller of the two; one -inf term gives
// hi - ln 2, two give -inf (the word is no candidate)
__device__ __forceinline__ float sbs_mean_logp(float p, float q) {
    const float hi = fmaxf(p, q), lo = fminf(p, q);
    return hi > -INFINITY ? (hi + log1pf(expf(lo - hi))) - 0.69314718f : -INFINITY;
}

// NM models per row: 1 = log_softmax(y); 2 = log(0.5 (softmax(y_e) + softmax(y_d))), each model tempered before the average.
// TRUNC: the row's kept set S = {order_key(z) >= thr} is found on z = y (NM == 1) or z = l (NM == 2), words outside S are
// never candidates and the log-sum-exp runs over S; at least one of tr.top_k / tr.top_p is on (the host launches the untruncated
// instantiation otherwise).
template <bool REG, int NM, bool TRUNC>
__global__ void __launch_bounds__(256) sbs_rows_k(const SbsRowArgs a, const SbsTrunc tr) {
    __shared__ float s_red[NM][4];
    __shared__ int s_cnt[2][4];          // TRUNC: per-wave partials of one descent pass, double-buffered (one barrier a pass)
    __shared__ float s_mass[2][4];
    __shared__ float s_zmax[4];          // TRUNC, NM == 2: the waves' maxima of l
    __shared__ float s_bv[2][4];
    __shared__ int s_bi[2][4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V;
    const float Gj = a.G[r], phij = a.phi[r];
    // a dead slot, a finished slot (one candidate: itself) and every slot of a closed image offer no words: nothing is read
    if (Gj == -INFINITY || a.fin[r] != 0 || a.n_open[r / a.k] == 0) return;
    const float* row = a.logits + (long long)r * a.ld;
    const float* row2 = NM == 2 ? a.logits2 + (long long)r * a.ld : row;
    sbs_f32x4 x[ROW_MAXQ], x2[NM == 2 ? ROW_MAXQ : 1];
    uint32_t thr = 0;                                    // TRUNC: S = {order_key(z) >= thr}; 0 until the descent has run
    if (REG) {
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
            x[q] = (sbs_f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (NM == 2) x2[NM == 2 ? q : 0] = x[q];
            if (v < V) {
                const sbs_f32x4 w = *reinterpret_cast<const sbs_f32x4*>(row + v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v + e < V) x[q][e] = __fmul_rn(w[e], a.inv_t);
                if (NM == 2) {
                    const sbs_f32x4 w2 = *reinterpret_cast<const sbs_f32x4*>(row2 + v);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (v + e < V) x2[NM == 2 ? q : 0][e] = __fmul_rn(w2[e], a.inv_t);
                }
            }
        }
    }
    // every thread visits its quads tid, tid + 256, ... in that order on either path, both models' quads of a visit together
    // (NM == 1: the one row twice); words past V are -inf.  TRUNC, one model: words outside S are -inf once thr stands (the
    // registers are cut in place, the scalar reads are masked here)
    auto sweep = [&](auto&& f) {
        if (REG) {
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
                if ((tid + 256 * q) * 4 < V) f(tid + 256 * q, x[q], NM == 2 ? x2[NM == 2 ? q : 0] : x[q]);
        } else {
            for (int j = tid; 4 * j < V; j += 256) {
                sbs_f32x4 y, y2;
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = 4 * j + e < V ? __fmul_rn(row[4 * j + e], a.inv_t) : -INFINITY;
                if (TRUNC && NM == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (order_key(y[e]) < thr) y[e] = -INFINITY;
                }
                if (NM == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) y2[e] = 4 * j + e < V ? __fmul_rn(row2[4 * j + e], a.inv_t) : -INFINITY;
                }
                f(j, y, NM == 2 ? y2 : y);
            }
        }
    };
    // per model: max, sum of exp and log-sum-exp, each formed as the one-model pick forms its own
    float my[NM], sum[NM], lse[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) { my[m] = -INFINITY; sum[m] = 0.f; }
    auto max4 = [](const sbs_f32x4& y) { return fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])); };
    sweep([&](int, const sbs_f32x4& y, const sbs_f32x4& y2) {
        my[0] = fmaxf(my[0], max4(y));
        if (NM == 2) my[NM - 1] = fmaxf(my[NM - 1], max4(y2));
    });
#pragma unroll
    for (int m = 0; m < NM; ++m) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) my[m] = fmaxf(my[m], __shfl_xor(my[m], o));
        if (lane == 0) s_red[m][wave] = my[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NM; ++m) my[m] = fmaxf(fmaxf(s_red[m][0], s_red[m][1]), fmaxf(s_red[m][2], s_red[m][3]));
    __syncthreads();
    // TRUNC, scalar path: quad j of z as the sweeps form it, uncut (NM == 2: lse stands by the time this is called); no read past V
    auto zquad = [&](int j) -> sbs_f32x4 {
        sbs_f32x4 z;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 4 * j + e;
            z[e] = v < V ? __fmul_rn(row[v], a.inv_t) : -INFINITY;
            if (NM == 2) z[e] = sbs_mean_logp(z[e] - lse[0], (v < V ? __fmul_rn(row2[v], a.inv_t) : -INFINITY) - lse[NM - 1]);
        }
        return z;
    };
    // TRUNC: thr of the kept set of z with maximum `best`, sample_pick_k's descent (epilogue.hip): every pass is block-uniform,
    // each wave leaves one partial in LDS, one barrier, every thread adds the four in the same order.  Padding (-inf) never
    // changes a decision: it lies below every threshold that matters.  The registers are cut to S on the way out.
    auto kept_threshold = [&](float best) -> uint32_t {
        uint32_t key[ROW_MAXQ][4];
        if (REG) {
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) key[q][e] = order_key(x[q][e]);
        }
        int pass = 0;
        uint32_t lo = 0, t = 0;
        if (tr.top_k > 0) {              // lo = key of the top_k-th largest value: the largest lo with |{key >= lo}| >= top_k
            for (int bit = 31; bit >= 0; --bit, ++pass) {
                const uint32_t cand = lo | (1u << bit);
                int c = 0;               // wave-uniform
                if (REG) {
#pragma unroll
                    for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) c += __popcll(__ballot(key[q][e] >= cand));
                } else {
                    for (int j0 = 0; 4 * j0 < V; j0 += 256) {             // (a block-uniform trip count: every lane votes)
                        const sbs_f32x4 z = zquad(j0 + tid);
#pragma unroll
                        for (int e = 0; e < 4; ++e) c += __popcll(__ballot(order_key(z[e]) >= cand));
                    }
                }
                if (lane == 0) s_cnt[pass & 1][wave] = c;
                __syncthreads();
                const int* sc = s_cnt[pass & 1];
                if ((sc[0] + sc[1]) + (sc[2] + sc[3]) >= tr.top_k) lo = cand;
            }
            t = lo;
        }
        if (tr.top_p < 1.f) {
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
                } else {
                    for (int j = tid; 4 * j < V; j += 256) {
                        const sbs_f32x4 z = zquad(j);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const uint32_t kz = order_key(z[e]);
                            sm += (kz >= lo && kz >= cand) ? expf(z[e] - best) : 0.f;
                        }
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
            const float need = tr.top_p * mass_ge(lo);
            uint32_t hi = 0;             // the largest hi with mass_ge(hi) >= need; hi >= lo as mass_ge(lo) >= need
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = hi | (1u << bit);
                if (mass_ge(cand) >= need) hi = cand;
            }
            t = hi;
        }
        const uint32_t kbest = order_key(best);
        if (t > kbest) t = kbest;        // the arg-max is always kept
        if (REG) {
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) if (key[q][e] < t) x[q][e] = -INFINITY;
        }
        return t;
    };
    if (TRUNC && NM == 1) thr = kept_threshold(my[0]);   // the sums below then run over S: lse is the log-sum-exp over S
    sweep([&](int, const sbs_f32x4& y, const sbs_f32x4& y2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[0] += expf(y[e] - my[0]);                     // exp(-inf) == 0
        if (NM == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[NM - 1] += expf(y2[e] - my[NM - 1]);
        }
    });
#pragma unroll
    for (int m = 0; m < NM; ++m) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum[m] += __shfl_xor(sum[m], o);
        if (lane == 0) s_red[m][wave] = sum[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NM; ++m) lse[m] = my[m] + logf((s_red[m][0] + s_red[m][1]) + (s_red[m][2] + s_red[m][3]));
    // two models on the register path: the first row's registers take the word's log-probability under the averaged
    // distributions here, so that the sweep below is the one-model sweep (and unrolls as it does)
    if (REG && NM == 2) {
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q)
            if ((tid + 256 * q) * 4 < V) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[q][e] = sbs_mean_logp(x[q][e] - lse[0], x2[NM == 2 ? q : 0][e] - lse[NM - 1]);
            }
    }
    // TRUNC, two models: S on l, then L_S = max l + log(sum over S of exp(l - max l)); a kept word's log-probability is l - L_S
    float LS = 0.f;
    if (TRUNC && NM == 2) {
        auto zsweep = [&](auto&& f) {                    // the quads of l in the sweeps' order: the registers, or recomputed
            if (REG) {
#pragma unroll
                for (int q = 0; q < ROW_MAXQ; ++q)
                    if ((tid + 256 * q) * 4 < V) f(x[q]);
            } else {
                for (int j = tid; 4 * j < V; j += 256) f(zquad(j));
            }
        };
        float ml = -INFINITY;
        zsweep([&](const sbs_f32x4& z) { ml = fmaxf(ml, max4(z)); });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ml = fmaxf(ml, __shfl_xor(ml, o));
        if (lane == 0) s_zmax[wave] = ml;
        __syncthreads();
        ml = fmaxf(fmaxf(s_zmax[0], s_zmax[1]), fmaxf(s_zmax[2], s_zmax[3]));
        thr = kept_threshold(ml);
        float sm = 0.f;
        zsweep([&](const sbs_f32x4& z) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sm += order_key(z[e]) >= thr ? expf(z[e] - ml) : 0.f;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
        if (lane == 0) s_red[0][wave] = sm;              // (every read of s_red for lse precedes the barrier above)
        __syncthreads();
        LS = ml + logf((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]));
    }
    // the thread's own best SBS_KMAX words by (g descending, v ascending): it meets its words in ascending order, so a strict
    // comparison keeps the lower word in front
    float tv[SBS_KMAX], tp[SBS_KMAX];
    int ti[SBS_KMAX];
#pragma unroll
    for (int i = 0; i < SBS_KMAX; ++i) { tv[i] = -INFINITY; tp[i] = 0.f; ti[i] = SBS_NONE; }
    sweep([&](int j, const sbs_f32x4& y, const sbs_f32x4& y2) {
        uint32_t c[4];
        gumbel_quad_words(a.seed, a.offset, r, a.t, j, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float l;
            if (NM == 1) {
                if (!(y[e] > -INFINITY)) continue;                                    // -inf (and past V): never a candidate
                l = y[e] - lse[0];
            } else {
                l = REG ? y[e] : sbs_mean_logp(y[e] - lse[0], y2[e] - lse[NM - 1]);
                if (!(l > -INFINITY)) continue;                                       // impossible in both models (and past V)
                if (TRUNC) {
                    if (!REG && order_key(l) < thr) continue;                         // outside S (the registers were cut)
                    l -= LS;
                }
            }
            const float ph = phij + l;
            const float g = ph + gumbel_of_word(c[e]);
            if (g > tv[SBS_KMAX - 1]) {
                tv[SBS_KMAX - 1] = g; tp[SBS_KMAX - 1] = ph; ti[SBS_KMAX - 1] = 4 * j + e;
#pragma unroll
                for (int i = SBS_KMAX - 1; i > 0; --i)
                    if (tv[i] > tv[i - 1]) {
                        const float fv = tv[i], fp = tp[i]; const int fi = ti[i];
                        tv[i] = tv[i - 1]; tp[i] = tp[i - 1]; ti[i] = ti[i - 1];
                        tv[i - 1] = fv; tp[i - 1] = fp; ti[i - 1] = fi;
                    }
            }
        }
    });
    // k rounds: the workgroup's best head wins, its owner records and pops it
    float* cg = a.cand_g + (long long)r * SBS_KMAX;
    float* cp = a.cand_phi + (long long)r * SBS_KMAX;
    int* cv = a.cand_v + (long long)r * SBS_KMAX;
    for (int n = 0; n < a.k; ++n) {
        float bv = tv[0];
        int bi = ti[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_bv[n & 1][wave] = bv; s_bi[n & 1][wave] = bi; }
        __syncthreads();
        bv = s_bv[n & 1][0]; bi = s_bi[n & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = s_bv[n & 1][w];
            const int oi = s_bi[n & 1][w];
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (bi == SBS_NONE) {                                                         // the row has run out of words
            if (tid == 0) { cg[n] = -INFINITY; cp[n] = 0.f; cv[n] = 0; }
        } else if (ti[0] == bi) {
            cg[n] = tv[0]; cp[n] = tp[0]; cv[n] = bi;
#pragma unroll
            for (int i = 0; i + 1 < SBS_KMAX; ++i) { tv[i] = tv[i + 1]; tp[i] = tp[i + 1]; ti[i] = ti[i + 1]; }
            tv[SBS_KMAX - 1] = -INFINITY; ti[SBS_KMAX - 1] = SBS_NONE;
        }
    }
}

struct SbsMergeArgs {
    int k, V, Lmax;
    long long end_idx;
    float* phi; float* G; int* fin; int* len;            // (NI, k), updated in place
    const long long* seqs_in; long long* seqs_out;       // (NI, k, Lmax)
    long long* words; int* rows; int* n_open;
    const float* cand_g; const float* cand_phi; const int* cand_v;
};

// log(1 - exp(d)), d <= 0, without cancellation near d = 0 (d == 0 gives -inf)
__device__ __forceinline__ float sbs_log1mexp(float d) {
    return d > -0.6931472f ? logf(-expm1f(d)) : log1pf(-expf(d));
}

// one wave per image; lane c < k * k is candidate (parent c / k, the parent's rank-(c % k) word)
__global__ void __launch_bounds__(64) sbs_merge_k(const SbsMergeArgs a) {
    __shared__ int s_src[SBS_KMAX], s_len[SBS_KMAX], s_ext[SBS_KMAX];
    __shared__ long long s_word[SBS_KMAX];
    const int img = blockIdx.x, lane = threadIdx.x, k = a.k;
    const int base = img * k;
    const long long* sin = a.seqs_in + (long long)base * a.Lmax;
    long long* sout = a.seqs_out + (long long)base * a.Lmax;
    if (a.n_open[img] == 0) {                            // closed: the state stays, the tokens follow the buffer swap
        if (lane < k) { a.words[base + lane] = 0; a.rows[base + lane] = base + lane; }
        for (int e = lane; e < k * a.Lmax; e += 64) sout[e] = sin[e];
        return;
    }
    const int p = lane / k, i = lane - p * k;
    float val = -INFINITY, nphi = 0.f;
    int flat = SBS_NONE, word = 0, pfin = 0, plen = 0;
    if (lane < k * k) {
        const float Gp = a.G[base + p];
        pfin = a.fin[base + p];
        plen = a.len[base + p];
        if (Gp == -INFINITY) {
            // a dead slot has no candidates
        } else if (pfin) {
            if (i == 0) { val = Gp; nphi = a.phi[base + p]; word = (int)a.end_idx; flat = p * a.V + word; }
        } else {
            const long long c = (long long)(base + p) * SBS_KMAX;
            const float g = a.cand_g[c + i];
            if (g > -INFINITY) {
                word = a.cand_v[c + i];
                nphi = a.cand_phi[c + i];
                flat = p * a.V + word;
                if (i == 0) {
                    val = Gp;                            // the arg-max child inherits the parent's score exactly
                } else {
                    const float Z = a.cand_g[c];
                    const float u = (Gp - g) + sbs_log1mexp(g - Z);      // -inf when g == Z
                    val = Gp - fmaxf(u, 0.f) - log1pf(expf(-fabsf(u)));
                }
            }
        }
    }
    __syncthreads();                                     // every read of the slot state precedes every write below
    // rank by counting: candidates ahead of this one in (value descending, flat index ascending, lane ascending)
    int rank = 0;
    for (int l = 0; l < 64; ++l) {
        const float ov = __shfl(val, l);
        const int of = __shfl(flat, l);
        rank += (ov > val || (ov == val && (of < flat || (of == flat && l < lane)))) ? 1 : 0;
    }
    const bool slot = rank < k;                          // this lane fills output slot `rank`
    const bool hit = slot && val > -INFINITY;
    const bool nfin = hit && (pfin || (long long)word == a.end_idx);
    const unsigned long long open = __ballot(hit && !nfin);
    if (lane == 0) a.n_open[img] = __popcll(open);
    if (slot) {
        const int o = base + rank;
        const bool ext = hit && !pfin;                   // a live parent's child: one more token
        a.G[o] = hit ? val : -INFINITY;
        a.phi[o] = hit ? nphi : -INFINITY;
        a.fin[o] = nfin ? 1 : 0;
        a.len[o] = hit ? plen + (ext ? 1 : 0) : 0;
        a.words[o] = (hit && !nfin) ? (long long)word : 0;
        a.rows[o] = ext ? base + p : o;
        s_src[rank] = hit ? p : -1;
        s_len[rank] = plen;
        s_ext[rank] = ext ? 1 : 0;
        s_word[rank] = word;
    }
    __syncthreads();
    for (int s = 0; s < k; ++s) {
        if (s_src[s] < 0) continue;
        const int n = s_len[s] < a.Lmax ? s_len[s] : a.Lmax;
        const long long* from = sin + (long long)s_src[s] * a.Lmax;
        long long* to = sout + (long long)s * a.Lmax;
        for (int e = lane; e < n; e += 64) to[e] = from[e];
        if (lane == 0 && s_ext[s] && n < a.Lmax) to[n] = s_word[s];
    }
}

}  // namespace set

using namespace set;

extern "C" {

size_t set_sbs_workspace_bytes(int NI, int k) {
    if (NI <= 0 || k < 1 || k > SBS_KMAX) return 0;
    return 3 * round_up((size_t)NI * k * SBS_KMAX * sizeof(float), 256);
}

// logits2 == nullptr: one model (set_sbs_pick_f32); otherwise the two-model pick.  with_trunc: the *_opts entries, whose opts
// may carry top_k / top_p; the others refuse them
static int sbs_pick(const SetSbsArgs* a, const float* logits2, const SetSampleOpts* opts, bool with_trunc, void* stream) {
    if (!a || !a->logits || !a->phi || !a->G || !a->finished || !a->len || !a->seqs_in || !a->seqs_out || !a->words || !a->rows ||
        !a->n_open || !a->ws)
        return SET_ERR_ARG;
    if (a->NI <= 0 || a->k < 1 || a->k > SBS_KMAX || a->V <= 0 || a->t < 0 || a->t > GUMBEL_MAX_LEN - 1 || a->ld < a->V ||
        a->Lmax < a->t + 1 || a->seqs_in == a->seqs_out || a->end_idx < 0 || a->end_idx >= a->V)
        return SET_ERR_ARG;                              // (<end> is a word: a finished slot's flat index j V + end_idx stays inside slot j)
    SetSampleOpts tempered = {1.f, 0, 1.f, 0};           // opts without its truncation, for the check of the rest
    SbsTrunc tc = {0, 1.f};
    if (with_trunc && opts) {
        SET_TRY(sample_opts_check(opts));
        tempered.temperature = opts->temperature;
        tc.top_k = opts->top_k >= a->V ? 0 : opts->top_k;
        tc.top_p = opts->top_p;
    }
    SET_TRY(gumbel_opts_check(with_trunc ? &tempered : opts, a->V, 1));     // temperature only; V within the noise counters
    const bool trunc = tc.top_k > 0 || tc.top_p < 1.f;   // nothing to cut: the untruncated instantiation, the same bytes
    if ((long long)a->NI * a->k >= 0x7fffffffLL / SBS_KMAX) return SET_ERR_ARG;
    if (a->ws_bytes < set_sbs_workspace_bytes(a->NI, a->k) || !aligned16(a->ws)) return SET_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int B = a->NI * a->k;
    Carver cv(a->ws);
    SbsRowArgs ra;
    ra.logits = a->logits; ra.logits2 = logits2; ra.ld = a->ld; ra.k = a->k; ra.V = a->V; ra.t = a->t;
    ra.inv_t = opts ? 1.0f / opts->temperature : 1.f;
    ra.seed = a->seed; ra.offset = a->offset;
    ra.phi = a->phi; ra.G = a->G; ra.fin = a->finished; ra.n_open = a->n_open;
    ra.cand_g = cv.take<float>((size_t)B * SBS_KMAX);
    ra.cand_phi = cv.take<float>((size_t)B * SBS_KMAX);
    ra.cand_v = cv.take<int>((size_t)B * SBS_KMAX);
    SbsMergeArgs ma;
    ma.k = a->k; ma.V = a->V; ma.Lmax = a->Lmax; ma.end_idx = a->end_idx;
    ma.phi = a->phi; ma.G = a->G; ma.fin = a->finished; ma.len = a->len;
    ma.seqs_in = (const long long*)a->seqs_in; ma.seqs_out = (long long*)a->seqs_out;
    ma.words = (long long*)a->words; ma.rows = a->rows; ma.n_open = a->n_open;
    ma.cand_g = ra.cand_g; ma.cand_phi = ra.cand_phi; ma.cand_v = ra.cand_v;
    const bool reg = pick_reg_ok(Slabs{a->logits, 0, a->ld, 1}, a->V) && aligned16(logits2);
    // the scalar path re-reads the row in every sweep: three of them, and under truncation one per descent pass (32 for top-k,
    // 33 for top-p) and, for two models, two more for the maximum and the sum over the kept set
    const double sweeps = reg ? 1.0 : 3.0 + (trunc ? (tc.top_k > 0 ? 32.0 : 0.0) + (tc.top_p < 1.f ? 33.0 : 0.0) + (logits2 ? 2.0 : 0.0) : 0.0);
    static const char* const scope[2][2][2] = {          // [two models][truncated][scalar]
        {{"sbs_rows", "sbs_rows_scalar"}, {"sbs_rows_trunc", "sbs_rows_trunc_scalar"}},
        {{"sbs_rows_ens", "sbs_rows_ens_scalar"}, {"sbs_rows_ens_trunc", "sbs_rows_ens_trunc_scalar"}}};
#define SET_SBS_ROWS(REG, NM, TRUNC) hipLaunchKernelGGL((sbs_rows_k<REG, NM, TRUNC>), dim3(B), dim3(256), 0, st, ra, tc)
#define SET_SBS_ROWS_NM(REG, TRUNC) do { if (logits2) SET_SBS_ROWS(REG, 2, TRUNC); else SET_SBS_ROWS(REG, 1, TRUNC); } while (0)
#define SET_SBS_ROWS_REG(TRUNC) do { if (reg) SET_SBS_ROWS_NM(true, TRUNC); else SET_SBS_ROWS_NM(false, TRUNC); } while (0)
    {
        ProfScope ps(scope[logits2 != nullptr][trunc][!reg], st, 0.0, (logits2 ? 8.0 : 4.0) * sweeps * B * a->V);
        if (trunc) SET_SBS_ROWS_REG(true); else SET_SBS_ROWS_REG(false);
        SET_LAUNCH_CHECK();
    }
#undef SET_SBS_ROWS_REG
#undef SET_SBS_ROWS_NM
#undef SET_SBS_ROWS
    {
        ProfScope ps("sbs_merge", st, 0.0, 16.0 * B * (a->t + 1));
        hipLaunchKernelGGL(sbs_merge_k, dim3(a->NI), dim3(64), 0, st, ma);
        SET_LAUNCH_CHECK();
    }
    return SET_OK;
}

int set_sbs_pick_f32(const SetSbsArgs* a, const SetSampleOpts* opts, void* stream) { return sbs_pick(a, nullptr, opts, false, stream); }

int set_sbs_pick_ensemble_f32(const SetSbsArgs* a, const float* logits2, const SetSampleOpts* opts, void* stream) {
    if (!logits2) return SET_ERR_ARG;
    return sbs_pick(a, logits2, opts, false, stream);
}

int set_sbs_pick_opts_f32(const SetSbsArgs* a, const SetSampleOpts* opts, void* stream) { return sbs_pick(a, nullptr, opts, true, stream); }

int set_sbs_pick_ensemble_opts_f32(const SetSbsArgs* a, const float* logits2, const SetSampleOpts* opts, void* stream) {
    if (!logits2) return SET_ERR_ARG;
    return sbs_pick(a, logits2, opts, true, stream);
}

}  // extern "C"
