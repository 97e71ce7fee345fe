// Constrained beam-search pick (include/set_hip.h "Constrained beam-search pick"): the step epilogue of beam.hip with candidates
// REMOVED before the flat top-k — banned words, <end> before a minimum length, words that would repeat an n-gram of the
// hypothesis's own history — and completed hypotheses ranked by a length-normalised score.  Nothing is renormalised: a surviving
// candidate's value is the model's own log-probability plus the running score.
//
// Two launches, the shape of sbs.hip:
//   bc_rows_k    one workgroup per (image, slot) row — the V-sized work.  The row's ban list is built in LDS first (banned ids,
//                <end> while the minimum length forbids it, the words rule c yields from the row's tokens), the row is read once
//                (float4 into registers, or scalar re-reads), log-sum-exp, per-thread sorted top-k lists in which a word is looked
//                up in the ban list only when it would enter, k rounds of block arg-max.  A parent can place only its own k best
//                survivors among the image's k picks, so k (value, word) pairs per row are all the merge needs.
//   bd_merge_k   one wave per image, the slots in groups (one group: the constrained pick; set_beam_pick_diverse_f32: several, with
//                a Hamming penalty on the words earlier groups picked at this step): per group the flat top-g of its g x k
//                candidates (ties: lowest flat index j V + v), then the bookkeeping and the sequence copy of beam_tail.h with the
//                rank score r = x / cur_len^alpha for completed hypotheses.
// Both row-read paths give every thread the same quads in the same order and feed one set of lambdas: the outputs do not depend
// on the path.  No floating-point atomics, no scratch.
#include "beam_tail.h"

namespace set {

constexpr int BC_KMAX = BEAM_KMAX;
constexpr int BC_NONE = BEAM_NONE;
constexpr int BC_MAXBAN = 64;            // SetBeamConstraints::n_banned
constexpr int BC_MAXLEN = 256;           // Lmax: the row's tokens and the words rule c yields live in LDS
constexpr int BC_MAXNGRAM = 16;

struct BcRowArgs {
    const float* logits; const float* logits2; long long ld;     // logits2: the second model's rows (NM == 2), same V and ld
    int k, V, cur_len, Lmax;
    long long end_idx;
    const float* scores; const int* k_left; const long long* seqs_in;
    int ngram, min_len, n_banned;
    const long long* banned;
    float* cand_x; int* cand_w;                                   // (NI * k, BC_KMAX): value descending, word ascending among equals
};

template <bool REG, int NM>
__global__ void __launch_bounds__(256) bc_rows_k(const BcRowArgs a) {
    __shared__ float s_red[NM][4];
    __shared__ float s_bv[2][4];
    __shared__ int s_bi[2][4];
    __shared__ long long s_seq[BC_MAXLEN];
    __shared__ int s_ban[BC_MAXBAN + 1 + BC_MAXLEN];
    __shared__ int s_wcnt[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, L = a.cur_len, n = a.ngram;
    const float sc = a.scores[r];
    // a dead slot and every slot of a finished image offer no words: nothing is read
    if (sc == -INFINITY || a.k_left[r / a.k] <= 0) return;

    // ---- the row's ban list: words of [0, V), -1 = an entry that matches nothing
    if (tid < L) s_seq[tid] = a.seqs_in[(long long)r * a.Lmax + tid];
    int nfix = a.n_banned;
    if (tid < a.n_banned) {
        const long long b = a.banned[tid];
        s_ban[tid] = (b >= 0 && b < V) ? (int)b : -1;
    }
    if (L - 1 < a.min_len) {                             // rule b
        if (tid == 0) s_ban[nfix] = (a.end_idx >= 0 && a.end_idx < V) ? (int)a.end_idx : -1;
        ++nfix;
    }
    __syncthreads();
    // rule c: thread i - 1 owns position i in 1 .. L - n; the hits are compacted behind the fixed entries in position order
    bool hit = false;
    int hw = -1;
    if (n >= 1 && tid + 1 <= L - n) {
        const int i = tid + 1;
        hit = true;
        for (int q = 0; q + 1 < n; ++q) hit = hit && s_seq[i + q] == s_seq[L - n + 1 + q];
        const long long w = s_seq[i + n - 1];
        hit = hit && w >= 0 && w < V;
        hw = (int)w;
    }
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(votes);
    __syncthreads();
    int at = nfix, nban = nfix;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) at += s_wcnt[w]; nban += s_wcnt[w]; }
    if (hit) s_ban[at + __popcll(votes & ((1ull << lane) - 1ull))] = hw;
    __syncthreads();

    // ---- the row, read once
    const float* row = a.logits + (long long)r * a.ld;
    const float* row2 = NM == 2 ? a.logits2 + (long long)r * a.ld : row;
    f32x4 x[ROW_MAXQ], x2[NM == 2 ? ROW_MAXQ : 1];
    if (REG) {
#pragma unroll
        for (int q = 0; q < ROW_MAXQ; ++q) {
            const int v = (tid + 256 * q) * 4;
            x[q] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (NM == 2) x2[NM == 2 ? q : 0] = x[q];
            if (v < V) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(row + v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v + e < V) x[q][e] = w[e];
                if (NM == 2) {
                    const f32x4 w2 = *reinterpret_cast<const f32x4*>(row2 + v);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (v + e < V) x2[NM == 2 ? q : 0][e] = w2[e];
                }
            }
        }
    }
    // every thread visits its quads tid, tid + 256, ... in that order on either path, both models' quads of a visit together
    // (NM == 1: the one row twice); words past V are -inf
    auto sweep = [&](auto&& f) {
        if (REG) {
#pragma unroll
            for (int q = 0; q < ROW_MAXQ; ++q)
                if ((tid + 256 * q) * 4 < V) f(tid + 256 * q, x[q], NM == 2 ? x2[NM == 2 ? q : 0] : x[q]);
        } else {
            for (int j = tid; 4 * j < V; j += 256) {
                f32x4 y, y2;
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = 4 * j + e < V ? row[4 * j + e] : -INFINITY;
                if (NM == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) y2[e] = 4 * j + e < V ? row2[4 * j + e] : -INFINITY;
                }
                f(j, y, NM == 2 ? y2 : y);
            }
        }
    };
    // ---- per model: max, sum of exp in the fixed order of block_sum, log-sum-exp
    float my[NM], sum[NM], lse[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) { my[m] = -INFINITY; sum[m] = 0.f; }
    auto max4 = [](const f32x4& y) { return fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])); };
    sweep([&](int, const f32x4& y, const f32x4& y2) {
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
    sweep([&](int, const f32x4& y, const f32x4& y2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[0] += expf(y[e] - my[0]);                     // exp(-inf) == 0
        if (NM == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[NM - 1] += expf(y2[e] - my[NM - 1]);
        }
    });
#pragma unroll
    for (int m = 0; m < NM; ++m) lse[m] = my[m] + logf(block_sum(sum[m], s_red[m]));

    // ---- the thread's own best BC_KMAX survivors by (value descending, word ascending): it meets its words in ascending order,
    // so a strict comparison keeps the lower word in front.  The ban list is consulted only for a word that would enter.
    float tv[BC_KMAX];
    int ti[BC_KMAX];
#pragma unroll
    for (int i = 0; i < BC_KMAX; ++i) { tv[i] = -INFINITY; ti[i] = BC_NONE; }
    sweep([&](int j, const f32x4& y, const f32x4& y2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float lp;
            if (NM == 1) lp = y[e] - lse[0];
            else lp = logf((expf(y[e] - lse[0]) + expf(y2[e] - lse[NM - 1])) * 0.5f);
            const float c = sc + lp;
            if (c > tv[BC_KMAX - 1]) {                                                // (-inf, NaN and words past V never enter)
                const int word = 4 * j + e;
                bool banned = false;
                for (int b = 0; b < nban; ++b) banned = banned || s_ban[b] == word;
                if (banned) continue;
                tv[BC_KMAX - 1] = c; ti[BC_KMAX - 1] = word;
#pragma unroll
                for (int i = BC_KMAX - 1; i > 0; --i)
                    if (tv[i] > tv[i - 1]) {
                        const float fv = tv[i]; const int fi = ti[i];
                        tv[i] = tv[i - 1]; ti[i] = ti[i - 1];
                        tv[i - 1] = fv; ti[i - 1] = fi;
                    }
            }
        }
    });
    // ---- k rounds: the workgroup's best head wins, its owner records and pops it
    float* cx = a.cand_x + (long long)r * BC_KMAX;
    int* cw = a.cand_w + (long long)r * BC_KMAX;
    for (int p = 0; p < a.k; ++p) {
        float bv = tv[0];
        int bi = ti[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (beam_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_bv[p & 1][wave] = bv; s_bi[p & 1][wave] = bi; }
        __syncthreads();
        bv = s_bv[p & 1][0]; bi = s_bi[p & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (beam_better(s_bv[p & 1][w], s_bi[p & 1][w], bv, bi)) { bv = s_bv[p & 1][w]; bi = s_bi[p & 1][w]; }
        if (bi == BC_NONE) {                                                          // the row has run out of survivors
            if (tid == 0) { cx[p] = -INFINITY; cw[p] = 0; }
        } else if (ti[0] == bi) {
            cx[p] = tv[0]; cw[p] = bi;
#pragma unroll
            for (int i = 0; i + 1 < BC_KMAX; ++i) { tv[i] = tv[i + 1]; ti[i] = ti[i + 1]; }
            tv[BC_KMAX - 1] = -INFINITY; ti[BC_KMAX - 1] = BC_NONE;
        }
    }
}

// ---- the merge behind bc_rows_k, for the constrained pick (one group of k slots, no penalty, g_left IS k_left, no done_group) and
// for diverse (group) beam search.  The k slots of an image are G groups of g = k / G; group gi picks among the survivors of its own
// g rows by the key y = x - penalty n(word), n = how many counted non-<end> picks of groups 0 .. gi - 1 of this step took the word,
// and carries x.  At most k - g words are penalised and a penalty only lowers a key, so a row's k best survivors hold every
// candidate a group can pick: the (k, value, word) lists bc_rows_k writes are enough.  The bookkeeping of a group and the sequence
// copy are beam_tail.h's, with the rank score r = x / cur_len^alpha for completed hypotheses.
struct BcMergeArgs {
    BeamState s;
    float alpha;
    const float* cand_x; const int* cand_w;
    int* done_group;                            // (NI, k) group of every listed completion, or nullptr
    int* g_left;                                // (NI, groups); one group: may be k_left itself (both writes store the same number)
    int groups;
    float penalty;
};

// one wave per image, the groups one after the other; for group gi lane c < g * k is candidate (parent gi g + c / k, that parent's
// rank-(c % k) survivor)
__global__ void __launch_bounds__(64) bd_merge_k(const BcMergeArgs b) {
    __shared__ float s_cx[BC_KMAX * BC_KMAX];   // the image's k x k candidates, read before any slot state is written
    __shared__ int s_cw[BC_KMAX * BC_KMAX];     // BC_NONE: no candidate
    __shared__ float s_pick_v[BC_KMAX];         // the group's picks: carried value x (not the key)
    __shared__ int s_pick_i[BC_KMAX];
    __shared__ int s_pen[BC_KMAX];              // words of the earlier groups' counted non-<end> picks of this step
    __shared__ int s_npen;
    __shared__ BeamTailLds s_t;
    const BeamState& a = b.s;
    const int img = blockIdx.x, lane = threadIdx.x, k = a.k, V = a.V, G = b.groups, g = k / G;
    const int base = img * k;
    if (a.k_left[img] <= 0) {                    // finished image: identity state map, nothing else changes
        if (lane < k) { a.rows[base + lane] = base + lane; a.words[base + lane] = 0; }
        return;
    }
    {
        const int p = lane / k, i = lane - p * k;
        float val = -INFINITY;
        int w = BC_NONE;
        if (lane < k * k && a.scores[base + p] != -INFINITY) {   // (a dead slot's workspace row was not written)
            const long long c = (long long)(base + p) * BC_KMAX + i;
            const float cx = b.cand_x[c];
            if (cx > -INFINITY) { val = cx; w = b.cand_w[c]; }
        }
        s_cx[lane] = val; s_cw[lane] = w;
    }
    if (lane < BC_KMAX) s_t.copy[lane] = 0;
    if (lane == 0) { s_npen = 0; beam_tail_begin(a, img, s_t); }
    const float den = b.alpha != 0.f ? powf((float)a.cur_len, b.alpha) : 1.f;
    int left = 0;                                // lane 0: the image's k_left after the step
    for (int gi = 0; gi < G; ++gi) {
        const int gbase = gi * g;
        const int gl = b.g_left[img * G + gi];
        if (gl <= 0) {                           // a group that has ended: as a finished image
            if (lane < g) { a.rows[base + gbase + lane] = base + gbase + lane; a.words[base + gbase + lane] = 0; }
            continue;
        }
        if (lane < BC_KMAX) { s_pick_v[lane] = -INFINITY; s_pick_i[lane] = BC_NONE; }
        __syncthreads();                         // the candidates, the earlier groups' words and the cleared picks are in LDS
        float x = -INFINITY, y = -INFINITY;
        int flat = BC_NONE;
        if (lane < g * k) {
            const int w = s_cw[gbase * k + lane];
            if (w != BC_NONE) {
                x = s_cx[gbase * k + lane];
                flat = (gbase + lane / k) * V + w;
                int n = 0;
                for (int q = 0; q < s_npen; ++q) n += s_pen[q] == w ? 1 : 0;
                y = n ? x - b.penalty * (float)n : x;             // (<end> is never counted, so never penalised)
            }
        }
        // rank by counting: candidates ahead of this one in (key descending, flat index ascending, lane ascending); the lanes from
        // g k on hold none
        int rank = 0;
        for (int l = 0; l < g * k; ++l) {
            const float ov = __shfl(y, l);
            const int of = __shfl(flat, l);
            rank += (beam_better(ov, of, y, flat) || (ov == y && of == flat && l < lane)) ? 1 : 0;
        }
        if (rank < g && flat != BC_NONE) { s_pick_v[rank] = x; s_pick_i[rank] = flat; }
        __syncthreads();
        if (lane == 0) {                         // a group with no surviving finite candidate ends here
            const int gl_new = beam_tail_group<true, true>(a, img, gbase, g, gl, s_pick_v, s_pick_i, b.alpha, den, gi, b.done_group,
                                                           s_pen, &s_npen, s_t);
            b.g_left[img * G + gi] = gl_new;
            left += gl_new;
        }
    }
    __syncthreads();
    if (lane == 0) { a.k_left[img] = left; a.n_done[img] = s_t.done_at + s_t.done_n; }
    beam_tail_copy(a, img, s_t, lane, 64);
}

}  // namespace set

using namespace set;

extern "C" {

size_t set_beam_pick_constrained_workspace_bytes(int NI, int k) {
    if (NI <= 0 || k < 1 || k > BC_KMAX) return 0;
    return 2 * round_up((size_t)NI * k * BC_KMAX * sizeof(float), 256);
}

size_t set_beam_pick_diverse_workspace_bytes(int NI, int k) { return set_beam_pick_constrained_workspace_bytes(NI, k); }

// the pointer, range and constraint checks of both entries
static int bc_check(const float* logits, int64_t ld, int NI, const BeamState& s, const SetBeamConstraints* c, const void* ws,
                    size_t ws_bytes) {
    if (!logits || !s.scores || !s.k_left || !s.seqs_in || !s.seqs_out || !s.best_score || !s.best_seq || !s.best_len || !s.words ||
        !s.rows)
        return SET_ERR_ARG;
    if (!s.done_score || !s.done_seq || !s.done_len || !s.n_done || !c || !ws || !aligned16(ws)) return SET_ERR_ARG;
    if (NI <= 0 || s.k <= 0 || s.V <= 0 || s.cur_len < 1 || s.cur_len + 1 > s.Lmax || ld < s.V) return SET_ERR_ARG;
    if (c->no_repeat_ngram < 0 || c->no_repeat_ngram > BC_MAXNGRAM || c->min_len < 0) return SET_ERR_ARG;
    if (!std::isfinite(c->length_alpha) || c->length_alpha < 0.f) return SET_ERR_ARG;
    if (c->n_banned < 0 || c->n_banned > BC_MAXBAN || (c->n_banned == 0) != (c->banned == nullptr)) return SET_ERR_ARG;
    if (s.k > BC_KMAX || (long long)s.k * s.V >= 0x7fffffffLL || s.Lmax > BC_MAXLEN) return SET_ERR_UNSUPPORTED;
    if ((long long)NI * s.k >= 0x7fffffffLL / BC_KMAX || ws_bytes < set_beam_pick_constrained_workspace_bytes(NI, s.k)) return SET_ERR_ARG;
    return SET_OK;
}

// the workspace carve and the rows launch of both entries; ma gets the state, alpha and the candidate lists the merge reads
static int bc_rows(const float* logits, const float* logits2, int64_t ld, int NI, const BeamState& s, const SetBeamConstraints* c,
                   void* ws, hipStream_t st, BcMergeArgs& ma) {
    const int B = NI * s.k;
    Carver cv(ws);
    BcRowArgs ra;
    ra.logits = logits; ra.logits2 = logits2; ra.ld = ld; ra.k = s.k; ra.V = s.V; ra.cur_len = s.cur_len; ra.Lmax = s.Lmax;
    ra.end_idx = s.end_idx; ra.scores = s.scores; ra.k_left = s.k_left; ra.seqs_in = s.seqs_in;
    ra.ngram = c->no_repeat_ngram; ra.min_len = c->min_len; ra.n_banned = c->n_banned; ra.banned = (const long long*)c->banned;
    ra.cand_x = cv.take<float>((size_t)B * BC_KMAX);
    ra.cand_w = cv.take<int>((size_t)B * BC_KMAX);
    ma.s = s; ma.alpha = c->length_alpha; ma.cand_x = ra.cand_x; ma.cand_w = ra.cand_w;
    const bool reg = pick_reg_ok(Slabs{logits, 0, ld, 1}, s.V) && aligned16(logits2);
    static const char* const scope[2][2] = {{"beam_rows", "beam_rows_scalar"}, {"beam_rows_ens", "beam_rows_ens_scalar"}};
#define SET_BC_ROWS(REG, NM) hipLaunchKernelGGL((bc_rows_k<REG, NM>), dim3(B), dim3(256), 0, st, ra)
    // the scalar path re-reads the row in each of its three sweeps
    ProfScope ps(scope[logits2 != nullptr][!reg], st, 0.0, (logits2 ? 8.0 : 4.0) * (reg ? 1.0 : 3.0) * B * s.V);
    if (reg) { if (logits2) SET_BC_ROWS(true, 2); else SET_BC_ROWS(true, 1); }
    else { if (logits2) SET_BC_ROWS(false, 2); else SET_BC_ROWS(false, 1); }
#undef SET_BC_ROWS
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// the merge of one group of k slots: its g_left is k_left
int set_beam_pick_constrained_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                                  int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in, int64_t* seqs_out,
                                  float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                                  float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done,
                                  const SetBeamConstraints* c, void* ws, size_t ws_bytes, void* stream) {
    const BeamState s = beam_state(k, V, end_idx, cur_len, Lmax, scores, k_left, seqs_in, seqs_out, best_score, best_seq, best_len, words,
                                   rows, done_score, done_seq, done_len, n_done);
    if (int rc = bc_check(logits, ld, NI, s, c, ws, ws_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    BcMergeArgs ma;
    if (int rc = bc_rows(logits, logits2, ld, NI, s, c, ws, st, ma)) return rc;
    ma.done_group = nullptr; ma.g_left = k_left; ma.groups = 1; ma.penalty = 0.f;
    ProfScope ps("beam_merge", st, 0.0, 16.0 * NI * k * (cur_len + 1));
    hipLaunchKernelGGL(bd_merge_k, dim3(NI), dim3(64), 0, st, ma);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

// the rows launch of set_beam_pick_constrained_f32 (k_left is the sum of the image's g_left), then the group merge
int set_beam_pick_diverse_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                              int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in, int64_t* seqs_out,
                              float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                              float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done,
                              int32_t* done_group, int32_t* g_left, int groups, float penalty,
                              const SetBeamConstraints* c, void* ws, size_t ws_bytes, void* stream) {
    const BeamState s = beam_state(k, V, end_idx, cur_len, Lmax, scores, k_left, seqs_in, seqs_out, best_score, best_seq, best_len, words,
                                   rows, done_score, done_seq, done_len, n_done);
    if (!done_group || !g_left || groups < 1 || k % groups != 0 || !std::isfinite(penalty) || penalty < 0.f) return SET_ERR_ARG;
    if (int rc = bc_check(logits, ld, NI, s, c, ws, ws_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    BcMergeArgs ma;
    if (int rc = bc_rows(logits, logits2, ld, NI, s, c, ws, st, ma)) return rc;
    ma.done_group = done_group; ma.g_left = g_left; ma.groups = groups; ma.penalty = penalty;
    ProfScope ps("beam_merge_groups", st, 0.0, 16.0 * NI * k * (cur_len + 1));
    hipLaunchKernelGGL(bd_merge_k, dim3(NI), dim3(64), 0, st, ma);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

}  // extern "C"

