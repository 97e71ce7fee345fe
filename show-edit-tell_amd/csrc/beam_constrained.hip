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
//   bc_merge_k   one wave per image: the flat top-k of the k x k candidates (ties: lowest flat index j V + v), then the bookkeeping
//                of beam_pick_k step 3 with the rank score r = x / cur_len^alpha for completed hypotheses, and the sequence copy.
//   bd_merge_k   set_beam_pick_diverse_f32's merge behind the same bc_rows_k launch: the slots in groups, a Hamming penalty on the
//                words earlier groups picked at this step (see there).
// Both row-read paths give every thread the same quads in the same order and feed one set of lambdas: the outputs do not depend
// on the path.  No floating-point atomics, no scratch.
#include "row_pick.h"

namespace set {

constexpr int BC_KMAX = 8;
constexpr int BC_NONE = 0x7fffffff;
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

struct BcMergeArgs {
    int k, V, cur_len, Lmax;
    long long end_idx;
    float alpha;
    float* scores; int* k_left;
    const long long* seqs_in; long long* seqs_out;
    float* best_score; long long* best_seq; int* best_len;
    long long* words; int* rows;
    float* done_score; long long* done_seq; int* done_len; int* n_done;
    const float* cand_x; const int* cand_w;
};

// one wave per image; lane c < k * k is candidate (parent c / k, the parent's rank-(c % k) survivor)
__global__ void __launch_bounds__(64) bc_merge_k(const BcMergeArgs a) {
    __shared__ float s_pick_v[BC_KMAX];
    __shared__ int s_pick_i[BC_KMAX];
    __shared__ int s_src[BC_KMAX];              // per output slot: parent hypothesis
    __shared__ long long s_word[BC_KMAX];       // per output slot: appended word
    __shared__ int s_best_parent;
    __shared__ long long s_best_word;
    __shared__ int s_done_par[BC_KMAX];         // per completion of this pick: parent hypothesis
    __shared__ long long s_done_word[BC_KMAX];
    __shared__ int s_done_at, s_done_n, s_exhausted;
    const int img = blockIdx.x, lane = threadIdx.x, k = a.k, V = a.V;
    const int base = img * k;
    const int kl = a.k_left[img];
    if (kl <= 0) {                               // finished image: identity state map, nothing else changes
        if (lane < k) { a.rows[base + lane] = base + lane; a.words[base + lane] = 0; }
        return;
    }
    const int p = lane / k, i = lane - p * k;
    float val = -INFINITY;
    int flat = BC_NONE;
    if (lane < k * k && a.scores[base + p] != -INFINITY) {       // (a dead slot's workspace row was not written)
        const long long c = (long long)(base + p) * BC_KMAX + i;
        const float cx = a.cand_x[c];
        if (cx > -INFINITY) { val = cx; flat = p * V + a.cand_w[c]; }
    }
    if (lane < BC_KMAX) { s_pick_v[lane] = -INFINITY; s_pick_i[lane] = BC_NONE; }
    __syncthreads();                             // every read of the slot state precedes every write below
    // rank by counting: candidates ahead of this one in (value descending, flat index ascending, lane ascending)
    int rank = 0;
    for (int l = 0; l < 64; ++l) {
        const float ov = __shfl(val, l);
        const int of = __shfl(flat, l);
        rank += (beam_better(ov, of, val, flat) || (ov == val && of == flat && l < lane)) ? 1 : 0;
    }
    if (rank < k && flat != BC_NONE) { s_pick_v[rank] = val; s_pick_i[rank] = flat; }
    __syncthreads();

    // ---- the bookkeeping of one image: beam_pick_k step 3 (beam.hip) with the rank score of completed hypotheses
    if (lane == 0) {
        int n_end = 0, c_arg = -1, slot = 0;
        float c_best = -INFINITY;
        bool live[BC_KMAX];
        float rs[BC_KMAX];                       // rank score of pick r, where it completes a hypothesis
        const float den = a.alpha != 0.f ? powf((float)a.cur_len, a.alpha) : 1.f;
        s_exhausted = s_pick_i[0] == BC_NONE;    // no surviving finite candidate: the image ends here
        for (int r = 0; r < k; ++r) {
            const int fl = s_pick_i[r];
            const bool ok = fl != BC_NONE && r < kl;                      // only the first k_left picks count
            const long long word = ok ? fl % V : 0;
            const bool is_end = ok && word == a.end_idx;
            live[r] = ok && !is_end;
            rs[r] = a.alpha != 0.f ? s_pick_v[r] / den : s_pick_v[r];
            if (is_end) {
                ++n_end;
                if (rs[r] > c_best) { c_best = rs[r]; c_arg = r; }       // first maximum
            }
        }
        s_best_parent = -1;
        if (c_arg >= 0 && c_best > a.best_score[img]) {
            a.best_score[img] = c_best;
            a.best_len[img] = a.cur_len + 1;
            s_best_parent = s_pick_i[c_arg] / V;
            s_best_word = s_pick_i[c_arg] % V;
        }
        a.k_left[img] = s_exhausted ? 0 : kl - n_end;
        const int at = max(a.n_done[img], 0);    // the completions of this pick, in pick-rank order
        int nd = 0;
        for (int r = 0; r < k; ++r) {
            const int fl = s_pick_i[r];
            if (!(fl != BC_NONE && r < kl && fl % V == a.end_idx) || at + nd >= k) continue;
            a.done_score[base + at + nd] = rs[r];
            a.done_len[base + at + nd] = a.cur_len + 1;
            s_done_par[nd] = fl / V;
            s_done_word[nd] = fl % V;
            ++nd;
        }
        a.n_done[img] = at + nd;
        s_done_at = at; s_done_n = nd;
        // live picks first, in pick order; the other slots die
        for (int pass = 0; pass < 2; ++pass)
            for (int r = 0; r < k; ++r) {
                if ((pass == 0) != live[r]) continue;
                const int fl = s_pick_i[r];
                const int parent = fl != BC_NONE ? fl / V : 0;
                const long long word = fl != BC_NONE ? fl % V : 0;
                a.scores[base + slot] = live[r] ? s_pick_v[r] : -INFINITY;
                a.words[base + slot] = live[r] ? word : 0;
                a.rows[base + slot] = s_exhausted ? base + slot : base + parent;
                s_src[slot] = parent;
                s_word[slot] = word;
                ++slot;
            }
    }
    __syncthreads();
    if (s_exhausted) return;                     // like a finished image: the sequences are not copied
    const int L = a.cur_len;
    const long long* sin = a.seqs_in + (long long)base * a.Lmax;
    long long* sout = a.seqs_out + (long long)base * a.Lmax;
    for (int e = lane; e < k * (L + 1); e += 64) {
        const int slot = e / (L + 1), q = e - slot * (L + 1);
        sout[(long long)slot * a.Lmax + q] = q < L ? sin[(long long)s_src[slot] * a.Lmax + q] : s_word[slot];
    }
    if (s_best_parent >= 0)
        for (int q = lane; q <= L; q += 64)
            a.best_seq[(long long)img * a.Lmax + q] = q < L ? sin[(long long)s_best_parent * a.Lmax + q] : s_best_word;
    if (s_done_n > 0) {
        long long* dout = a.done_seq + ((long long)base + s_done_at) * a.Lmax;
        for (int e = lane; e < s_done_n * (L + 1); e += 64) {
            const int j = e / (L + 1), q = e - j * (L + 1);
            dout[(long long)j * a.Lmax + q] = q < L ? sin[(long long)s_done_par[j] * a.Lmax + q] : s_done_word[j];
        }
    }
}

// ---- diverse (group) beam search: the merge of set_beam_pick_diverse_f32 behind an unchanged bc_rows_k launch.  The k slots of an
// image are G groups of g = k / G; group gi picks among the survivors of its own g rows by the key y = x - penalty n(word), n = how
// many counted non-<end> picks of groups 0 .. gi - 1 of this step took the word, and carries x.  At most k - g words are penalised
// and a penalty only lowers a key, so a row's k best survivors hold every candidate a group can pick: the (k, value, word) lists
// bc_rows_k writes are enough.  The bookkeeping of a group is bc_merge_k's on its g slots and its own g_left, restated here
// because bc_merge_k was not to change.
struct BdMergeArgs {
    BcMergeArgs m;
    int* done_group; int* g_left;
    int groups;
    float penalty;
};

// one wave per image, the groups one after the other; for group gi lane c < g * k is candidate (parent gi g + c / k, that parent's
// rank-(c % k) survivor)
__global__ void __launch_bounds__(64) bd_merge_k(const BdMergeArgs b) {
    __shared__ float s_cx[BC_KMAX * BC_KMAX];   // the image's k x k candidates, read before any slot state is written
    __shared__ int s_cw[BC_KMAX * BC_KMAX];     // BC_NONE: no candidate
    __shared__ float s_pick_v[BC_KMAX];         // the group's picks: carried value x (not the key)
    __shared__ int s_pick_i[BC_KMAX];
    __shared__ int s_pen[BC_KMAX];              // words of the earlier groups' counted non-<end> picks of this step
    __shared__ int s_npen;
    __shared__ int s_src[BC_KMAX];              // per output slot: parent hypothesis (slot index within the image)
    __shared__ long long s_word[BC_KMAX];       // per output slot: appended word
    __shared__ int s_copy[BC_KMAX];             // per output slot: its group picked at this step, the sequence is copied
    __shared__ int s_best_parent;
    __shared__ long long s_best_word;
    __shared__ int s_done_par[BC_KMAX];         // per completion of this step: parent hypothesis
    __shared__ long long s_done_word[BC_KMAX];
    __shared__ int s_done_at, s_done_n;
    const BcMergeArgs& a = b.m;
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
            const float cx = a.cand_x[c];
            if (cx > -INFINITY) { val = cx; w = a.cand_w[c]; }
        }
        s_cx[lane] = val; s_cw[lane] = w;
    }
    if (lane < BC_KMAX) s_copy[lane] = 0;
    if (lane == 0) { s_npen = 0; s_best_parent = -1; s_done_n = 0; s_done_at = max(a.n_done[img], 0); }
    const float den = a.alpha != 0.f ? powf((float)a.cur_len, a.alpha) : 1.f;
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
        // ---- the bookkeeping of one group: bc_merge_k's on the slots gbase .. gbase + g - 1
        if (lane == 0) {
            const bool exhausted = s_pick_i[0] == BC_NONE;        // no surviving finite candidate: the group ends here
            int n_end = 0, c_arg = -1, slot = 0, nd = 0;
            float c_best = -INFINITY;
            for (int r = 0; r < g; ++r) {
                const int fl = s_pick_i[r];
                if (!(fl != BC_NONE && r < gl && fl % V == a.end_idx)) continue;   // only the first g_left picks count
                const float rs = a.alpha != 0.f ? s_pick_v[r] / den : s_pick_v[r];
                ++n_end;
                if (rs > c_best) { c_best = rs; c_arg = r; }      // first maximum
                const int at = s_done_at + s_done_n + nd;         // completions in group order, then pick rank
                if (at >= k) continue;
                a.done_score[base + at] = rs;
                a.done_len[base + at] = a.cur_len + 1;
                b.done_group[base + at] = gi;
                s_done_par[s_done_n + nd] = fl / V;
                s_done_word[s_done_n + nd] = fl % V;
                ++nd;
            }
            s_done_n += nd;
            if (c_arg >= 0 && c_best > a.best_score[img]) {
                a.best_score[img] = c_best;
                a.best_len[img] = a.cur_len + 1;
                s_best_parent = s_pick_i[c_arg] / V;
                s_best_word = s_pick_i[c_arg] % V;
            }
            const int gl_new = exhausted ? 0 : gl - n_end;
            b.g_left[img * G + gi] = gl_new;
            left += gl_new;
            // live picks first, in pick order; the other slots die
            for (int pass = 0; pass < 2; ++pass)
                for (int r = 0; r < g; ++r) {
                    const int fl = s_pick_i[r];
                    const bool live = fl != BC_NONE && r < gl && fl % V != a.end_idx;
                    if ((pass == 0) != live) continue;
                    const int parent = fl != BC_NONE ? fl / V : gbase;
                    const long long word = fl != BC_NONE ? fl % V : 0;
                    const int o = gbase + slot;
                    a.scores[base + o] = live ? s_pick_v[r] : -INFINITY;
                    a.words[base + o] = live ? word : 0;
                    a.rows[base + o] = exhausted ? base + o : base + parent;
                    s_src[o] = parent;
                    s_word[o] = word;
                    s_copy[o] = exhausted ? 0 : 1;                // like a finished image: the sequences are not copied
                    if (live) s_pen[s_npen++] = (int)word;        // at most k - g words before the last group
                    ++slot;
                }
        }
    }
    __syncthreads();
    if (lane == 0) { a.k_left[img] = left; a.n_done[img] = s_done_at + s_done_n; }
    const int L = a.cur_len;
    const long long* sin = a.seqs_in + (long long)base * a.Lmax;
    long long* sout = a.seqs_out + (long long)base * a.Lmax;
    for (int e = lane; e < k * (L + 1); e += 64) {
        const int slot = e / (L + 1), q = e - slot * (L + 1);
        if (s_copy[slot]) sout[(long long)slot * a.Lmax + q] = q < L ? sin[(long long)s_src[slot] * a.Lmax + q] : s_word[slot];
    }
    if (s_best_parent >= 0)
        for (int q = lane; q <= L; q += 64)
            a.best_seq[(long long)img * a.Lmax + q] = q < L ? sin[(long long)s_best_parent * a.Lmax + q] : s_best_word;
    if (s_done_n > 0) {
        long long* dout = a.done_seq + ((long long)base + s_done_at) * a.Lmax;
        for (int e = lane; e < s_done_n * (L + 1); e += 64) {
            const int j = e / (L + 1), q = e - j * (L + 1);
            dout[(long long)j * a.Lmax + q] = q < L ? sin[(long long)s_done_par[j] * a.Lmax + q] : s_done_word[j];
        }
    }
}

}  // namespace set

using namespace set;

extern "C" {

size_t set_beam_pick_constrained_workspace_bytes(int NI, int k) {
    if (NI <= 0 || k < 1 || k > BC_KMAX) return 0;
    return 2 * round_up((size_t)NI * k * BC_KMAX * sizeof(float), 256);
}

int set_beam_pick_constrained_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                                  int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in, int64_t* seqs_out,
                                  float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                                  float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done,
                                  const SetBeamConstraints* c, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !scores || !k_left || !seqs_in || !seqs_out || !best_score || !best_seq || !best_len || !words || !rows)
        return SET_ERR_ARG;
    if (!done_score || !done_seq || !done_len || !n_done || !c || !ws || !aligned16(ws)) return SET_ERR_ARG;
    if (NI <= 0 || k <= 0 || V <= 0 || cur_len < 1 || cur_len + 1 > Lmax || ld < V) return SET_ERR_ARG;
    if (c->no_repeat_ngram < 0 || c->no_repeat_ngram > BC_MAXNGRAM || c->min_len < 0) return SET_ERR_ARG;
    if (!std::isfinite(c->length_alpha) || c->length_alpha < 0.f) return SET_ERR_ARG;
    if (c->n_banned < 0 || c->n_banned > BC_MAXBAN || (c->n_banned == 0) != (c->banned == nullptr)) return SET_ERR_ARG;
    if (k > BC_KMAX || (long long)k * V >= 0x7fffffffLL || Lmax > BC_MAXLEN) return SET_ERR_UNSUPPORTED;
    if ((long long)NI * k >= 0x7fffffffLL / BC_KMAX || ws_bytes < set_beam_pick_constrained_workspace_bytes(NI, k)) return SET_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int B = NI * k;
    Carver cv(ws);
    BcRowArgs ra;
    ra.logits = logits; ra.logits2 = logits2; ra.ld = ld; ra.k = k; ra.V = V; ra.cur_len = cur_len; ra.Lmax = Lmax;
    ra.end_idx = end_idx; ra.scores = scores; ra.k_left = k_left; ra.seqs_in = (const long long*)seqs_in;
    ra.ngram = c->no_repeat_ngram; ra.min_len = c->min_len; ra.n_banned = c->n_banned; ra.banned = (const long long*)c->banned;
    ra.cand_x = cv.take<float>((size_t)B * BC_KMAX);
    ra.cand_w = cv.take<int>((size_t)B * BC_KMAX);
    BcMergeArgs ma;
    ma.k = k; ma.V = V; ma.cur_len = cur_len; ma.Lmax = Lmax; ma.end_idx = end_idx; ma.alpha = c->length_alpha;
    ma.scores = scores; ma.k_left = k_left; ma.seqs_in = (const long long*)seqs_in; ma.seqs_out = (long long*)seqs_out;
    ma.best_score = best_score; ma.best_seq = (long long*)best_seq; ma.best_len = best_len;
    ma.words = (long long*)words; ma.rows = rows;
    ma.done_score = done_score; ma.done_seq = (long long*)done_seq; ma.done_len = done_len; ma.n_done = n_done;
    ma.cand_x = ra.cand_x; ma.cand_w = ra.cand_w;
    const bool reg = pick_reg_ok(Slabs{logits, 0, ld, 1}, V) && aligned16(logits2);
    static const char* const scope[2][2] = {{"beam_rows", "beam_rows_scalar"}, {"beam_rows_ens", "beam_rows_ens_scalar"}};
#define SET_BC_ROWS(REG, NM) hipLaunchKernelGGL((bc_rows_k<REG, NM>), dim3(B), dim3(256), 0, st, ra)
    {
        // the scalar path re-reads the row in each of its three sweeps
        ProfScope ps(scope[logits2 != nullptr][!reg], st, 0.0, (logits2 ? 8.0 : 4.0) * (reg ? 1.0 : 3.0) * B * V);
        if (reg) { if (logits2) SET_BC_ROWS(true, 2); else SET_BC_ROWS(true, 1); }
        else { if (logits2) SET_BC_ROWS(false, 2); else SET_BC_ROWS(false, 1); }
        SET_LAUNCH_CHECK();
    }
#undef SET_BC_ROWS
    {
        ProfScope ps("beam_merge", st, 0.0, 16.0 * B * (cur_len + 1));
        hipLaunchKernelGGL(bc_merge_k, dim3(NI), dim3(64), 0, st, ma);
        SET_LAUNCH_CHECK();
    }
    return SET_OK;
}

size_t set_beam_pick_diverse_workspace_bytes(int NI, int k) { return set_beam_pick_constrained_workspace_bytes(NI, k); }

// the rows launch of set_beam_pick_constrained_f32, unchanged (k_left is the sum of the image's g_left), then the group merge
int set_beam_pick_diverse_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                              int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in, int64_t* seqs_out,
                              float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                              float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done,
                              int32_t* done_group, int32_t* g_left, int groups, float penalty,
                              const SetBeamConstraints* c, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !scores || !k_left || !seqs_in || !seqs_out || !best_score || !best_seq || !best_len || !words || !rows)
        return SET_ERR_ARG;
    if (!done_score || !done_seq || !done_len || !n_done || !done_group || !g_left || !c || !ws || !aligned16(ws))
        return SET_ERR_ARG;
    if (groups < 1 || k % groups != 0 || !std::isfinite(penalty) || penalty < 0.f) return SET_ERR_ARG;
    if (NI <= 0 || k <= 0 || V <= 0 || cur_len < 1 || cur_len + 1 > Lmax || ld < V) return SET_ERR_ARG;
    if (c->no_repeat_ngram < 0 || c->no_repeat_ngram > BC_MAXNGRAM || c->min_len < 0) return SET_ERR_ARG;
    if (!std::isfinite(c->length_alpha) || c->length_alpha < 0.f) return SET_ERR_ARG;
    if (c->n_banned < 0 || c->n_banned > BC_MAXBAN || (c->n_banned == 0) != (c->banned == nullptr)) return SET_ERR_ARG;
    if (k > BC_KMAX || (long long)k * V >= 0x7fffffffLL || Lmax > BC_MAXLEN) return SET_ERR_UNSUPPORTED;
    if ((long long)NI * k >= 0x7fffffffLL / BC_KMAX || ws_bytes < set_beam_pick_diverse_workspace_bytes(NI, k)) return SET_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int B = NI * k;
    Carver cv(ws);
    BcRowArgs ra;
    ra.logits = logits; ra.logits2 = logits2; ra.ld = ld; ra.k = k; ra.V = V; ra.cur_len = cur_len; ra.Lmax = Lmax;
    ra.end_idx = end_idx; ra.scores = scores; ra.k_left = k_left; ra.seqs_in = (const long long*)seqs_in;
    ra.ngram = c->no_repeat_ngram; ra.min_len = c->min_len; ra.n_banned = c->n_banned; ra.banned = (const long long*)c->banned;
    ra.cand_x = cv.take<float>((size_t)B * BC_KMAX);
    ra.cand_w = cv.take<int>((size_t)B * BC_KMAX);
    BdMergeArgs da;
    BcMergeArgs& ma = da.m;
    ma.k = k; ma.V = V; ma.cur_len = cur_len; ma.Lmax = Lmax; ma.end_idx = end_idx; ma.alpha = c->length_alpha;
    ma.scores = scores; ma.k_left = k_left; ma.seqs_in = (const long long*)seqs_in; ma.seqs_out = (long long*)seqs_out;
    ma.best_score = best_score; ma.best_seq = (long long*)best_seq; ma.best_len = best_len;
    ma.words = (long long*)words; ma.rows = rows;
    ma.done_score = done_score; ma.done_seq = (long long*)done_seq; ma.done_len = done_len; ma.n_done = n_done;
    ma.cand_x = ra.cand_x; ma.cand_w = ra.cand_w;
    da.done_group = done_group; da.g_left = g_left; da.groups = groups; da.penalty = penalty;
    const bool reg = pick_reg_ok(Slabs{logits, 0, ld, 1}, V) && aligned16(logits2);
    static const char* const scope[2][2] = {{"beam_rows", "beam_rows_scalar"}, {"beam_rows_ens", "beam_rows_ens_scalar"}};
#define SET_BC_ROWS(REG, NM) hipLaunchKernelGGL((bc_rows_k<REG, NM>), dim3(B), dim3(256), 0, st, ra)
    {
        // the scalar path re-reads the row in each of its three sweeps
        ProfScope ps(scope[logits2 != nullptr][!reg], st, 0.0, (logits2 ? 8.0 : 4.0) * (reg ? 1.0 : 3.0) * B * V);
        if (reg) { if (logits2) SET_BC_ROWS(true, 2); else SET_BC_ROWS(true, 1); }
        else { if (logits2) SET_BC_ROWS(false, 2); else SET_BC_ROWS(false, 1); }
        SET_LAUNCH_CHECK();
    }
#undef SET_BC_ROWS
    {
        ProfScope ps("beam_merge_groups", st, 0.0, 16.0 * B * (cur_len + 1));
        hipLaunchKernelGGL(bd_merge_k, dim3(NI), dim3(64), 0, st, da);
        SET_LAUNCH_CHECK();
    }
    return SET_OK;
}

}  // extern "C"
