// Word edit distance on the device (include/set_hip.h set_edit_device_score / set_edit_device_align): the statistics, the
// similarity and the canonical word alignment that editdist.py states, from id tensors in device memory: how far a caption is
// from its closest reference (evaluate.validation_edit), how much the model edited and which input word each output word
// corresponds to (evaluate.edit_statistics / edit_alignment), and a utility for evaluate.consensus_rerank.
//
//   d(h, r) = unit-cost Levenshtein distance;  m = max(len h, len r);  sim = (m - d) / m, 1 when both are empty
//   the reference of a set = the one of largest sim, compared as fractions (empty against empty: 1/1), of equal ones the first
//   stats = (dist, len_h, len_r, ref);  score = sim of those integers
//
// One wave holds a sentence, one position per lane (csrc/ngram_wave.h states the limits and the length rules and reads the row),
// so a column of the table's vertical differences is two 64-bit wave masks and the distance is the bit-parallel recurrence of
// Myers in Hyyro's global-distance form on wave-uniform words: lane i holds the field g_i = id + 1 of the sentence that lies along
// the rows (0 beyond its length m), Pv = the low m bits, Mv = 0, dist = m, and for every position j of the other sentence
//     Eq = ballot(g_lane == f_j);  Xv = Eq | Mv;  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;  Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh
//     dist += bit m-1 of Ph;  dist -= bit m-1 of Mh;  Ph = (Ph << 1) | 1;  Mh <<= 1
//     Pv = (Mh | ~(Xv | Ph)) & mask;  Mv = Ph & Xv & mask
// f_j >= 1 inside a sentence, so the 0 fields of padding never match; the carry out of bit 63 is dropped; the 1 shifted into Ph
// is row 0 of the table growing by 1 per column.  The lanes only supply the match masks.  A cell of the table follows from its
// column's pair:  D[i][j] = j + popcount(Pv_j & low(i)) - popcount(Mv_j & low(i)),  low(i) = bits 0 .. i-1, column 0 = (ones, 0).
// References are BLEU's prepared records, walked through ngram_wave.h's RefWalk (the refusal of a row, the record in flight,
// the length clamp, the order of request and recurrence) as in csrc/rouge_device.hip; the score
// entry is its score_launch.  The scores are double and a function of the row's integers alone, so a row's bits cannot
// depend on the launch it is part of.  No LDS, no atomics; every store is an ordinary vector store of a declared output.
#include "ngram_wave.h"

namespace {

using namespace set::ngram;

typedef unsigned long long u64;

// editdist.py EditDistance.score_from_stats: one double division of two integers
__device__ __forceinline__ double ed_sim(int dist, int len_h, int len_r) {
#pragma clang fp contract(off)
    const int m = len_h > len_r ? len_h : len_r;
    if (m <= 0) return 1.0;
    return (double)(m - dist) / (double)m;
}

__device__ __forceinline__ u64 low_bits(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

// the wave-uniform state of one column of vertical differences, m rows
struct EdCol {
    u64 Pv, Mv, mask, top;
    int dist;
    __device__ __forceinline__ void start(int m) {
        mask = low_bits(m);
        top = m > 0 ? 1ull << (m - 1) : 0ull;
        Pv = mask;
        Mv = 0;
        dist = m;
    }
    __device__ __forceinline__ void step(u64 Eq) {
        const u64 Xv = Eq | Mv;
        const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        u64 Ph = Mv | ~(Xh | Pv);
        u64 Mh = Pv & Xh;
        dist += (Ph & top) ? 1 : 0;
        dist -= (Mh & top) ? 1 : 0;
        Ph = (Ph << 1) | 1ull;
        Mh = Mh << 1;
        Pv = (Mh | ~(Xv | Ph)) & mask;
        Mv = Ph & Xv & mask;
    }
};

// One wave, one hypothesis against the references of its set (RefWalk, the order-1 word of a position): the next reference's
// record is requested before the current one's recurrence runs.
__global__ __launch_bounds__(64) void ed_score_k(const int64_t* hyp, long long ld, const int* lens, int L, const int* set_of,
                                                 const uint64_t* ref_recs, int ref_L, long long n_refs, const int64_t* set_off,
                                                 int n_sets, int max_set, int* stats, double* scores, double* pairs,
                                                 long long pair_ld) {
    const int lane = threadIdx.x & 63;
    const long long i = blockIdx.x;
    RefWalk<KeyOrder1> W;
    if (!W.open(i, set_of, ref_recs, ref_L, n_refs, set_off, n_sets, max_set, pairs, pair_ld)) return refuse_row(i, stats, 4, scores, 1);
    WaveSent S;
    wave_read(hyp, ld, lens, i, L, 1, S);
    const unsigned f = (unsigned)S.key[0];                         // this position's field, 0 at and beyond the length
    // the chosen reference; an empty set: the distance to no words, no reference
    int b_dist = S.len, b_len = 0, b_ref = -1;
    long long b_num = 0, b_den = 1;
    W.each(S.bad, [&](long long k, int rlen, const KeyOrder1& key) {
        const unsigned g = (unsigned)key.w;
        EdCol C;                                                  // wave-uniform: the compiler keeps it in scalar registers
        C.start(rlen);
        if (rlen > 0) {
            for (int j = 0; j < S.len; ++j) {
                const unsigned fj = (unsigned)__builtin_amdgcn_readlane((int)f, j);
                C.step(__ballot(g == fj));
            }
        } else {
            C.dist = S.len;
        }
        // the larger similarity, as fractions: (m - d) / m, both empty 1 / 1; the first of equal ones stays
        const int m = S.len > rlen ? S.len : rlen;
        const long long num = m > 0 ? m - C.dist : 1, den = m > 0 ? m : 1;
        if (k == 0 || num * b_den > b_num * den) {
            b_num = num;
            b_den = den;
            b_dist = C.dist;
            b_len = rlen;
            b_ref = (int)k;
        }
        W.put_pair(k, [&] { return ed_sim(C.dist, S.len, rlen); });
    });
    if (lane < 4) stats[i * 4 + lane] = W.bad ? -1 : lane == 0 ? b_dist : lane == 1 ? S.len : lane == 2 ? b_len : b_ref;
    if (scores && lane == 0) scores[i] = W.bad ? quiet_nan() : ed_sim(b_dist, S.len, b_len);
}

__device__ __forceinline__ u64 read_lane64(u64 v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// One wave, one (source, hypothesis) pair: the source lies along the rows (one position per lane), the hypothesis is walked
// column by column and lane j keeps the pair (Pv, Mv) of the column behind hypothesis position j.  The canonical walk-back of
// editdist.alignment then reads cells from those pairs: at most len_h + len_s wave-uniform steps.
__global__ __launch_bounds__(64) void ed_align_k(const int64_t* hyp, long long hyp_ld, const int* hyp_lens, int L,
                                                 const int64_t* src, long long src_ld, const int* src_lens, int src_L, int* stats,
                                                 signed char* hyp_ops, long long ops_ld, int* hyp_src, signed char* src_ops,
                                                 long long src_ops_ld) {
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x;
    WaveSent H, Sr;
    wave_read(hyp, hyp_ld, hyp_lens, row, L, 1, H);
    wave_read(src, src_ld, src_lens, row, src_L, 1, Sr);
    const unsigned f = (unsigned)H.key[0], g = (unsigned)Sr.key[0];
    const bool bad = H.bad || Sr.bad;
    const int len_h = H.len, len_s = Sr.len;
    EdCol C;
    C.start(len_s);
    u64 colP = 0, colM = 0;                                        // lane j: the column behind hypothesis position j
    if (len_s > 0) {
        for (int j = 0; j < len_h; ++j) {
            const unsigned fj = (unsigned)__builtin_amdgcn_readlane((int)f, j);
            C.step(__ballot(g == fj));
            colP = lane == j ? C.Pv : colP;
            colM = lane == j ? C.Mv : colM;
        }
    } else {
        C.dist = len_h;                                            // no row below row 0: every column pair stays (0, 0)
    }
    // the walk-back from (len_s, len_h): wave-uniform masks of positions, lane j-1 records its source position
    u64 h_keep = 0, h_sub = 0, h_ins = 0, s_keep = 0, s_sub = 0, s_del = 0;
    int my_src = -1;
    int i = len_s, j = len_h;
    u64 Pc = ~0ull, Mc = 0;                                        // column j; column 0 is (ones, 0): D[i][0] = i
    if (j > 0) {
        Pc = read_lane64(colP, j - 1);
        Mc = read_lane64(colM, j - 1);
    }
    for (int step = 0; step < 2 * NG_MAXL && (i > 0 || j > 0); ++step) {
        u64 Pp = ~0ull, Mp = 0;                                    // column j - 1
        if (j > 1) {
            Pp = read_lane64(colP, j - 2);
            Mp = read_lane64(colM, j - 2);
        }
        const int Dij = j + __popcll(Pc & low_bits(i)) - __popcll(Mc & low_bits(i));
        int op = 4;                                                // 1 keep, 2 substitute, 3 insert, 4 delete
        if (i > 0 && j > 0) {
            const int Dd = (j - 1) + __popcll(Pp & low_bits(i - 1)) - __popcll(Mp & low_bits(i - 1));
            const unsigned gs = (unsigned)__builtin_amdgcn_readlane((int)g, i - 1);
            const unsigned fh = (unsigned)__builtin_amdgcn_readlane((int)f, j - 1);
            if (gs == fh && Dij == Dd) op = 1;
            else if (Dij == Dd + 1) op = 2;
        }
        if (op == 4 && j > 0) {
            const int Dl = (j - 1) + __popcll(Pp & low_bits(i)) - __popcll(Mp & low_bits(i));
            if (Dij == Dl + 1 || i == 0) op = 3;
        }
        if (op <= 2) {
            const u64 hb = 1ull << (j - 1), sb = 1ull << (i - 1);
            if (op == 1) { h_keep |= hb; s_keep |= sb; } else { h_sub |= hb; s_sub |= sb; }
            my_src = lane == j - 1 ? i - 1 : my_src;
            --i;
            --j;
            Pc = Pp;
            Mc = Mp;
        } else if (op == 3) {
            h_ins |= 1ull << (j - 1);
            --j;
            Pc = Pp;
            Mc = Mp;
        } else {
            s_del |= 1ull << (i - 1);
            --i;
        }
    }
    const u64 me = 1ull << lane;
    if (lane < L) {
        const int op = bad ? 0 : (h_keep & me) ? 1 : (h_sub & me) ? 2 : (h_ins & me) ? 3 : 0;
        hyp_ops[row * ops_ld + lane] = (signed char)op;
        hyp_src[row * ops_ld + lane] = bad ? -1 : my_src;
    }
    if (lane < src_L) {
        const int op = bad ? 0 : (s_keep & me) ? 1 : (s_sub & me) ? 2 : (s_del & me) ? 3 : 0;
        src_ops[row * src_ops_ld + lane] = (signed char)op;
    }
    if (lane < 8) {
        const int keep = __popcll(h_keep), sub = __popcll(h_sub), ins = __popcll(h_ins), del = __popcll(s_del);
        const int v = lane == 0 ? C.dist : lane == 1 ? len_h : lane == 2 ? len_s : lane == 3 ? keep : lane == 4 ? sub :
                      lane == 5 ? ins : lane == 6 ? del : (C.dist == 0 ? 1 : 0);
        stats[row * 8 + lane] = bad ? -1 : v;
    }
}

}  // namespace

extern "C" {

int set_edit_device_score(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L, const int32_t* set_of_hyp,
                          const void* ref_recs, int ref_L, int64_t n_refs, const int64_t* ref_set_off, int n_sets, int max_set,
                          int32_t* stats, double* scores, double* pair_scores, int64_t pair_ld, void* stream) {
    return score_launch<>("edit_score", ed_score_k, true, hyp, hyp_ld, hyp_lens, n_hyp, L, set_of_hyp, ref_recs, ref_L, n_refs,
                          ref_set_off, n_sets, max_set, stats, scores, pair_scores, pair_ld, stream);
}

int set_edit_device_align(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n, int L, const int64_t* src,
                          int64_t src_ld, const int32_t* src_lens, int src_L, int32_t* stats, int8_t* hyp_ops, int64_t ops_ld,
                          int32_t* hyp_src, int8_t* src_ops, int64_t src_ops_ld, void* stream) {
    if (n < 0 || L < 1 || src_L < 1 || hyp_ld < L || src_ld < src_L || ops_ld < L || src_ops_ld < src_L ||
        (n > 0 && (!hyp || !src || !stats || !hyp_ops || !hyp_src || !src_ops)))
        return SET_ERR_ARG;
    if (L > NG_MAXL || src_L > NG_MAXL) return SET_ERR_UNSUPPORTED;
    if (n == 0) return SET_OK;
    set::ProfScope prof("edit_align", static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(ed_align_k, dim3((unsigned)n), dim3(64), 0, static_cast<hipStream_t>(stream), hyp, (long long)hyp_ld,
                       hyp_lens, L, src, (long long)src_ld, src_lens, src_L, stats, reinterpret_cast<signed char*>(hyp_ops),
                       (long long)ops_ld, hyp_src, reinterpret_cast<signed char*>(src_ops), (long long)src_ops_ld);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

}  // extern "C"
