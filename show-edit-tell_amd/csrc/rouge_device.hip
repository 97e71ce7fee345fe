// ROUGE-L on the device (include/set_hip.h set_rouge_device_score): the statistics and score of coco-caption's Rouge (beta = 1.2)
// as rouge.py states them, from id tensors in device memory: ROUGE_L for validation (evaluate.validation_rouge_l /
// validation_scores), the ROUGE-L term of the self-critical reward, and a utility for evaluate.consensus_rerank.
//
//   lcs(h, r) = length of the longest common subsequence
//   lcs_p = max_r lcs(h, r);  (lcs_r, len_r) = the reference of the largest recall lcs / len(r), compared as fractions, of equal
//   ones the first; references of no ids are skipped unless all are empty: (0, 0)
//   P = lcs_p / len(h), Rc = lcs_r / len_r;  score = (1 + beta^2) P Rc / (Rc + beta^2 P) when both are non-zero, else 0
//
// One wave holds a sentence, one position per lane (csrc/ngram_wave.h states the limits and the length rules and reads the row),
// so a set of positions is one 64-bit wave mask and the LCS is the bit-parallel recurrence of Allison & Dix / Hyyro on ONE
// wave-uniform word: lane i holds the reference's field g_i = id + 1 (0 beyond its length), V starts at all ones and for every
// hypothesis position j
//     M = ballot(g_lane == f_j);  U = V & M;  V = (V + U) | (V & ~M);           lcs = 64 - popcount(V)
// f_j >= 1 inside the hypothesis, so the 0 fields of padding never match; the carry out of bit 63 is dropped.  The lanes only
// supply the match masks: one lane read, one compare and five scalar operations per position.  References are BLEU's prepared
// records (ngram_wave.h ref_rec_words; the order-1 key of a position is its field), so one preparation serves both metrics, and
// the walk over them is ngram_wave.h's RefWalk (the refusal of a row, the record in flight, the length clamp, the order of
// request and recurrence) as in csrc/editdist_device.hip; the score entry is its score_launch.
// The score is double and a function of the row's four integers alone, so a row's bits cannot depend on the launch it is part
// of.  No LDS, no atomics; every store is an ordinary vector store of a declared output.
#include <cmath>
#include "ngram_wave.h"

namespace {

using namespace set::ngram;

// rouge.py RougeL.score_from_stats: the operations of the host in the host's order, none contracted
__device__ __forceinline__ double rg_score(int lcs_p, int len_h, int lcs_r, int len_r, double beta2) {
#pragma clang fp contract(off)
    if (lcs_p <= 0 || lcs_r <= 0 || len_h <= 0 || len_r <= 0) return 0.0;
    const double P = (double)lcs_p / (double)len_h;
    const double Rc = (double)lcs_r / (double)len_r;
    return (1.0 + beta2) * P * Rc / (Rc + beta2 * P);
}

// One wave, one hypothesis against the references of its set (RefWalk, the order-1 word of a position): the next reference's
// record is requested before the current one's recurrence runs.
__global__ __launch_bounds__(64) void rg_score_k(const int64_t* hyp, long long ld, const int* lens, int L, const int* set_of,
                                                 const uint64_t* ref_recs, int ref_L, long long n_refs, const int64_t* set_off,
                                                 int n_sets, int max_set, double beta2, int* stats, double* scores, double* pairs,
                                                 long long pair_ld) {
    const int lane = threadIdx.x & 63;
    const long long i = blockIdx.x;
    RefWalk<KeyOrder1> W;
    if (!W.open(i, set_of, ref_recs, ref_L, n_refs, set_off, n_sets, max_set, pairs, pair_ld)) return refuse_row(i, stats, 4, scores, 1);
    WaveSent S;
    wave_read(hyp, ld, lens, i, L, 1, S);
    const unsigned f = (unsigned)S.key[0];                         // this position's field, 0 at and beyond the length
    int lcs_p = 0, lcs_r = 0, len_r = 0;
    W.each(S.bad, [&](long long k, int rlen, const KeyOrder1& key) {
        const unsigned g = (unsigned)key.w;
        unsigned long long V = ~0ull;                              // wave-uniform: the compiler keeps it in scalar registers
        for (int j = 0; j < S.len; ++j) {
            const unsigned fj = (unsigned)__builtin_amdgcn_readlane((int)f, j);
            const unsigned long long M = __ballot(g == fj);
            const unsigned long long U = V & M;
            V = (V + U) | (V & ~M);
        }
        const int lcs = 64 - __popcll(V);
        lcs_p = lcs > lcs_p ? lcs : lcs_p;
        // the larger recall, as fractions: lcs / rlen > lcs_r / len_r; the first of equal ones stays
        if (rlen > 0 && (len_r == 0 || lcs * len_r > lcs_r * rlen)) {
            lcs_r = lcs;
            len_r = rlen;
        }
        W.put_pair(k, [&] { return rg_score(lcs, S.len, lcs, rlen, beta2); });
    });
    if (lane < 4) stats[i * 4 + lane] = W.bad ? -1 : lane == 0 ? lcs_p : lane == 1 ? S.len : lane == 2 ? lcs_r : len_r;
    if (scores && lane == 0) scores[i] = W.bad ? quiet_nan() : rg_score(lcs_p, S.len, lcs_r, len_r, beta2);
}

}  // namespace

extern "C" {

int set_rouge_device_score(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L, const int32_t* set_of_hyp,
                           const void* ref_recs, int ref_L, int64_t n_refs, const int64_t* ref_set_off, int n_sets, int max_set,
                           double beta, int32_t* stats, double* scores, double* pair_scores, int64_t pair_ld, void* stream) {
    return score_launch<double>("rouge_score", rg_score_k, std::isfinite(beta) && beta > 0.0, hyp, hyp_ld, hyp_lens, n_hyp, L, set_of_hyp,
                                ref_recs, ref_L, n_refs, ref_set_off, n_sets, max_set, stats, scores, pair_scores, pair_ld, stream,
                                beta * beta);
}

}  // extern "C"
