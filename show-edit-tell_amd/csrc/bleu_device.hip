// BLEU on the device (include/set_hip.h set_bleu_device_*): the statistics and scores of coco-caption's BleuScorer (n = 4,
// option "closest") as bleu.py states them, from id tensors in device memory: corpus Bleu_1..4 for validation
// (evaluate.validation_bleu), the BLEU term of the self-critical reward, and a utility for evaluate.consensus_rerank.
//
//   guess[k]   = max(0, len(h) - k + 1)                                                    k = 1..4
//   correct[k] = sum over distinct k-grams g of h: min(count_h(g), max_r count_r(g))
//   reflen     = the len(r) that minimises (|len(r) - len(h)|, len(r))
//   b *= (correct[k] + 1e-15) / (guess[k] + 1e-9);  bleu[k] = b^(1/k);  ratio = (testlen + 1e-15) / (reflen + 1e-9);
//   ratio < 1: bleu[k] *= exp(1 - 1 / ratio)
//
// One wave holds a sentence, one position per lane, and lane i owns the (up to) four packed grams that start at position i:
// csrc/ngram_wave.h states the packing, the limits and the length rules and reads the row (shared with csrc/ciderd_device.hip).
// Counts are found lane against lane through LDS, all four orders in one pass over the other sentence's length; the
// statistics are integers, the four orders' clipped counts travel through one xor-butterfly as the bytes of one word (each
// sum is at most 64).  A prepared reference is one record of ngram_wave.h's layout (ref_rec_words; csrc/rouge_device.hip reads
// the same records).  bl_score_k walks them with a loop of its own: on ngram_wave.h's RefWalk (staging hook, or the
// step in two halves) it compiled to other code that measured about 0.3 us (2 %) above the parent's spread
// (profiles/metric_walk_bench.json), so the frame that csrc/rouge_device.hip and csrc/editdist_device.hip take from RefWalk is
// written out here.  The score entry is ngram_wave.h's score_launch.  Scores are double and a function of the row's ten integers alone, so a row's bits cannot depend on the
// launch it is part of.  No atomics; every store is an ordinary vector store of a declared output.
#include <cmath>
#include "ngram_wave.h"

namespace {

using namespace set::ngram;

// bleu[1..4] from the ten integers (bleu.py Bleu.scores_from_stats); c: the four clipped counts as bytes of one word
__device__ __forceinline__ void bl_scores(int c_packed, int testlen, int reflen, double out[4]) {
    double b = 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = (c_packed >> (8 * k)) & 0xFF;
        const int g = testlen - k > 0 ? testlen - k : 0;
        b *= ((double)c + 1e-15) / ((double)g + 1e-9);
        out[k] = k == 0 ? b : pow(b, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)testlen + 1e-15) / ((double)reflen + 1e-9);
    if (ratio < 1.0) {
        const double f = exp(1.0 - 1.0 / ratio);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] *= f;
    }
}

__global__ __launch_bounds__(64) void bl_prepare_k(const int64_t* tokens, long long ld, const int* lens, int L, uint64_t* recs) {
    const int lane = threadIdx.x & 63;
    const long long i = blockIdx.x;
    WaveSent S;
    wave_read(tokens, ld, lens, i, L, 4, S);
    uint64_t* v = recs + i * (long long)ref_rec_words(L);
    if (lane < 8) v[lane] = lane == 0 ? (uint64_t)S.len : lane == 1 ? (S.bad ? 1u : 0u) : 0u;
    if (lane < L) {
        ulonglong2* p = reinterpret_cast<ulonglong2*>(v + 8 + 4 * lane);      // records are 64 bytes + 32 per position
        p[0] = make_ulonglong2(S.key[0], S.key[1]);
        p[1] = make_ulonglong2(S.key[2], S.key[3]);
    }
}

// One wave, one hypothesis against the references of its set.  The next reference's record is requested before the
// current one is counted.
__global__ __launch_bounds__(64) void bl_score_k(const int64_t* hyp, long long ld, const int* lens, int L, const int* set_of,
                                                 const uint64_t* ref_recs, int ref_L, long long n_refs, const int64_t* set_off,
                                                 int n_sets, int max_set, int* stats, double* scores, double* pairs, long long pair_ld) {
    __shared__ ulonglong2 s_key[2 * 64];                           // [position][order pair]: one sentence's keys
    const int lane = threadIdx.x & 63;
    const long long i = blockIdx.x;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    long long r0, r1;
    if (!set_range(set_of, i, set_off, n_sets, n_refs, max_set, r0, r1)) {   // -1 / NaN, nothing else touched
        if (lane < 10) stats[i * 10 + lane] = -1;
        if (scores && lane < 4) scores[i * 4 + lane] = nan;
        return;
    }
    const size_t words = ref_rec_words(ref_L);
    ulonglong2 nk0, nk1;                                           // the record in flight
    uint64_t nlen = 0, nbad = 0;
    auto request = [&](long long r) {
        const uint64_t* rv = ref_recs + (size_t)r * words;
        nlen = rv[0];
        nbad = rv[1];
        const ulonglong2* p = reinterpret_cast<const ulonglong2*>(rv + 8 + 4 * lane);
        nk0 = lane < ref_L ? p[0] : make_ulonglong2(0, 0);
        nk1 = lane < ref_L ? p[1] : make_ulonglong2(0, 0);
    };
    if (r0 < r1) request(r0);
    WaveSent S;
    wave_read(hyp, ld, lens, i, L, 4, S);
    int cnt[4];
    bool first[4], need[4];
    own_grams(S, s_key, cnt, first);
#pragma unroll
    for (int k = 0; k < 4; ++k) need[k] = S.key[k] != 0 && first[k];
    bool bad = S.bad;
    int best[4] = {0, 0, 0, 0};                                    // max over the references of the gram's count there
    int reflen = 0;
    long long ref_dist = -1;
    for (long long r = r0; r < r1; ++r) {
        __syncthreads();
        s_key[2 * lane] = nk0;
        s_key[2 * lane + 1] = nk1;
        const int rlen = (int)nlen < ref_L ? ((int)nlen < 0 ? 0 : (int)nlen) : ref_L;
        bad = bad || nbad != 0;
        __syncthreads();
        if (r + 1 < r1) request(r + 1);
        int m[4] = {0, 0, 0, 0};
        for (int j = 0; j < rlen; ++j) {                           // keys behind rlen - k are 0 and match no gram
            const ulonglong2 a = s_key[2 * j], b = s_key[2 * j + 1];
            const uint64_t kj[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] += kj[k] == S.key[k] ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) best[k] = m[k] > best[k] ? m[k] : best[k];
        const long long d = rlen > S.len ? rlen - S.len : S.len - rlen;
        if (ref_dist < 0 || d < ref_dist || (d == ref_dist && rlen < reflen)) {
            ref_dist = d;
            reflen = rlen;
        }
        if (pairs) {                                               // this reference alone
            int c = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) c |= (need[k] ? (cnt[k] < m[k] ? cnt[k] : m[k]) : 0) << (8 * k);
            c = wave_sum(c);
            double b4[4];
            bl_scores(c, S.len, rlen, b4);
            if (lane == 0) pairs[i * pair_ld + (r - r0)] = bad ? nan : b4[3];
        }
    }
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c |= (need[k] ? (cnt[k] < best[k] ? cnt[k] : best[k]) : 0) << (8 * k);
    c = wave_sum(c);
    if (lane < 10) {
        int v;
        if (lane < 4) v = bad ? -1 : (c >> (8 * lane)) & 0xFF;
        else if (lane < 8) v = S.len - (lane - 4) > 0 ? S.len - (lane - 4) : 0;
        else v = lane == 8 ? S.len : reflen;
        stats[i * 10 + lane] = v;
    }
    if (scores) {
        double b4[4];
        bl_scores(c, S.len, reflen, b4);
        if (lane < 4) scores[i * 4 + lane] = bad ? nan : lane == 0 ? b4[0] : lane == 1 ? b4[1] : lane == 2 ? b4[2] : b4[3];
    }
}

}  // namespace

extern "C" {

size_t set_bleu_device_ref_bytes(int n_refs, int L) {
    if (n_refs < 0 || L < 1 || L > NG_MAXL) return 0;
    return (size_t)n_refs * ref_rec_words(L) * sizeof(uint64_t);
}

int set_bleu_device_prepare(const int64_t* tokens, int64_t ld, const int32_t* lens, int n_refs, int L, void* recs, void* stream) {
    if (n_refs < 0 || L < 1 || (n_refs > 0 && (!tokens || !recs || ld < L))) return SET_ERR_ARG;
    if (L > NG_MAXL) return SET_ERR_UNSUPPORTED;
    if (n_refs == 0) return SET_OK;
    set::ProfScope prof("bleu_prepare", static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(bl_prepare_k, dim3((unsigned)n_refs), dim3(64), 0, static_cast<hipStream_t>(stream), tokens, (long long)ld,
                       lens, L, static_cast<uint64_t*>(recs));
    SET_LAUNCH_CHECK();
    return SET_OK;
}

int set_bleu_device_score(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L, const int32_t* set_of_hyp,
                          const void* ref_recs, int ref_L, int64_t n_refs, const int64_t* ref_set_off, int n_sets, int max_set,
                          int32_t* stats, double* scores, double* pair_scores, int64_t pair_ld, void* stream) {
    return score_launch<>("bleu_score", bl_score_k, true, hyp, hyp_ld, hyp_lens, n_hyp, L, set_of_hyp, ref_recs, ref_L, n_refs,
                          ref_set_off, n_sets, max_set, stats, scores, pair_scores, pair_ld, stream);
}

}  // extern "C"
