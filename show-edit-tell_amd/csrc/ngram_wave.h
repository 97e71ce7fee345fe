// What the sentence metrics share (csrc/ciderd_device.hip, csrc/bleu_device.hip, csrc/rouge_device.hip, csrc/ciderd_host.hip):
// the packing of an n-gram into one 64-bit key, the hash of such a key, the two limits, the prepared-reference record of BLEU
// and ROUGE-L, and the device leaves that turn one row of ids into one wave's keys.  The rules stated here are the contract between CIDEr-D and BLEU on the device, the host scorer, the reward mix and
// evaluate.consensus_rerank; device_metric.py states the same two limits and the 0 rule for the Python side.
//
// A sentence is at most NG_MAXL ids: ONE WAVE holds it, one position per lane, and lane i owns the (up to) four grams that start
// at position i.  A gram of k ids is packed as id + 1 in 16-bit fields, so 0 is "no gram" and the length is implied.
#pragma once
#include "set_common.h"

namespace set {
namespace ngram {

constexpr int NG_MAXL = 64;                    // one position per lane
constexpr int64_t NG_PACK_LIMIT = 65534;       // ids + 1 must fit 16 bits and stay below 0xFFFF

__host__ __device__ inline bool packable(int64_t id) { return id >= 0 && id < NG_PACK_LIMIT; }

__host__ __device__ inline uint64_t make_key(const int64_t* tok, int k) {
    uint64_t g = 0;
    for (int j = 0; j < k; ++j) g |= (uint64_t)(tok[j] + 1) << (16 * j);
    return g;
}

__host__ __device__ inline uint64_t hash(uint64_t x) {         // the 64-bit mix of the host table and of the device probe
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// record of one prepared reference, in 8-byte words (written by csrc/bleu_device.hip bl_prepare_k; read there and by
// csrc/rouge_device.hip and csrc/editdist_device.hip, which need words 0, 1 and the order-1 key of every position):
//   [0] length   [1] 1: an id that cannot be packed   [2..7] 0
//   [8 + 4 i + k]  key of the order-(k+1) gram that starts at position i (0: none), EVERY occurrence (counts need them)
__host__ __device__ inline size_t ref_rec_words(int L) { return 8 + 4 * (size_t)L; }

// The argument checks that the score entries of the metrics share (include/set_hip.h: the same parameters under the same names);
// an entry checks its own pointers (handle, scores, stats) BEFORE this, so that a bad argument wins over an unsupported length.
inline int score_args_check(const void* hyp, int64_t hyp_ld, int n_hyp, int L, const void* set_of_hyp, const void* ref_recs, int ref_L,
                            int64_t n_refs, const void* ref_set_off, int n_sets, int max_set, const void* pair_scores, int64_t pair_ld) {
    if (n_hyp < 0 || n_sets < 0 || n_refs < 0 || max_set < 0 || L < 1 || ref_L < 1 || !ref_set_off ||
        (n_hyp > 0 && (!hyp || !set_of_hyp || hyp_ld < L)) || (n_refs > 0 && !ref_recs) || (pair_scores && pair_ld < max_set))
        return SET_ERR_ARG;
    if (L > NG_MAXL || ref_L > NG_MAXL) return SET_ERR_UNSUPPORTED;
    return SET_OK;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) {                   // fixed shape: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct WaveSent {
    uint64_t key[4];                           // this lane's grams of order 1..4, 0: none
    int len;
    bool bad;                                  // an id that cannot be packed inside the sentence
};

// One wave, row i of `tokens` (L <= NG_MAXL ids, leading dimension ld) -> the keys of the grams that start at this lane, up to
// order n.  lens == nullptr: the decoder's rule (cut after the first 0, the 0 stays; no 0: the whole row); else the row is
// lens[i] ids long, clamped to [0, L].
__device__ __forceinline__ void wave_read(const int64_t* tokens, long long ld, const int* lens, long long i, int L, int n, WaveSent& S) {
    const int lane = threadIdx.x & 63;
    const int64_t t = lane < L ? tokens[i * ld + lane] : 1;
    int len;
    if (lens) {
        const int given = lens[i] < 0 ? 0 : lens[i];
        len = given < L ? given : L;
    } else {
        const unsigned long long z = __ballot(lane < L && t == 0);
        len = z ? __ffsll((long long)z) : L;
    }
    const bool in = lane < len;
    S.len = len;
    S.bad = __any(in && !packable(t)) != 0;
    const unsigned f = (in && packable(t)) ? (unsigned)(t + 1) : 0u;
    uint64_t key = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned fk = k == 0 ? f : (unsigned)__shfl_down((int)f, k);
        key |= (uint64_t)fk << (16 * k);
        S.key[k] = (k < n && lane + k < len) ? key : 0;
    }
}

// The sentence against itself: cnt[k] = how often this lane's order-(k+1) gram occurs in the sentence, first[k] = no lower lane
// holds the same gram.  Every lane against positions 0 .. len - 1, all four orders in one pass: two 16-byte broadcast reads per
// position.  The keys behind len - k are 0 and match no gram, so a lane that holds a gram counts the len - k grams of its order.
// s_key: 2 * NG_MAXL words of this wave's LDS, free on entry; on return it holds the sentence as [position][order pair], and the
// caller puts a barrier before it writes there again.
__device__ __forceinline__ void own_grams(const WaveSent& S, ulonglong2* s_key, int cnt[4], bool first[4]) {
    const int lane = threadIdx.x & 63;
    s_key[2 * lane] = make_ulonglong2(S.key[0], S.key[1]);
    s_key[2 * lane + 1] = make_ulonglong2(S.key[2], S.key[3]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cnt[k] = 0;
        first[k] = true;
    }
    for (int j = 0; j < S.len; ++j) {
        const ulonglong2 a = s_key[2 * j], b = s_key[2 * j + 1];
        const uint64_t kj[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool same = kj[k] == S.key[k];
            cnt[k] += same ? 1 : 0;
            first[k] = first[k] && !(same && j < lane);
        }
    }
}

// The references [r0, r1) of set s; false: refused (a set index outside [0, n_sets), offsets outside the n_refs records, a set
// larger than max_set).  The host cannot see these values: the kernel marks the row and touches nothing else.
__device__ __forceinline__ bool set_range(int s, const int64_t* set_off, int n_sets, long long n_refs, int max_set, long long& r0,
                                          long long& r1) {
    r0 = 0;
    r1 = -1;
    if (s >= 0 && s < n_sets) {
        r0 = set_off[s];
        r1 = set_off[s + 1];
    }
    return !(r0 < 0 || r1 < r0 || r1 > n_refs || r1 - r0 > max_set);
}

// The references of hypothesis i's set, set_of[i].
__device__ __forceinline__ bool set_range(const int* set_of, long long i, const int64_t* set_off, int n_sets, long long n_refs,
                                          int max_set, long long& r0, long long& r1) {
    return set_range(set_of[i], set_off, n_sets, n_refs, max_set, r0, r1);
}

}  // namespace ngram
}  // namespace set
