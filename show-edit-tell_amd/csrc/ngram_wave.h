// What the sentence metrics share (csrc/ciderd_device.hip, csrc/bleu_device.hip, csrc/rouge_device.hip, csrc/editdist_device.hip,
// csrc/ciderd_host.hip): the packing of an n-gram into one 64-bit key, the hash of such a key, the two limits, the
// prepared-reference record of BLEU, ROUGE-L and edit distance, the device leaves that turn one row of ids into one wave's keys,
// the walk of a hypothesis over the records of its reference set (RefWalk: the one place where ROUGE-L and edit distance state
// the refusal of a row, the record in flight, the length clamp and the order "request record r + 1, then work on record r";
// bl_score_k keeps its own loop, see csrc/bleu_device.hip) and the one host launcher of the three record-reading score entries
// (score_launch).  The rules stated here are the contract between the four metrics on
// the device, the host scorers, the reward mix and evaluate.consensus_rerank; device_metric.py states the same two limits and
// the 0 rule for the Python side.
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

// record of one prepared reference, in 8-byte words (written by csrc/bleu_device.hip bl_prepare_k; read there by bl_score_k and,
// through RefWalk below, by rg_score_k and ed_score_k, which need words 0, 1 and the order-1 key of every position):
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

// ---- the walk of one hypothesis over the reference records of its set (rg_score_k, ed_score_k) -----------------------------------
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// What a refused row gets (set_range said no): -1 in its n_stats statistics, NaN in its n_scores scores, nothing else touched.
__device__ __forceinline__ void refuse_row(long long i, int* stats, int n_stats, double* scores, int n_scores) {
    const int lane = threadIdx.x & 63;
    if (lane < n_stats) stats[i * n_stats + lane] = -1;
    if (scores && lane < n_scores) scores[i * n_scores + lane] = quiet_nan();
}

// How much of a position's 32-byte key block a lane keeps of a record: the order-1 word, the position's field id + 1 (ROUGE-L,
// edit distance).  `pos`: the block of this lane's position, read only where `in`.
struct KeyOrder1 {
    uint64_t w = 0;
    __device__ __forceinline__ void load(const uint64_t* pos, bool in) { w = in ? pos[0] : 0; }
};

// One wave, hypothesis i, the records [r0, r1) of its set in order.  open() decides the range and requests the first record, so
// that it travels underneath the caller's read of the hypothesis; each() hands the records over one by one.  Everything is
// inlined into the kernel: what the body keeps wave-uniform (ROUGE-L's V, edit distance's EdCol) stays in scalar registers.
template <class Key>
struct RefWalk {
    const uint64_t* recs;
    size_t words;
    int ref_L;
    long long i, r0, r1;
    double* pairs;
    long long pair_ld;
    Key nkey;                                  // the record in flight: the lane's keys, the length word, the bad word
    uint64_t nlen = 0, nbad = 0;
    bool bad = false;                          // an id that cannot be packed, in the hypothesis or in a record handed over so far

    __device__ __forceinline__ void request(long long r) {
        const uint64_t* rv = recs + (size_t)r * words;
        const int lane = threadIdx.x & 63;
        nlen = rv[0];
        nbad = rv[1];
        nkey.load(rv + 8 + 4 * lane, lane < ref_L);
    }

    // false: the row is refused; the caller marks it (refuse_row) and returns
    __device__ __forceinline__ bool open(long long row, const int* set_of, const uint64_t* ref_recs, int ref_L_, long long n_refs,
                                         const int64_t* set_off, int n_sets, int max_set, double* pairs_, long long pair_ld_) {
        if (!set_range(set_of, row, set_off, n_sets, n_refs, max_set, r0, r1)) return false;
        i = row;
        recs = ref_recs;
        ref_L = ref_L_;
        words = ref_rec_words(ref_L_);
        pairs = pairs_;
        pair_ld = pair_ld_;
        if (r0 < r1) request(r0);
        return true;
    }

    // For r = r0 .. r1 - 1: in flight -> current (keys, length clamped to [0, ref_L], bad accumulated), stage(key) (a hook
    // for a kernel with work of its own before the next request; ROUGE-L and edit distance have none), the request of record r + 1, and only then
    // body(r - r0, rlen, key), the metric's recurrence or count.
    template <class Stage, class Body>
    __device__ __forceinline__ void each(bool hyp_bad, Stage stage, Body body) {
        bad = hyp_bad;
        for (long long r = r0; r < r1; ++r) {
            const Key key = nkey;
            const int rlen = (int)nlen < ref_L ? ((int)nlen < 0 ? 0 : (int)nlen) : ref_L;
            bad = bad || nbad != 0;
            stage(key);
            if (r + 1 < r1) request(r + 1);
            body(r - r0, rlen, key);
        }
    }
    template <class Body>
    __device__ __forceinline__ void each(bool hyp_bad, Body body) { each(hyp_bad, [](const Key&) {}, body); }

    // the hypothesis against reference k of its set alone, where the caller asked for pairs: NaN once bad, else value(), which
    // is asked of lane 0 only (a wave-level operation belongs in front of this call)
    template <class Value>
    __device__ __forceinline__ void put_pair(long long k, Value value) const {
        if (pairs && (threadIdx.x & 63) == 0) pairs[i * pair_ld + k] = bad ? quiet_nan() : value();
    }
};

// The kernels above the walk take the score entries' parameters in the entries' order; X: what an entry adds between max_set and
// stats (ROUGE-L: beta^2).
template <class... X>
using score_kernel_t = void (*)(const int64_t*, long long, const int*, int, const int*, const uint64_t*, int, long long, const int64_t*,
                                int, int, X..., int*, double*, double*, long long);

// The one body of set_bleu_device_score, set_rouge_device_score and set_edit_device_score: a null stats or the entry's own
// refusal (own_ok false) first, then score_args_check, then nothing to do for no hypothesis, then the launch, one wave a row.
template <class... X>
inline int score_launch(const char* tag, score_kernel_t<X...> kernel, bool own_ok, const int64_t* hyp, int64_t hyp_ld,
                        const int32_t* hyp_lens, int n_hyp, int L, const int32_t* set_of_hyp, const void* ref_recs, int ref_L,
                        int64_t n_refs, const int64_t* ref_set_off, int n_sets, int max_set, int32_t* stats, double* scores,
                        double* pair_scores, int64_t pair_ld, void* stream, X... extra) {
    if ((n_hyp > 0 && !stats) || !own_ok) return SET_ERR_ARG;
    SET_TRY(score_args_check(hyp, hyp_ld, n_hyp, L, set_of_hyp, ref_recs, ref_L, n_refs, ref_set_off, n_sets, max_set, pair_scores, pair_ld));
    if (n_hyp == 0) return SET_OK;
    set::ProfScope prof(tag, static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_hyp), dim3(64), 0, static_cast<hipStream_t>(stream), hyp, (long long)hyp_ld, hyp_lens,
                       L, set_of_hyp, static_cast<const uint64_t*>(ref_recs), ref_L, (long long)n_refs, ref_set_off, n_sets, max_set,
                       extra..., stats, scores, pair_scores, (long long)pair_ld);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

}  // namespace ngram
}  // namespace set
