// CIDEr-D on the device (include/set_hip.h set_ciderd_device_*): the integer reward path of ciderd.py score_token_ids
// (ciderd.py:211-250) and csrc/ciderd_host.hip Table::vectorise / similarity / score (ciderd_host.hip:77-156) without the
// host trip, and the same kernel with device-resident candidates as each other's references (evaluate.consensus_rerank).
//
//   g_n(s)      = tf(ngram) * (log N_docs - log max(1, df(ngram)))                      n = 1..4
//   sim_n(c, r) = sum_ngram min(g(c), g(r)) * g(r) / (|g(c)| |g(r)|) * exp(-(l_c - l_r)^2 / (2 sigma^2))
//   CIDEr-D(c)  = 10 / (n |refs|) * sum_n sum_r sim_n(c, r),      l = number of bigrams
//
// One wave holds a sentence, one position per lane, and lane i owns the (up to) four packed n-grams that start at position i:
// csrc/ngram_wave.h states the packing (the host scorer's), the limits and the length rules, reads the row and finds the
// duplicate grams of a sentence by comparing every lane's keys with the whole sentence's keys through LDS (no sort; shared with
// csrc/bleu_device.hip).  The first lane of a gram carries its tf and looks its document count up in
// an open-addressing table (linear probing, 16-byte {key, df} slots: one load per probe).  Everything is double; sums
// over lanes are one fixed xor-butterfly, so a row's bits do not depend on the launch it is part of.  No atomics; every
// store is an ordinary vector store of a declared output.
//
// The table comes from the host (set_ciderd_device_create: counts pickled from a training set, the SCST reward) or is built here
// from the reference sets of the corpus that is scored (set_ciderd_device_create_corpus, cd_build_k below: cocoEval's `CIDEr`,
// the same formula with df and N of the evaluated corpus).  That build is the one place with atomics: a compare-and-swap on a
// slot's key and an add on its count.
#include <cmath>
#include <cstring>
#include <vector>
#include "ngram_wave.h"

namespace {

using namespace set::ngram;

struct alignas(16) CdSlot { uint64_t key; double df; };

struct CdTable {                               // kernel argument: the device table and the metric's constants
    const CdSlot* slots;
    uint64_t mask;                             // capacity - 1 (capacity: a power of two, at least 2 * entries)
    double log_ref_len, sigma;
    int n;
};
struct CdHandle {
    CdTable t;
    CdSlot* slots;
    unsigned long long* dropped = nullptr;     // a table built on the device: the grams that found no slot (behind the slots)
};

// record of one vectorised sentence in the caller's workspace, in 8-byte words:
//   [0..3] norm of order 1..4 (double)   [4] number of bigrams   [5] length   [6] 1: an id that cannot be packed   [7] 0
//   [8 + k L + i]        key of the order-(k+1) gram that starts at position i (0: none, or a repeat of an earlier one)
//   [8 + 4 L + k L + i]  its weight tf * (log ref_len - log max(1, df)) (double; 0 where the key is 0)
__host__ __device__ inline size_t cd_vec_words(int L) { return 8 + 8 * (size_t)L; }

// the length the penalty uses: the bigrams that were counted (none with n = 1: ciderd_host.hip:94, ciderd.py:121-122)
__device__ __forceinline__ int cd_bigrams(const CdTable& T, int len) { return T.n >= 2 && len > 1 ? len - 1 : 0; }

struct CdSent : WaveSent {                     // key: kept on the first lane of each gram only
    double w[4];
    double norm[4];
};

// One wave, row i of `tokens` (ciderd_host.hip Table::vectorise); tokens, ld, lens, L as wave_read takes them.  s_key: the LDS of
// own_grams.  Block = one wave.
__device__ __forceinline__ void cd_vectorise(const CdTable& T, const int64_t* tokens, long long ld, const int* lens, long long i, int L,
                                             ulonglong2* s_key, CdSent& S) {
    const int lane = threadIdx.x & 63;
    wave_read(tokens, ld, lens, i, L, T.n, S);
    int cnt[4];
    bool need[4];                                                 // the first lane of a gram carries its tf
    own_grams(S, s_key, cnt, need);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        need[k] = need[k] && k < T.n && lane + k < S.len;
        // a gram made only of ids that cannot be packed has the key 0 (its row is refused, its record is still written): the k
        // empty entries behind len - k are not occurrences of it
        if (S.key[k] == 0) cnt[k] -= k;
        if (!need[k]) S.key[k] = 0;
    }
    // document counts: the four orders' first probes are in flight together
    uint64_t slot[4];
    CdSlot got[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        slot[k] = hash(S.key[k]) & T.mask;
        got[k] = need[k] ? T.slots[slot[k]] : CdSlot{0, 0.0};
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t left = T.mask;                                   // the table is at most half full: an empty slot ends every chain
        while (need[k] && got[k].key != S.key[k] && got[k].key != 0 && left-- > 0) {
            slot[k] = (slot[k] + 1) & T.mask;
            got[k] = T.slots[slot[k]];
        }
        const double d = (need[k] && got[k].key == S.key[k]) ? got[k].df : 0.0;
        S.w[k] = need[k] ? (double)cnt[k] * (T.log_ref_len - log(fmax(1.0, d))) : 0.0;
        S.norm[k] = sqrt(wave_sum(S.w[k] * S.w[k]));
    }
}

__global__ __launch_bounds__(64) void cd_vectorise_k(CdTable T, const int64_t* tokens, long long ld, const int* lens, int L,
                                                     uint64_t* vecs) {
    __shared__ ulonglong2 s_key[2 * 64];
    const int lane = threadIdx.x & 63;
    const long long i = blockIdx.x;
    CdSent S;
    cd_vectorise(T, tokens, ld, lens, i, L, s_key, S);
    uint64_t* v = vecs + i * (long long)cd_vec_words(L);
    if (lane < 8) {
        uint64_t h = 0;
        if (lane < 4) h = (uint64_t)__double_as_longlong(lane == 0 ? S.norm[0] : lane == 1 ? S.norm[1] : lane == 2 ? S.norm[2] : S.norm[3]);
        else if (lane == 4) h = (uint64_t)cd_bigrams(T, S.len);
        else if (lane == 5) h = (uint64_t)S.len;
        else if (lane == 6) h = S.bad ? 1 : 0;
        v[lane] = h;
    }
    if (lane < L) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[8 + k * L + lane] = S.key[k];
            v[8 + 4 * L + k * L + lane] = (uint64_t)__double_as_longlong(S.w[k]);
        }
    }
}

__global__ __launch_bounds__(64) void cd_lookup_k(CdTable T, const uint64_t* keys, long long n, double* out) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    double d = 0.0;
    if (key != 0) {
        uint64_t slot = hash(key) & T.mask, left = T.mask;
        CdSlot g = T.slots[slot];
        while (g.key != key && g.key != 0 && left-- > 0) {
            slot = (slot + 1) & T.mask;
            g = T.slots[slot];
        }
        if (g.key == key) d = g.df;
    }
    out[i] = d;
}

// One wave, one hypothesis against the references of its set (ciderd_host.hip:101-117, 143-154).  The next reference's
// record is requested before the current one is scored.
__global__ __launch_bounds__(64) void cd_score_k(CdTable T, const int64_t* hyp, long long ld, const int* lens, int L, const int* set_of,
                                                 const uint64_t* ref_vecs, int ref_L, long long n_refs, const int64_t* set_off,
                                                 int n_sets, int max_set, double* scores, double* pairs, long long pair_ld) {
    __shared__ ulonglong2 s_own[2 * 64];                           // the hypothesis against itself, then one reference's keys
    __shared__ double s_w[4 * 64];
    __shared__ uint64_t s_hdr[8];
    const int lane = threadIdx.x & 63;
    const long long i = blockIdx.x;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    long long r0, r1;
    if (!set_range(set_of, i, set_off, n_sets, n_refs, max_set, r0, r1)) {   // NaN, nothing else touched
        if (lane == 0) scores[i] = nan;
        return;
    }
    const size_t words = cd_vec_words(ref_L);
    uint64_t nk[4], nw[4], nh = 0;                                 // the record in flight
    auto request = [&](long long r) {
        const uint64_t* rv = ref_vecs + (size_t)r * words;
        nh = lane < 8 ? rv[lane] : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nk[k] = lane < ref_L ? rv[8 + k * ref_L + lane] : 0;
            nw[k] = lane < ref_L ? rv[8 + 4 * ref_L + k * ref_L + lane] : 0;
        }
    };
    if (r0 < r1) request(r0);
    CdSent S;
    cd_vectorise(T, hyp, ld, lens, i, L, s_own, S);
    uint64_t* s_key = reinterpret_cast<uint64_t*>(s_own);          // [order][position] from here on
    const long long lh = cd_bigrams(T, S.len);
    bool bad = S.bad;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long r = r0; r < r1; ++r) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_key[k * 64 + lane] = nk[k];
            s_w[k * 64 + lane] = __longlong_as_double((long long)nw[k]);
        }
        if (lane < 8) s_hdr[lane] = nh;
        __syncthreads();
        if (r + 1 < r1) request(r + 1);
        const long long lr = (long long)s_hdr[4];
        const int rlen = (int)s_hdr[5] < ref_L ? (int)s_hdr[5] : ref_L;
        bad = bad || s_hdr[6] != 0;
        const double delta = (double)(lh - lr);
        const double penalty = exp(-(delta * delta) / (2.0 * T.sigma * T.sigma));
        double pair = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < T.n) {
                const int ng = rlen - k;
                double p = 0.0;
                for (int j = 0; j < ng; ++j) {
                    const uint64_t kj = s_key[k * 64 + j];
                    const double wj = s_w[k * 64 + j];
                    if (kj == S.key[k] && kj != 0) p = fmin(S.w[k], wj) * wj;       // keys of a record are distinct
                }
                double sum = wave_sum(p);
                const double rn = __longlong_as_double((long long)s_hdr[k]);
                if (S.norm[k] != 0.0 && rn != 0.0) sum /= S.norm[k] * rn;
                tot[k] += sum * penalty;
                pair += sum * penalty;
            }
        }
        if (pairs && lane == 0) pairs[i * pair_ld + (r - r0)] = bad ? nan : pair / (double)T.n * 10.0;
    }
    double mean = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < T.n) mean += tot[k];
    mean /= (double)T.n;
    const long long cnt = r1 - r0;
    if (lane == 0) scores[i] = bad ? nan : mean / (double)(cnt > 1 ? cnt : 1) * 10.0;
}

// ---- the table of a corpus, built from its reference sets (set_ciderd_device_create_corpus) ----------------------------------
// df(g) = the number of SETS whose references hold the gram g: a gram counts once per set however often it occurs there.
//
// One gram into the table: the slot's key word goes empty -> key by a 64-bit compare-and-swap (a key never changes once it is
// set, so the relaxed load in front only spares the swap on a slot that is taken), and the lane whose slot is, or has just become,
// its key adds 1.0 to the slot's count with a double atomic add.  The count is a sum of ones below 2^53: every partial sum is an
// integer that a double holds exactly, so the order of arrival does not show in it.  Which slot a key lands in does depend on the
// order of arrival; the map key -> count does not.  A gram that finds no slot within mask + 1 probes (the caller's bound was
// too small and the table is full) is dropped and counted in *dropped.
__device__ __forceinline__ void cd_insert(CdSlot* slots, uint64_t mask, uint64_t key, unsigned long long* dropped) {
    uint64_t slot = hash(key) & mask, left = mask;
    for (;;) {
        unsigned long long* kw = reinterpret_cast<unsigned long long*>(&slots[slot].key);
        unsigned long long old = __hip_atomic_load(kw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) old = atomicCAS(kw, 0ull, (unsigned long long)key);
        if (old == 0 || old == key) {
            atomicAdd(&slots[slot].df, 1.0);
            return;
        }
        if (left-- == 0) break;
        slot = (slot + 1) & mask;
    }
    atomicAdd(dropped, 1ull);
}

// One wave per reference set.  Reference r keeps, on the first lane of each of its distinct grams (own_grams), the grams that no
// earlier reference r0 .. r - 1 of the set holds: those rows are read again (they sit in L2) and staged in LDS one sentence at a
// time, every lane against every position.  LDS is that of one sentence whatever the set size, there is no workspace; the cost is
// quadratic in the set size, which max_set bounds.  A reference with an id that cannot be packed contributes nothing and hides
// nothing (cd_score_k marks its set NaN).  A set the host could not check (set_range) touches nothing.
__global__ __launch_bounds__(64) void cd_build_k(CdSlot* slots, uint64_t mask, unsigned long long* dropped, const int64_t* tokens,
                                                 long long ld, const int* lens, int L, long long n_refs, const int64_t* set_off,
                                                 int n_sets, int max_set, int n) {
    __shared__ ulonglong2 s_key[2 * 64];
    const int lane = threadIdx.x & 63;
    long long r0, r1;
    if (!set_range((int)blockIdx.x, set_off, n_sets, n_refs, max_set, r0, r1)) return;
    for (long long r = r0; r < r1; ++r) {
        WaveSent S;
        wave_read(tokens, ld, lens, r, L, n, S);
        if (S.bad) continue;                                      // the same on every lane
        int cnt[4];
        bool keep[4];
        __syncthreads();                                          // the reads of the reference before are done
        own_grams(S, s_key, cnt, keep);
#pragma unroll
        for (int k = 0; k < 4; ++k) keep[k] = keep[k] && S.key[k] != 0;
        for (long long q = r0; q < r; ++q) {
            WaveSent Q;
            wave_read(tokens, ld, lens, q, L, n, Q);
            if (Q.bad) continue;
            __syncthreads();
            s_key[2 * lane] = make_ulonglong2(Q.key[0], Q.key[1]);
            s_key[2 * lane + 1] = make_ulonglong2(Q.key[2], Q.key[3]);
            __syncthreads();
            for (int j = 0; j < Q.len; ++j) {
                const ulonglong2 a = s_key[2 * j], b = s_key[2 * j + 1];
                const uint64_t kj[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
                for (int k = 0; k < 4; ++k) keep[k] = keep[k] && kj[k] != S.key[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (keep[k]) cd_insert(slots, mask, S.key[k], dropped);
    }
}

}  // namespace

extern "C" {

int set_ciderd_device_key(const int64_t* tokens, int k, uint64_t* key_out) {
    if (!tokens || !key_out || k < 1 || k > 4) return SET_ERR_ARG;
    for (int j = 0; j < k; ++j)
        if (!packable(tokens[j])) return SET_ERR_UNSUPPORTED;
    *key_out = make_key(tokens, k);
    return SET_OK;
}

int set_ciderd_device_create(const int64_t* tokens, const int32_t* lens, const double* df, int64_t n_entries, double ref_len,
                             int n, double sigma, void* stream, void** handle_out) {
    if (!handle_out) return SET_ERR_ARG;
    *handle_out = nullptr;
    if (n < 1 || n > 4 || !(ref_len > 0.0) || !(sigma > 0.0) || n_entries < 0 || (n_entries > 0 && (!tokens || !lens || !df)))
        return SET_ERR_ARG;
    for (int64_t i = 0; i < n_entries; ++i)
        for (int j = 0; j < lens[i] && j < 4; ++j)
            if (!packable(tokens[4 * i + j])) return SET_ERR_UNSUPPORTED;
    uint64_t cap = 2;
    while (cap < 2 * (uint64_t)n_entries) cap <<= 1;
    std::vector<CdSlot> host((size_t)cap, CdSlot{0, 0.0});
    for (int64_t i = 0; i < n_entries; ++i) {
        if (lens[i] < 1 || lens[i] > 4) continue;
        const uint64_t key = make_key(tokens + 4 * i, lens[i]);
        uint64_t slot = hash(key) & (cap - 1);
        while (host[slot].key != 0 && host[slot].key != key) slot = (slot + 1) & (cap - 1);
        host[slot] = CdSlot{key, df[i]};                           // a repeated gram: the last count stands, as on the host
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    CdSlot* dev = nullptr;
    SET_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev), (size_t)cap * sizeof(CdSlot)));
    hipError_t e = hipMemcpyAsync(dev, host.data(), (size_t)cap * sizeof(CdSlot), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);             // `host` goes away with this call
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return set::hip_fail(e);
    }
    CdHandle* h = new CdHandle();
    h->slots = dev;
    h->t = CdTable{dev, cap - 1, std::log(ref_len), sigma, n};
    *handle_out = h;
    return SET_OK;
}

int set_ciderd_device_create_corpus(const int64_t* ref_tokens, int64_t ld, const int32_t* ref_lens, int64_t n_refs, int L,
                                    const int64_t* ref_set_off, int n_sets, int max_set, int64_t gram_bound, int n, double sigma,
                                    void* stream, void** handle_out) {
    if (!handle_out) return SET_ERR_ARG;
    *handle_out = nullptr;
    if (n < 1 || n > 4 || !(sigma > 0.0) || n_sets < 1 || n_refs < 0 || max_set < 0 || gram_bound < 0 || L < 1 || ld < L ||
        !ref_set_off || (n_refs > 0 && !ref_tokens))
        return SET_ERR_ARG;
    if (L > NG_MAXL || gram_bound > ((int64_t)1 << 40)) return SET_ERR_UNSUPPORTED;
    uint64_t cap = 2;
    while (cap < 2 * (uint64_t)gram_bound) cap <<= 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CdSlot* dev = nullptr;                                         // the slots, and one more whose key word is the drop counter
    SET_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev), (size_t)(cap + 1) * sizeof(CdSlot)));
    hipError_t e = hipMemsetAsync(dev, 0, (size_t)(cap + 1) * sizeof(CdSlot), st);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return set::hip_fail(e);
    }
    CdHandle* h = new CdHandle();
    h->slots = dev;
    h->dropped = reinterpret_cast<unsigned long long*>(&dev[cap].key);
    h->t = CdTable{dev, cap - 1, std::log((double)n_sets), sigma, n};
    {
        set::ProfScope prof("ciderd_build", st);
        hipLaunchKernelGGL(cd_build_k, dim3((unsigned)n_sets), dim3(64), 0, st, dev, cap - 1, h->dropped, ref_tokens, (long long)ld,
                           ref_lens, L, (long long)n_refs, ref_set_off, n_sets, max_set, n);
    }
    e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipFree(dev);
        delete h;
        return set::hip_fail(e);
    }
    *handle_out = h;
    return SET_OK;
}

int set_ciderd_device_dropped(void* handle, int64_t* dropped_out, void* stream) {
    if (!handle || !dropped_out) return SET_ERR_ARG;
    const CdHandle* h = static_cast<const CdHandle*>(handle);
    *dropped_out = 0;
    if (!h->dropped) return SET_OK;                                // a table from the host holds every entry it was given
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long got = 0;
    SET_HIP_TRY(hipMemcpyAsync(&got, h->dropped, sizeof(got), hipMemcpyDeviceToHost, st));
    SET_HIP_TRY(hipStreamSynchronize(st));
    *dropped_out = (int64_t)got;
    return SET_OK;
}

void set_ciderd_device_destroy(void* handle) {
    CdHandle* h = static_cast<CdHandle*>(handle);
    if (!h) return;
    (void)hipFree(h->slots);
    delete h;
}

int set_ciderd_device_lookup(void* handle, const uint64_t* keys, int64_t n, double* df_out, void* stream) {
    if (!handle || n < 0 || (n > 0 && (!keys || !df_out))) return SET_ERR_ARG;
    if (n > (int64_t)0x7FFFFFFF * 64) return SET_ERR_UNSUPPORTED;
    if (n == 0) return SET_OK;
    const CdHandle* h = static_cast<const CdHandle*>(handle);
    hipLaunchKernelGGL(cd_lookup_k, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), h->t, keys,
                       (long long)n, df_out);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

size_t set_ciderd_device_vec_bytes(int n_sent, int L) {
    if (n_sent < 0 || L < 1 || L > NG_MAXL) return 0;
    return (size_t)n_sent * cd_vec_words(L) * sizeof(uint64_t);
}

int set_ciderd_device_vectorise(void* handle, const int64_t* tokens, int64_t ld, const int32_t* lens, int n_sent, int L,
                                void* vecs, void* stream) {
    if (!handle || n_sent < 0 || L < 1 || (n_sent > 0 && (!tokens || !vecs || ld < L))) return SET_ERR_ARG;
    if (L > NG_MAXL) return SET_ERR_UNSUPPORTED;
    if (n_sent == 0) return SET_OK;
    const CdHandle* h = static_cast<const CdHandle*>(handle);
    set::ProfScope prof("ciderd_vectorise", static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(cd_vectorise_k, dim3((unsigned)n_sent), dim3(64), 0, static_cast<hipStream_t>(stream), h->t, tokens,
                       (long long)ld, lens, L, static_cast<uint64_t*>(vecs));
    SET_LAUNCH_CHECK();
    return SET_OK;
}

int set_ciderd_device_score(void* handle, const int64_t* hyp_tokens, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L,
                            const int32_t* set_of_hyp, const void* ref_vecs, int ref_L, int64_t n_refs,
                            const int64_t* ref_set_off, int n_sets, int max_set, double* scores, double* pair_scores,
                            int64_t pair_ld, void* stream) {
    if (!handle || (n_hyp > 0 && !scores)) return SET_ERR_ARG;
    SET_TRY(score_args_check(hyp_tokens, hyp_ld, n_hyp, L, set_of_hyp, ref_vecs, ref_L, n_refs, ref_set_off, n_sets, max_set, pair_scores,
                             pair_ld));
    if (n_hyp == 0) return SET_OK;
    const CdHandle* h = static_cast<const CdHandle*>(handle);
    set::ProfScope prof("ciderd_score", static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(cd_score_k, dim3((unsigned)n_hyp), dim3(64), 0, static_cast<hipStream_t>(stream), h->t, hyp_tokens,
                       (long long)hyp_ld, hyp_lens, L, set_of_hyp, static_cast<const uint64_t*>(ref_vecs), ref_L,
                       (long long)n_refs, ref_set_off, n_sets, max_set, scores, pair_scores, (long long)pair_ld);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

}  // extern "C"
