// Host-side CIDEr-D for the self-critical reward (editnet_rl.py:611-646 calls an external,
// un-vendored Python scorer per batch).  No device code here: scoring is per-sample string/n-gram work that shards
// with the batch, but at 5 samples per image it was HALF of the SCST step's wall time in Python (74 of 147 ms at
// B = 64), so the hot part — n-gram counting, tf-idf vectors, clipped cosine with the length penalty — is native:
//
//   g_n(s)      = tf(ngram) * (log N_docs - log max(1, df(ngram)))                      n = 1..4
//   sim_n(c, r) = sum_ngram min(g(c), g(r)) * g(r) / (|g(c)| |g(r)|) * exp(-(l_c - l_r)^2 / (2 sigma^2))
//   CIDEr-D(c)  = 10 / (n |refs|) * sum_n sum_r sim_n(c, r),      l = number of bigrams
//
// Sentences arrive as int64 token ids (the Python wrapper interns token strings); an n-gram is a (length, 4 ids) key.
// The Python implementation in ciderd.py stays as the readable statement of the metric and as the cross-check.
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>
#include <algorithm>
#include <cstdlib>
#include <thread>
#include "ngram_wave.h"

namespace {

// An n-gram key.  Wide: (length, 4 ids).  Packed: when every interned token id is below the pack limit of csrc/ngram_wave.h (any
// realistic caption vocabulary) the four ids + 1 fit one 64-bit word — sorting, comparing and hashing a sentence's n-grams then
// works on plain integers (3x faster scoring than with the 40-byte key).  The packing and the hash are the device scorers'.
struct Gram {
    int64_t t[4];
    int32_t n;
    bool operator==(const Gram& o) const { return n == o.n && t[0] == o.t[0] && t[1] == o.t[1] && t[2] == o.t[2] && t[3] == o.t[3]; }
    bool operator<(const Gram& o) const {
        if (n != o.n) return n < o.n;
        for (int i = 0; i < 4; ++i) if (t[i] != o.t[i]) return t[i] < o.t[i];
        return false;
    }
};
struct GramHash {
    size_t operator()(const Gram& g) const {
        uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)(g.n + 1);
        for (int i = 0; i < 4; ++i) {
            h ^= (uint64_t)g.t[i] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
            h *= 0xBF58476D1CE4E5B9ull;
        }
        return (size_t)(h ^ (h >> 31));
    }
};
struct U64Hash {
    size_t operator()(uint64_t x) const { return (size_t)set::ngram::hash(x); }
};
inline Gram make_key(const int64_t* tok, int k, Gram*) {
    Gram g{{0, 0, 0, 0}, k};
    for (int j = 0; j < k; ++j) g.t[j] = tok[j];
    return g;
}
inline uint64_t make_key(const int64_t* tok, int k, uint64_t*) { return set::ngram::make_key(tok, k); }
using set::ngram::packable;

template <class K>
struct Vec {                                   // tf-idf vector of one sentence, per n-gram order
    std::vector<std::pair<K, double>> w[4];    // sorted by key
    double norm[4];
    long length;                               // number of bigrams (the length the public implementations use)
};

template <class K, class H>
struct Table {
    std::unordered_map<K, double, H> df;

    // n-gram counts by sort + run-length (a sentence has at most 4 * len grams: no per-sentence hash map), one df
    // lookup per DISTINCT gram; `scratch` is reused across the sentences of one thread
    void vectorise(const int64_t* tok, int64_t len, Vec<K>& v, std::vector<K>& scratch, int n, double log_ref_len) const {
        for (int k = 0; k < 4; ++k) { v.w[k].clear(); v.norm[k] = 0.0; }
        v.length = 0;
        for (int k = 1; k <= n; ++k) {
            scratch.clear();
            for (int64_t i = 0; i + k <= len; ++i) scratch.push_back(make_key(tok + i, k, (K*)nullptr));
            std::sort(scratch.begin(), scratch.end());
            double s = 0.0;
            for (size_t i = 0; i < scratch.size();) {
                size_t j = i + 1;
                while (j < scratch.size() && scratch[j] == scratch[i]) ++j;
                const int cnt = (int)(j - i);
                auto it = df.find(scratch[i]);
                const double d = it == df.end() ? 0.0 : it->second;
                const double w = (double)cnt * (log_ref_len - std::log(std::max(1.0, d)));
                v.w[k - 1].emplace_back(scratch[i], w);                // already in key order
                s += w * w;                                             // fixed (key) order: deterministic
                if (k == 2) v.length += cnt;
                i = j;
            }
            v.norm[k - 1] = std::sqrt(s);
        }
    }

    static void similarity(const Vec<K>& h, const Vec<K>& r, double* out, int n, double sigma) {
        const double delta = (double)(h.length - r.length);
        const double penalty = std::exp(-(delta * delta) / (2.0 * sigma * sigma));
        for (int k = 0; k < n; ++k) {
            double s = 0.0;
            size_t i = 0, j = 0;
            const auto& a = h.w[k];
            const auto& b = r.w[k];
            while (i < a.size() && j < b.size()) {                      // both sorted by key: merge join
                if (a[i].first < b[j].first) ++i;
                else if (b[j].first < a[i].first) ++j;
                else { s += std::min(a[i].second, b[j].second) * b[j].second; ++i; ++j; }
            }
            if (h.norm[k] != 0.0 && r.norm[k] != 0.0) s /= h.norm[k] * r.norm[k];
            out[k] += s * penalty;
        }
    }

    int score(const int64_t* hyp_tokens, const int64_t* hyp_off, int n_hyp, const int32_t* set_of_hyp,
              const int64_t* ref_tokens, const int64_t* ref_off, const int64_t* ref_set_off, int n_sets, double* scores, int n,
              double log_ref_len, double sigma) const {
        const int64_t n_refs = n_sets > 0 ? ref_set_off[n_sets] : 0;
        std::vector<Vec<K>> rv((size_t)n_refs);
        // sentences are independent: a few host threads (the caller holds no lock: ctypes releases the GIL); every score
        // is computed by exactly one thread in a fixed order, so the result does not depend on the thread count
        const int64_t work = n_refs + n_hyp;
        unsigned hw = std::thread::hardware_concurrency();
        int nthreads = (int)std::min<int64_t>(std::min<unsigned>(hw ? hw : 1u, 4u), std::max<int64_t>(1, work / 200));   // 960 sentences: 1.7 ms on one thread, 1.3 on four
        if (const char* e = getenv("SET_CIDERD_THREADS")) nthreads = std::max(1, atoi(e));
        auto run = [&](auto&& fn, int64_t count) {
            if (nthreads <= 1 || count < 2) { std::vector<K> scratch; for (int64_t i = 0; i < count; ++i) fn(i, scratch); return; }
            std::vector<std::thread> th;
            for (int t = 0; t < nthreads; ++t)
                th.emplace_back([&, t] {
                    std::vector<K> scratch;
                    for (int64_t i = t; i < count; i += nthreads) fn(i, scratch);
                });
            for (auto& x : th) x.join();
        };
        run([&](int64_t r, std::vector<K>& scratch) {
            vectorise(ref_tokens + ref_off[r], ref_off[r + 1] - ref_off[r], rv[(size_t)r], scratch, n, log_ref_len);
        }, n_refs);
        run([&](int64_t i, std::vector<K>& scratch) {
            Vec<K> hv;
            const int s = set_of_hyp[i];
            vectorise(hyp_tokens + hyp_off[i], hyp_off[i + 1] - hyp_off[i], hv, scratch, n, log_ref_len);
            double tot[4] = {0.0, 0.0, 0.0, 0.0};
            const int64_t r0 = ref_set_off[s], r1 = ref_set_off[s + 1];
            for (int64_t r = r0; r < r1; ++r) similarity(hv, rv[(size_t)r], tot, n, sigma);
            double mean = 0.0;
            for (int k = 0; k < n; ++k) mean += tot[k];
            mean /= (double)n;
            scores[i] = mean / (double)std::max<int64_t>(1, r1 - r0) * 10.0;
        }, n_hyp);
        return SET_OK;
    }
};

struct Scorer {
    Table<Gram, GramHash> wide;                // always filled
    Table<uint64_t, U64Hash> packed;           // filled when every df token id is packable
    bool packable = true;
    double log_ref_len, sigma;
    int n;
};

}  // namespace

extern "C" {

void* set_ciderd_create(const int64_t* tokens, const int32_t* lens, const double* df, int64_t n_entries, double ref_len,
                        int n, double sigma) {
    if (n < 1 || n > 4 || ref_len <= 0.0 || n_entries < 0 || (n_entries > 0 && (!tokens || !lens || !df))) return nullptr;
    Scorer* s = new Scorer();
    s->n = n;
    s->sigma = sigma;
    s->log_ref_len = std::log(ref_len);
    s->wide.df.reserve((size_t)n_entries * 2 + 16);
    for (int64_t i = 0; i < n_entries && s->packable; ++i)
        for (int j = 0; j < lens[i] && j < 4; ++j)
            if (!packable(tokens[4 * i + j])) s->packable = false;
    if (s->packable) s->packed.df.reserve((size_t)n_entries * 2 + 16);
    for (int64_t i = 0; i < n_entries; ++i) {
        if (lens[i] < 1 || lens[i] > 4) continue;
        s->wide.df[make_key(tokens + 4 * i, lens[i], (Gram*)nullptr)] = df[i];
        if (s->packable) s->packed.df[make_key(tokens + 4 * i, lens[i], (uint64_t*)nullptr)] = df[i];
    }
    return s;
}

void set_ciderd_destroy(void* h) { delete static_cast<Scorer*>(h); }

// hypothesis i = hyp_tokens[hyp_off[i] .. hyp_off[i+1]); its reference set = set_of_hyp[i]; set s holds the references
// r in [ref_set_off[s], ref_set_off[s+1]); reference r = ref_tokens[ref_off[r] .. ref_off[r+1]).  scores (n_hyp) doubles.
int set_ciderd_score(void* h, const int64_t* hyp_tokens, const int64_t* hyp_off, int n_hyp, const int32_t* set_of_hyp,
                     const int64_t* ref_tokens, const int64_t* ref_off, const int64_t* ref_set_off, int n_sets,
                     double* scores) {
    if (!h || n_hyp < 0 || n_sets < 0 || (n_hyp > 0 && (!hyp_off || !set_of_hyp || !scores)) ||
        (n_sets > 0 && (!ref_off || !ref_set_off)))
        return SET_ERR_ARG;
    const Scorer& S = *static_cast<Scorer*>(h);
    for (int i = 0; i < n_hyp; ++i)
        if (set_of_hyp[i] < 0 || set_of_hyp[i] >= n_sets) return SET_ERR_ARG;
    const int64_t n_refs = n_sets > 0 ? ref_set_off[n_sets] : 0;
    bool small = S.packable;                                  // sentence tokens may be words the df table never saw
    for (int64_t k = 0, e = n_hyp > 0 ? hyp_off[n_hyp] : 0; small && k < e; ++k) small = packable(hyp_tokens[k]);
    for (int64_t k = 0, e = n_refs > 0 ? ref_off[n_refs] : 0; small && k < e; ++k) small = packable(ref_tokens[k]);
    if (small)
        return S.packed.score(hyp_tokens, hyp_off, n_hyp, set_of_hyp, ref_tokens, ref_off, ref_set_off, n_sets, scores, S.n,
                              S.log_ref_len, S.sigma);
    return S.wide.score(hyp_tokens, hyp_off, n_hyp, set_of_hyp, ref_tokens, ref_off, ref_set_off, n_sets, scores, S.n,
                        S.log_ref_len, S.sigma);
}

}  // extern "C"
