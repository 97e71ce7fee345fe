// The rules of a per-step beam pick once the picks are known, shared by beam_pick_k (beam.hip) and bd_merge_k (beam_constrained.hip;
// the constrained pick is its one-group case): only the first g_left picks count; the first maximum among the completions of a pick
// wins, and only if it beats the best so far; live picks are compacted to the front in pick order; completions are appended in
// pick-rank order, at most k per image; then the three-part sequence copy.  A change to a rule is made here and in pb_pick
// (beam_persistent.h).  No barriers, no LDS of its own: a kernel declares one BeamTailLds and passes it in.
#pragma once
#include "row_pick.h"

namespace set {

constexpr int BEAM_KMAX = 8;
constexpr int BEAM_NONE = 0x7fffffff;        // flat index of a pick that found no candidate

// the search state a pick updates: what the kernels' argument structs have in common
struct BeamState {
    int k, V, cur_len, Lmax;
    long long end_idx;
    float* scores;               // (NI, k) running hypothesis scores, -inf = dead slot
    int* k_left;                 // (NI)
    const long long* seqs_in;    // (NI, k, Lmax), cur_len tokens valid
    long long* seqs_out;
    float* best_score;           // (NI) best completed hypothesis so far
    long long* best_seq;         // (NI, Lmax)
    int* best_len;               // (NI)
    long long* words;            // (NI*k) next input token per hypothesis row
    int* rows;                   // (NI*k) source row of each hypothesis row's recurrent state
    // the completion list (all four nullptr for set_beam_pick_f32): every counted <end> pick appends one entry, in completion order
    // (by pick, within a pick by group, then pick rank).  An image lists at most k hypotheses
    float* done_score;           // (NI, k)
    long long* done_seq;         // (NI, k, Lmax)
    int* done_len;               // (NI, k)
    int* n_done;                 // (NI) entries so far
};

inline BeamState beam_state(int k, int V, int64_t end_idx, int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in,
                            int64_t* seqs_out, float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                            float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done) {
    return BeamState{k, V, cur_len, Lmax, end_idx, scores, k_left, (const long long*)seqs_in, (long long*)seqs_out, best_score,
                     (long long*)best_seq, best_len, (long long*)words, rows, done_score, (long long*)done_seq, done_len, n_done};
}

// what the bookkeeping leaves in LDS for the sequence copy
struct BeamTailLds {
    int src[BEAM_KMAX];                 // per output slot: parent hypothesis (slot index within the image)
    long long word[BEAM_KMAX];          // per output slot: appended word
    int copy[BEAM_KMAX];                // per output slot: its group picked at this step, the sequence is copied
    int best_parent;                    // -1: no new best
    long long best_word;
    int done_par[BEAM_KMAX];            // per completion of this step: parent hypothesis
    long long done_word[BEAM_KMAX];
    int done_at, done_n;                // first entry of this step in the image's list, entries of this step
};

// ONE thread, before the first group of an image
__device__ __forceinline__ void beam_tail_begin(const BeamState& a, int img, BeamTailLds& t) {
    t.best_parent = -1;
    t.done_n = 0;
    t.done_at = a.n_done ? max(a.n_done[img], 0) : 0;
}

// ONE thread: the bookkeeping of the g slots gbase .. gbase + g - 1 of image img.  pv / pi: the group's picks in rank order, the
// carried value and the flat index slot * V + word (BEAM_NONE: none).  Returns the group's g_left after the step.
//   EXHAUST  a group whose first pick is empty ends here: 0 left, identity rows, its sequences are not copied
//   RANK     completed hypotheses carry v / den when alpha != 0 (den = cur_len^alpha); otherwise v, with no division
//   done_group (or nullptr): the group index gi of every listed completion; s_pen / s_npen (or nullptr): the group's live words are
//   appended to the penalised-word list
template <bool EXHAUST, bool RANK>
__device__ __forceinline__ int beam_tail_group(const BeamState& a, int img, int gbase, int g, int g_left, const float* pv, const int* pi,
                                               float alpha, float den, int gi, int* done_group, int* s_pen, int* s_npen,
                                               BeamTailLds& t) {
    const int base = img * a.k, V = a.V;
    const bool exhausted = EXHAUST && pi[0] == BEAM_NONE;             // no surviving finite candidate
    int n_end = 0, c_arg = -1, slot = 0;
    float c_best = -INFINITY;
    for (int r = 0; r < g; ++r) {
        const int fl = pi[r];
        if (!(fl != BEAM_NONE && r < g_left && fl % V == a.end_idx)) continue;   // only the first g_left picks count
        float rs = pv[r];
        if (RANK) rs = alpha != 0.f ? pv[r] / den : pv[r];
        ++n_end;
        if (rs > c_best) { c_best = rs; c_arg = r; }                  // first maximum
        const int at = t.done_at + t.done_n;                          // completions in group order, then pick rank
        if (!a.n_done || at >= a.k) continue;
        a.done_score[base + at] = rs;
        a.done_len[base + at] = a.cur_len + 1;
        if (done_group) done_group[base + at] = gi;
        t.done_par[t.done_n] = fl / V;
        t.done_word[t.done_n] = fl % V;
        ++t.done_n;
    }
    if (c_arg >= 0 && c_best > a.best_score[img]) {
        a.best_score[img] = c_best;
        a.best_len[img] = a.cur_len + 1;
        t.best_parent = pi[c_arg] / V;
        t.best_word = pi[c_arg] % V;
    }
    // live picks first, in pick order; the other slots die
    for (int pass = 0; pass < 2; ++pass)
        for (int r = 0; r < g; ++r) {
            const int fl = pi[r];
            const bool live = fl != BEAM_NONE && r < g_left && fl % V != a.end_idx;
            if ((pass == 0) != live) continue;
            const int parent = fl != BEAM_NONE ? fl / V : gbase;
            const long long word = fl != BEAM_NONE ? fl % V : 0;
            const int o = gbase + slot;
            a.scores[base + o] = live ? pv[r] : -INFINITY;
            a.words[base + o] = live ? word : 0;
            a.rows[base + o] = exhausted ? base + o : base + parent;
            t.src[o] = parent;
            t.word[o] = word;
            t.copy[o] = exhausted ? 0 : 1;
            if (s_pen && live) s_pen[(*s_npen)++] = (int)word;
            ++slot;
        }
    return exhausted ? 0 : g_left - n_end;
}

// thread tid of nt, behind a barrier after the bookkeeping: seqs_out (the slots whose group picked), best_seq, done_seq
__device__ __forceinline__ void beam_tail_copy(const BeamState& a, int img, const BeamTailLds& t, int tid, int nt) {
    const int k = a.k, L = a.cur_len;
    const long long* sin = a.seqs_in + (long long)img * k * a.Lmax;
    long long* sout = a.seqs_out + (long long)img * k * a.Lmax;
    for (int e = tid; e < k * (L + 1); e += nt) {
        const int slot = e / (L + 1), q = e - slot * (L + 1);
        if (t.copy[slot]) sout[(long long)slot * a.Lmax + q] = q < L ? sin[(long long)t.src[slot] * a.Lmax + q] : t.word[slot];
    }
    if (t.best_parent >= 0)
        for (int q = tid; q <= L; q += nt)
            a.best_seq[(long long)img * a.Lmax + q] = q < L ? sin[(long long)t.best_parent * a.Lmax + q] : t.best_word;
    if (t.done_n > 0) {
        long long* dout = a.done_seq + ((long long)img * k + t.done_at) * a.Lmax;
        for (int e = tid; e < t.done_n * (L + 1); e += nt) {
            const int j = e / (L + 1), q = e - j * (L + 1);
            dout[(long long)j * a.Lmax + q] = q < L ? sin[(long long)t.done_par[j] * a.Lmax + q] : t.done_word[j];
        }
    }
}

}  // namespace set
