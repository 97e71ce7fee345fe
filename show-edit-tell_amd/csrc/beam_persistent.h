// The pick tail of the three persistent beam searches (dcnet_persistent_k<.., BEAM> in decode_persistent.hip,
// editnet_persistent_wide_k<BEAM, ..> in decode_persistent_wide.hip, ensemble_persistent_k in decode_persistent_ensemble.hip):
// the one place that holds the rules of the pick for ONE image and k <= PW_BEAM_K hypotheses —
//   * candidates are ordered by value descending, flat index (parent * V + word) ascending among equals;
//   * of the k picks, only as many as there are live hypotheses (k_left) count, the best ones;
//   * among the hypotheses completed by one pick the FIRST maximum is kept, and only if it beats the best so far;
//   * live hypotheses are compacted to the front in pick order, the remaining slots are dead (-inf).
// The per-step picks (beam_pick_k in csrc/beam.hip, bd_merge_k in csrc/beam_constrained.hip) apply the same rules to MANY images
// per launch, up to BEAM_KMAX hypotheses and global outputs, through csrc/beam_tail.h, the other home of the rules; that tail stays
// separate from this one (sharing would take more parameters, not fewer lines).  A change to a rule is made in beam_tail.h and
// in pb_pick below.
// Everything here runs after a kernel's last MFMA of the timestep, in one wave per row and then in one thread: no weight
// tile is in flight, so — unlike the phase code, which every kernel keeps as its own copy because the order of its loads IS
// its schedule — these are plain forced-inline functions.  None of them contains a barrier: every __syncthreads() stays in
// the kernel body.  What differs between the kernels stays there too: how a lane's score is formed (log-sum-exp rescoring in
// the single-model kernels, the averaged probabilities in the ensemble) and which exchange the candidates travel in.
#pragma once
#include "decode_persistent.h"

namespace set {

// A candidate list: PW_BEAM_K (value, index) pairs in pick order, (-inf, 0x7fffffff) = no candidate.  Vector types, handed to the
// functions below by value: a list lives in registers whichever way it is indexed (an array behind a reference is memory to
// the compiler until it is inlined, and the select in pb_publish then left it in scratch memory)
typedef float pb_vals __attribute__((ext_vector_type(PW_BEAM_K)));
typedef int pb_idxs __attribute__((ext_vector_type(PW_BEAM_K)));
__device__ __forceinline__ void pb_none(pb_vals& v, pb_idxs& ix) { v = -INFINITY; ix = 0x7fffffff; }

// Slice top-k, one wave: lane l holds the score xx of candidate idx (ok = the lane holds one at all; -inf = none).  The B best
// (value, index) pairs of the 64 lanes, in order, the same in every lane; entries past B (or past the candidates) are empty.
__device__ __forceinline__ void pb_slice_topk(float xx, const int idx, const bool ok, const int B, pb_vals& cvv, pb_idxs& cii) {
#pragma unroll
    for (int q = 0; q < PW_BEAM_K; ++q) {
        float bv = -INFINITY;
        int bix = 0x7fffffff;
        if (q < B) {
            if (xx > -INFINITY) { bv = xx; bix = idx; }
            pw_wargmax(bv, bix);
            if (ok && idx == bix) xx = -INFINITY;
        }
        cvv[q] = bv; cii[q] = bix;
    }
}

// Candidate publish: the PW_BEAM_W words of one (row, slice) — two leading words of the caller's (the single-model kernels:
// max and sum exp of the slice), PW_BEAM_K x (value, index), two pads — stored by lanes 0 .. PW_BEAM_W - 1 at word0 + lane.
__device__ __forceinline__ void pb_publish(__amdgpu_buffer_rsrc_t rs, const int word0, const int lane, const float lead0,
                                           const float lead1, const pb_vals cvv, const pb_idxs cii, const unsigned tag) {
    if (lane < PW_BEAM_W) {
        float v = 0.f;
        if (lane == 0) v = lead0;
        else if (lane == 1) v = lead1;
        else if (lane < 2 + 2 * PW_BEAM_K) {
            const int q = (lane - 2) >> 1;
            float cv_ = cvv[0]; int ci_ = cii[0];
#pragma unroll
            for (int u = 1; u < PW_BEAM_K; ++u) if (q == u) { cv_ = cvv[u]; ci_ = cii[u]; }
            v = (lane & 1) ? __int_as_float(ci_) : cv_;
        }
        ll_put(rs, word0 + lane, v, tag);
    }
}

// Row merge, one wave: every lane holds 16 candidates (cv, ci) of the row (four slices of four), already scored and flat-indexed,
// (-inf, 0x7fffffff) = none.  The row's B best in order -> (ov, oi), the same in every lane; cv is consumed.
__device__ __forceinline__ void pb_row_merge(float (&cv)[16], const int (&ci)[16], const int B, pb_vals& ov, pb_idxs& oi) {
#pragma unroll
    for (int q = 0; q < PW_BEAM_K; ++q) {
        if (q < B) {
            float bv = -INFINITY;
            int bix = 0x7fffffff;
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (cv[c] > bv || (cv[c] == bv && ci[c] < bix)) { bv = cv[c]; bix = ci[c]; }
            if (!(bv > -INFINITY)) bix = 0x7fffffff;
            pw_wargmax(bv, bix);
#pragma unroll
            for (int c = 0; c < 16; ++c) if (ci[c] == bix) cv[c] = -INFINITY;
            ov[q] = bv; oi[q] = bix;
        }
    }
}
// ... and row j's list into sCand (K, K, 2): (score, flat index) of every row's best K candidates.  One lane calls this.
__device__ __forceinline__ void pb_row_store(float* sCand, const int j, const pb_vals ov, const pb_idxs oi) {
#pragma unroll
    for (int q = 0; q < PW_BEAM_K; ++q) { sCand[(j * PW_BEAM_K + q) * 2] = ov[q]; sCand[(j * PW_BEAM_K + q) * 2 + 1] = __int_as_float(oi[q]); }
}

// Pick bookkeeping, ONE thread of every workgroup (all compute the same; workgroup 0 — wg0 — writes the global outputs):
// the B best of the B x B candidates (ties: lowest flat index), then the bookkeeping the reference does on the host
// (editnet.py:666-699).  sScore / sTok / sPar: running score, next word and parent slot of every slot; *k_left: hypotheses alive;
// *best: best completed hypothesis so far; t = pick index, k = rows of the launch.
// bm_hist_score (optional, laid out like bm_hist_word): the value of the pick behind slot s after pick t if that pick counted
// (alive or just completed), -inf otherwise — a slot with word == <end> and a score above -inf IS a completion of pick t, and
// the completions of one pick stand in pick-rank order (the n-best list of the search).  NULL: nothing is written.
__device__ __forceinline__ void pb_pick(const float* sCand, float* sScore, long long* sTok, int* sPar, int* k_left, float* best,
                                        int* bm_hist_par, long long* bm_hist_word, float* bm_best_score, long long* bm_best_word,
                                        int* bm_result, const int V, const long long end_idx, const int t, const int k,
                                        const bool wg0, float* bm_hist_score = nullptr) {
    const int kl = *k_left;
    float pv_[PW_BEAM_K];
    int pi_[PW_BEAM_K];
    unsigned taken = 0u;
    for (int rr_ = 0; rr_ < k; ++rr_) {
        float bv = -INFINITY;
        int bix = 0x7fffffff, bc = -1;
        for (int c = 0; c < k * PW_BEAM_K; ++c) {
            if ((taken >> c) & 1u) continue;
            if ((c % PW_BEAM_K) >= k) continue;
            const float v = sCand[c * 2];
            const int ix = __float_as_int(sCand[c * 2 + 1]);
            if (ix == 0x7fffffff) continue;
            if (v > bv || (v == bv && ix < bix) || bc < 0) { bv = v; bix = ix; bc = c; }
        }
        if (bc >= 0) taken |= 1u << bc;
        pv_[rr_] = bc >= 0 ? bv : -INFINITY;
        pi_[rr_] = bc >= 0 ? bix : 0x7fffffff;
    }
    int n_end = 0, c_arg = -1, slot = 0;
    float c_best = -INFINITY;
    bool live[PW_BEAM_K];
    for (int rr_ = 0; rr_ < k; ++rr_) {
        const int flat = pi_[rr_];
        const bool okp = flat != 0x7fffffff && rr_ < kl;          // only the first k_left picks count
        const long long word = okp ? flat % V : 0;
        const bool is_end = okp && word == end_idx;
        live[rr_] = okp && !is_end;
        if (is_end) {
            ++n_end;
            if (pv_[rr_] > c_best) { c_best = pv_[rr_]; c_arg = rr_; }   // first maximum
        }
    }
    if (c_arg >= 0 && c_best > *best) {
        *best = c_best;
        if (wg0) {
            bm_best_score[0] = c_best;
            bm_best_word[0] = pi_[c_arg] % V;
            bm_result[0] = t;                                // pick index of the best completed hypothesis
            bm_result[1] = pi_[c_arg] / V;                   // its parent slot (numbering before this pick)
        }
    }
    *k_left = kl - n_end;
    for (int pass = 0; pass < 2; ++pass)                     // live slots first, in pick order
        for (int rr_ = 0; rr_ < k; ++rr_) {
            if ((pass == 0) != live[rr_]) continue;
            const int flat = pi_[rr_];
            const int parent = flat != 0x7fffffff ? flat / V : 0;
            const long long word = flat != 0x7fffffff ? flat % V : 0;
            sScore[slot] = live[rr_] ? pv_[rr_] : -INFINITY;
            sTok[slot] = live[rr_] ? word : 0;
            sPar[slot] = parent;
            if (wg0) {
                bm_hist_par[t * PW_BEAM_K + slot] = parent;
                bm_hist_word[t * PW_BEAM_K + slot] = word;
                if (bm_hist_score) bm_hist_score[t * PW_BEAM_K + slot] = (flat != 0x7fffffff && rr_ < kl) ? pv_[rr_] : -INFINITY;
            }
            ++slot;
        }
    if (wg0) { bm_result[2] = kl - n_end; bm_result[3] = t + 1; }
}

// an exchange of the launch timed out: never a search result
__device__ __forceinline__ void pb_poison(float* bm_best_score, int* bm_result) {
    bm_best_score[0] = __builtin_nanf(""); bm_result[2] = -1; bm_result[3] = -1;
}

}  // namespace set
