// Beam-search step epilogue for MANY images at once (the reference's evaluate() is
// batch 1: editnet.py:654-699, dcnet.py:450-500, eval_full.py:150-200).
//
// One workgroup per image.  The k hypotheses of image i are rows i*k .. i*k+k-1 of the logits.
//   1. log-softmax statistics of every live row (block-wide online max / sum-exp), or for the ensemble
//      log((softmax_e + softmax_d) / 2) (eval_full.py:151-153);
//   2. flat top-k over the k*V candidates  score[j] + logp[j][v]  (editnet.py:659-664): per-thread sorted
//      top-KMAX lists, then k rounds of block arg-max that pop the winner (ties: lowest flat index);
//   3. the bookkeeping the reference does on the host (editnet.py:666-699): parent / word split, completed
//      hypotheses (best completed score, first maximum over time), k shrinks by the number of <end>s, live
//      hypotheses compacted to the front in pick order, sequences re-indexed by parent and extended,
//      next input words, and the parent row map that beam_gather_k uses to re-index the LSTM states.
// Nothing is synchronised with the host; an image whose k has reached 0 is a no-op.
#include "beam_tail.h"

namespace set {

struct BeamArgs {
    const float* logits;
    const float* logits2;        // second model of the ensemble, or nullptr
    long long ld;
    BeamState s;                 // done_*: the n-best entry's arrays (set_beam_pick_nbest_f32), all four nullptr otherwise
};

__global__ void __launch_bounds__(256) beam_pick_k(const BeamArgs args) {
    __shared__ float s_m[4][2], s_s[4][2];
    __shared__ float s_lse[BEAM_KMAX][2];
    __shared__ float s_rv[4];
    __shared__ int s_ri[4];
    __shared__ float s_pick_v[BEAM_KMAX];
    __shared__ int s_pick_i[BEAM_KMAX];
    __shared__ BeamTailLds s_t;
    const BeamState& a = args.s;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k, V = a.V;
    const int kl = a.k_left[img];
    if (kl <= 0) {                               // finished image: identity state map, nothing else changes
        if (tid < k) { a.rows[img * k + tid] = img * k + tid; a.words[img * k + tid] = 0; }
        return;
    }
    float sc[BEAM_KMAX];
#pragma unroll
    for (int j = 0; j < BEAM_KMAX; ++j) sc[j] = j < k ? a.scores[img * k + j] : -INFINITY;

    // ---- 1. log-sum-exp of every live row (both models for the ensemble)
    const int nmodel = args.logits2 ? 2 : 1;
    for (int j = 0; j < k; ++j) {
        if (sc[j] == -INFINITY) continue;        // uniform across the block
        for (int mdl = 0; mdl < nmodel; ++mdl) {
            const float* row = (mdl ? args.logits2 : args.logits) + (long long)(img * k + j) * args.ld;
            float m = -INFINITY, s = 0.f;
            for (int v = tid; v < V; v += 256) {
                const float x = row[v];
                if (x > m) { s = s * expf(m - x) + 1.f; m = x; }
                else s += expf(x - m);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float om = __shfl_xor(m, off), os = __shfl_xor(s, off);
                const float nm = fmaxf(m, om);
                s = (m == -INFINITY ? 0.f : s * expf(m - nm)) + (om == -INFINITY ? 0.f : os * expf(om - nm));
                m = nm;
            }
            if (lane == 0) { s_m[wave][mdl] = m; s_s[wave][mdl] = s; }
        }
        __syncthreads();
        if (tid < nmodel) {
            float m = s_m[0][tid], s = s_s[0][tid];
            for (int w = 1; w < 4; ++w) {
                const float om = s_m[w][tid], os = s_s[w][tid], nm = fmaxf(m, om);
                s = s * expf(m - nm) + os * expf(om - nm);
                m = nm;
            }
            s_lse[j][tid] = m + logf(s);
        }
        __syncthreads();
    }

    // ---- 2a. per-thread sorted top-KMAX of the candidates it owns (ascending flat index per thread)
    float lv[BEAM_KMAX];
    int li[BEAM_KMAX];
#pragma unroll
    for (int q = 0; q < BEAM_KMAX; ++q) { lv[q] = -INFINITY; li[q] = BEAM_NONE; }
    for (int j = 0; j < k; ++j) {
        if (sc[j] == -INFINITY) continue;
        const float* row = args.logits + (long long)(img * k + j) * args.ld;
        const float* row2 = args.logits2 ? args.logits2 + (long long)(img * k + j) * args.ld : nullptr;
        const float l0 = s_lse[j][0], l1 = row2 ? s_lse[j][1] : 0.f;
        for (int v = tid; v < V; v += 256) {
            float lp;
            if (row2) lp = logf((expf(row[v] - l0) + expf(row2[v] - l1)) * 0.5f);
            else lp = row[v] - l0;
            const float x = sc[j] + lp;
            if (x > lv[BEAM_KMAX - 1]) {
                lv[BEAM_KMAX - 1] = x; li[BEAM_KMAX - 1] = j * V + v;
#pragma unroll
                for (int q = BEAM_KMAX - 1; q > 0; --q)
                    if (lv[q] > lv[q - 1]) {
                        const float tv = lv[q]; lv[q] = lv[q - 1]; lv[q - 1] = tv;
                        const int ti = li[q]; li[q] = li[q - 1]; li[q - 1] = ti;
                    }
            }
        }
    }
    // ---- 2b. k rounds of block arg-max over the list heads; the winner pops its head
    for (int r = 0; r < k; ++r) {
        float bv = lv[0];
        int bi = li[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (beam_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_rv[wave] = bv; s_ri[wave] = bi; }
        __syncthreads();
        bv = s_rv[0]; bi = s_ri[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (beam_better(s_rv[w], s_ri[w], bv, bi)) { bv = s_rv[w]; bi = s_ri[w]; }
        if (li[0] == bi && bi != BEAM_NONE) {
#pragma unroll
            for (int q = 0; q + 1 < BEAM_KMAX; ++q) { lv[q] = lv[q + 1]; li[q] = li[q + 1]; }
            lv[BEAM_KMAX - 1] = -INFINITY; li[BEAM_KMAX - 1] = BEAM_NONE;
        }
        if (tid == 0) { s_pick_v[r] = bv; s_pick_i[r] = bi; }
        __syncthreads();
    }

    // ---- 3. bookkeeping of one image (editnet.py:666-699; beam_tail.h): one group of k slots, never exhausted, plain scores
    if (tid == 0) {
        beam_tail_begin(a, img, s_t);
        a.k_left[img] = beam_tail_group<false, false>(a, img, 0, k, kl, s_pick_v, s_pick_i, 0.f, 1.f, 0, nullptr, nullptr, nullptr,
                                                      s_t);
        if (a.n_done) a.n_done[img] = s_t.done_at + s_t.done_n;
    }
    __syncthreads();
    beam_tail_copy(a, img, s_t, tid, 256);
}

// state[s][r] <- state[s][rows[r]] for the k rows of one image, in place (all parents are rows of the same image)
struct BeamStates {
    float* p[4];
    int n;
};
__global__ void __launch_bounds__(256) beam_gather_k(BeamStates st, const int* rows, int k, int D) {
    extern __shared__ float lds[];
    const int img = blockIdx.x, tid = threadIdx.x;
    float* base = st.p[blockIdx.y] + (long long)img * k * D;
    bool identity = true;
    for (int j = 0; j < k; ++j) identity = identity && rows[img * k + j] == img * k + j;
    if (identity) return;
    for (int e = tid; e < k * D; e += 256) lds[e] = base[e];
    __syncthreads();
    for (int e = tid; e < k * D; e += 256) {
        const int j = e / D, c = e - j * D;
        base[e] = lds[(rows[img * k + j] - img * k) * D + c];
    }
}

}  // namespace set

using namespace set;

extern "C" {

// done_*: all four NULL for set_beam_pick_f32 (nothing written), the n-best entry's arrays otherwise
static int beam_pick(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                     int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in, int64_t* seqs_out,
                     float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                     float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done, void* stream) {
    if (!logits || !scores || !k_left || !seqs_in || !seqs_out || !best_score || !best_seq || !best_len || !words || !rows)
        return SET_ERR_ARG;
    if (NI <= 0 || k <= 0 || V <= 0 || cur_len < 1 || cur_len + 1 > Lmax || ld < V) return SET_ERR_ARG;
    if (k > BEAM_KMAX || (long long)k * V >= BEAM_NONE) return SET_ERR_UNSUPPORTED;
    const BeamArgs a{logits, logits2, ld, beam_state(k, V, end_idx, cur_len, Lmax, scores, k_left, seqs_in, seqs_out, best_score, best_seq,
                                                    best_len, words, rows, done_score, done_seq, done_len, n_done)};
    ProfScope ps("beam_pick", (hipStream_t)stream, 0.0, 8.0 * NI * k * V * (logits2 ? 2.0 : 1.0));
    hipLaunchKernelGGL(beam_pick_k, dim3(NI), dim3(256), 0, (hipStream_t)stream, a);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

int set_beam_pick_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                      int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in, int64_t* seqs_out,
                      float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                      void* stream) {
    return beam_pick(logits, logits2, ld, NI, k, V, end_idx, cur_len, Lmax, scores, k_left, seqs_in, seqs_out, best_score,
                     best_seq, best_len, words, rows, nullptr, nullptr, nullptr, nullptr, stream);
}

int set_beam_pick_nbest_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                            int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in, int64_t* seqs_out,
                            float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words, int32_t* rows,
                            float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done, void* stream) {
    if (!done_score || !done_seq || !done_len || !n_done) return SET_ERR_ARG;
    return beam_pick(logits, logits2, ld, NI, k, V, end_idx, cur_len, Lmax, scores, k_left, seqs_in, seqs_out, best_score,
                     best_seq, best_len, words, rows, done_score, done_seq, done_len, n_done, stream);
}

int set_beam_gather_f32(float* s0, float* s1, float* s2, float* s3, const int32_t* rows, int NI, int k, int D,
                        void* stream) {
    if (!s0 || !rows || NI <= 0 || k <= 0 || D <= 0) return SET_ERR_ARG;
    if (k > BEAM_KMAX || (size_t)k * D * sizeof(float) > 64 * 1024) return SET_ERR_UNSUPPORTED;
    BeamStates st;
    st.p[0] = s0; st.p[1] = s1; st.p[2] = s2; st.p[3] = s3;
    st.n = s3 ? 4 : (s2 ? 3 : (s1 ? 2 : 1));
    ProfScope ps("beam_gather", (hipStream_t)stream, 0.0, 8.0 * NI * k * D * st.n);
    hipLaunchKernelGGL(beam_gather_k, dim3(NI, st.n), dim3(256), (size_t)k * D * sizeof(float), (hipStream_t)stream, st,
                       rows, k, D);
    SET_LAUNCH_CHECK();
    return SET_OK;
}

}  // extern "C"
