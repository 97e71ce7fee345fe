// Persistent free-running decode for small batches (B <= 8): the whole greedy loop of DCNet (dcnet_rl.py:286-346) as ONE
// launch of D / 4 workgroups that exchange activations through flag-in-data words instead of six launches per timestep.
// (EditNet's twin: decode_persistent_wide.hip.)
//
// At B = 4 a timestep of the per-step path is six dependent launches of 10-25 us that stream 123 MB of weights between
// them: every launch pays a boundary, a start-up and a tail, and the pointwise kernels between the GEMV launches run at the
// launch floor.  Here
//   * a workgroup OWNS 4 hidden units of both LSTM cells: the 16 gate rows of attention_lstm [W_ih[:, h2] | W_hh] and of
//     language_lstm [W_hh | W_ih[:, h1]] are contracted over the full K by its four waves (one K quarter each, weights
//     streamed as ready-made B operands of v_mfma_f32_16x16x4_f32: one 16-byte load per lane feeds four MFMAs, K permuted
//     identically in the activation operand read from LDS), the four partial tiles are added through LDS in wave order and
//     the cell update runs in the same workgroup: no split-K slabs, no pointwise launch, c1 / c2 never leave registers;
//   * the context half of language_lstm's input product is hoisted: W_ih[:, D:] ctx = sum_t alpha_t (W_ih[:, D:] enc_t), so
//     the prologue computes Pc = enc W_ih[:, D:]^T (B, T, 4D) once and a timestep only needs the attention weights —
//     16 MB of weights per timestep are not streamed at all, and every workgroup computes the (tiny) attention itself
//     (its cap_features_att rows stay in registers at B <= 4) instead of waiting for a context vector;
//   * cap_decoder_att(h1) (A x D) is the one product whose output every workgroup needs: A / 256 = 2 rows per workgroup;
//   * fc: a workgroup scores V / 256 (+) vocabulary rows and publishes (max, first arg-max, sum exp) per batch row; every
//     workgroup combines the 256 triples itself (same word everywhere, no broadcast round), workgroup 0 writes seq /
//     seq_logp and the loop's bookkeeping words.
// Four exchanges per timestep (h1, the attention projection, h2, the fc triples), each as 8-byte {value, tag} words
// (grid_barrier.h): a consumer polls the words it needs until they carry the exchange's tag — no counters, no fences.
// Weight tiles rotate through two register buffers of 64 KB per workgroup.  Where their requests sit matters: a wave's loads
// return in order (a poll waits for every tile requested before it), a saturated request queue blocks the wave at the next
// load, and the compiler drains outstanding requests at a loop header or branch join — so a tile is requested right before
// arithmetic that does not need it (fc's tiles around the attention scores), the h-dependent gate products of timestep t + 1
// are contracted while the fc triples of timestep t travel (S1'), and the B <= 4 variant has no loop around its per-row work.
// Teacher-forced mode (set_dcnet_xe_forward): words from the captions, scores written by the owners of the vocabulary rows,
// three exchanges.
// Sampled mode (set_dcnet_gumbel_persistent): the free-running loop with the Gumbel-max draw (philox.h) in place of the arg-max —
// the fc exchange's four words per (row, slice) carry (log-sum-exp of y, first arg-max of y + g, max of y + g, y there); same
// exchanges, same LDS.
// Same residency rule, fault word and event chain as the persistent encoder (grid_barrier.h PersistentGuard).  A poll that
// times out poisons seq_logp with NaN; the host raises SET_ERR_FAULT at its next call.
// Shared with the other two persistent decode kernels: the beam mode's pick (beam_persistent.h) and, on the host, the launch
// itself (decode_persistent.h: the per-instantiation record PersistentKernel, pdec_launch from the LDS cap and the residency
// check to the stamp report, and the fills of the argument block; pdec_dcnet_fill / pdec_dcnet_layout also serve the ensemble's
// DCNet half) and arithmetic leaves of the phases (decode_persistent.h: pd_sum4 / pd_sum4p, pd_cell in S1, pd_fc_score,
// pd_fc_triple, pd_clamp_tok).  Deliberately NOT shared: the schedule of the timestep — where a tile's loads sit between the
// MFMAs, the exchanges and the barriers — and the language cell and the masked row softmax of S3, which as leaves moved the
// AGPR counts of the register-resident instantiations (profiles/pdec_leaves_resources.json).
#include "beam_persistent.h"
#include "philox.h"

namespace set {

struct PDecDcnetArgs {
    // weights
    const float* al_wih_h2; long long ld_al;     // attention_lstm.weight_ih[:, E + 2C:] (4D, D)
    const float* al_whh;                         // (4D, D)
    const float* ll_whh;                         // (4D, D)
    const float* ll_wih; long long ld_ll;        // language_lstm.weight_ih (4D, 2E): columns [0, D) are used here
    const float *ll_bih, *ll_bhh;
    const float *ca_dec_w, *ca_dec_b, *ca_full_w, *ca_full_b;
    const float *fc_w, *fc_b;
    const float* tok_table; long long ld_tab;    // columns [0, 4D): attention_lstm.W_ih[:, :E] relu(E[v])
    // per sequence (prologue outputs)
    const float* pre1;                           // (B, 4D) final_hidden columns + both biases of attention_lstm
    const float* att1_c;                         // (B, T, A)
    const float* mask;                           // (B, T)
    const float* pc;                             // (B, T, 4D) hoisted language_lstm.W_ih[:, D:] enc
    // exchange buffers: flag-in-data words of 8 bytes per float (grid_barrier.h), zero-filled before the launch
    void* x_h1; void* x_h2;                      // (B, D)
    void* x_att2;                                // (B, A) cap_decoder_att(h1), bias not added
    void* x_fc;                                  // (B, G) x (max, arg-max, sum exp, -)
    // outputs / loop words
    long long* it; int* unfinished; int* alive;
    long long* seq; float* seq_logp;
    unsigned* status; unsigned* fault; unsigned spin_limit; int test_stall;
    int B, D, T, A, V, max_len, rpw;
    long long start_idx, end_idx;
    // teacher-forced mode (set_dcnet_xe_forward, dcnet.py:333-348): words from caps, scores of the first bt rows written out,
    // no pick and no fourth exchange
    const long long* caps; long long caps_stride;
    float* predictions; long long ld_pred_b;     // (B, maxT, V)
    int dlen[PDEC_MAXB];                         // decode lengths, descending (0 = free-running)
    int stamp_wg;
    unsigned long long* stamps;                  // diagnostic (SET_PDEC_STAMPS=1): 100-MHz time stamps of workgroup 0, 16 per timestep
    // (LH, teacher-forced) h2 of every row at its last step t = dlen[b] - 1 (dcnet_with_mse.py:321,341), (B, D).  Last member:
    // the offsets of the fields above, and so the instructions of the variants without it, stay as they were
    float* last_h2;
    // beam mode (BEAM, set_dcnet_beam_persistent): the rows are the k hypotheses of ONE image.  After last_h2, for the same reason
    void* x_fcb;                                 // (B, G, PW_BEAM_W) per-slice (max, sum exp, 4 x (score, word)) words
    int* bm_hist_par;                            // (max_len, 4) parent slot of every slot after every pick
    long long* bm_hist_word;                     // (max_len, 4) word appended to every slot at every pick
    float* bm_best_score;                        // [1] best completed hypothesis (-inf: none)
    long long* bm_best_word;                     // [1] its last word (<end>)
    int* bm_result;                              // [4] pick index and parent slot of the best completed hypothesis, k_left, picks made
    float* bm_hist_score;                        // (max_len, 4) or NULL: value of every counted pick, -inf elsewhere (n-best)
    // sampled mode (SAMPLE, set_dcnet_gumbel_persistent): key of the Gumbel noise (philox.h) and 1 / temperature.  After
    // bm_hist_score, for the same reason
    unsigned long long gm_seed, gm_offset;
    float gm_inv_t;
};

// RES: B <= 4 and T <= PDEC_TREG — a wave scores ONE fixed row, whose hoisted cap_features_att rows (loop-invariant, T x A
// floats = 160 registers per lane) then stay in registers for the whole decode.
// LH: teacher-forced only, also write last_h2 (set_dcnet_xe_forward_hidden).  The loop keeps computing every row until the
// longest caption ends, so no buffer holds a row's h2 at its own last step: the owner of h2[b, u] stores it when t + 1 ==
// dlen[b].  A template parameter, not a runtime test: the variants without it compile to the same instructions as before.
// BEAM: free-running only; the B <= PW_BEAM_K rows are the hypotheses of ONE image and the loop is the reference's beam search
// (dcnet.py:447-514) instead of the greedy loop: the arg-max epilogue (X4 / S6) becomes the pick that
// editnet_persistent_wide_k<BEAM> (decode_persistent_wide.hip) and the ensemble kernel run too — its slice top-k, candidate words,
// row merge and bookkeeping are the functions of beam_persistent.h, shared by the three kernels (they run after the timestep's
// last MFMA, no weight tile is in flight there); the phase code around them stays this kernel's own.  Per pick every workgroup
// publishes, per row, (max, sum exp, its PW_BEAM_K best (score, word) pairs) of its vocabulary slice, stages all slices and runs
// the same merge (value descending, flat index ascending among equals): the same (parent, word) per slot everywhere, no
// broadcast round.
// Recurrent state follows the parent map inside the launch: c1 / c2 of the owned units through a small LDS table, the
// h-dependent products contracted ahead of the pick (S1') are read through the parent slot — language_lstm.W_hh h2 therefore
// goes to LDS instead of staying in the accumulator that S2 continues.  h1 / h2 themselves are recomputed after every pick
// and need no permutation.  The per-sequence operands (pre1, att1_c, mask, pc) are REPLICATED k times by the prologue, as
// on the EditNet path (the rows of the workspace hold the image's previous caption k times).  A template parameter, not a
// runtime test, like LH.
// SAMPLE: free-running only, without LH and BEAM; the greedy loop with the Gumbel-max draw (philox.h; set_dcnet_gumbel_persistent)
// in place of the arg-max epilogue (X4 / S6) — "sampled mode" below.  A template parameter, not a runtime test, like LH and BEAM.
template <bool RES, bool LH = false, bool BEAM = false, bool SAMPLE = false>
__global__ void __launch_bounds__(PDEC_THREADS, 1) dcnet_persistent_k(const PDecDcnetArgs P) {
    static_assert(!SAMPLE || (!LH && !BEAM), "the sampled mode is the free-running greedy loop's only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ long long sTok[PDEC_MAXB];
    __shared__ int sUnf[PDEC_MAXB];
    const int tid = threadIdx.x, lane = tid & 63, kq = tid >> 6, r = lane & 15, g = lane >> 4;
    const int B = P.B, D = P.D, T = P.T, A = P.A, V = P.V;
    const int KQ = D >> 2, LDH = D + 4;
    const int wg = (int)blockIdx.x, u0 = wg * 4, G = (int)gridDim.x;
    float* sH1 = smem;                                   // (B, LDH) h1, rows padded by 16 bytes: conflict-free ds_read_b128
    float* sH2 = sH1 + B * LDH;
    float* sRed = sH2 + B * LDH;                         // [4 waves][3 tiles][16 batch rows][16 weight rows]
    float* sAl = sRed + 4 * 3 * 256;                     // (B, T) attention weights
    float* sG = sAl + PDEC_MAXB * PDEC_TMAX;             // (B, 16) gate pre-activations of language_lstm
    float* sA2 = sG + PDEC_MAXB * 16;                    // (B, A) cap_decoder_att(h1) of every row
    float* sF = sA2 + B * A;                             // (B, G, 4) fc triples of every workgroup
    float* sCon = sF + B * G * 4;                        // [cap_decoder_att.bias | cap_full_att.weight] (2, A): loop-invariant
    float* sPc = sCon + 2 * A;                           // (B, 16, TMAX) hoisted context products of the owned gate rows
    // beam mode only (pdec_lds_floats): every workgroup's per-slice candidates, language_lstm.W_hh h2 of the previous timestep
    // (added through the parent map), the cell states on their way through the parent map, the candidate lists of the pick and
    // the pick's bookkeeping words
    float* sFB = sPc + B * 16 * PDEC_TS;         // (B, G, PW_BEAM_W)
    float* sRedP = sFB + B * G * PW_BEAM_W;              // [4 waves][16 batch rows][16 weight rows]
    float* sCst = sRedP + 4 * 256;                       // (2, K, 4) c1 | c2 of the owned units
    float* sCand = sCst + 2 * PW_BEAM_K * 4;             // (K, K, 2) (score, flat index) of every row's best K candidates
    float* sScore = sCand + PW_BEAM_K * PW_BEAM_K * 2;   // (K) running scores of the slots (-inf = dead)
    int* sPar = reinterpret_cast<int*>(sScore + PW_BEAM_K);   // (K) parent slot of every slot (identity before the first pick)
    int* sKleft = sPar + PW_BEAM_K;                      // [0] hypotheses alive
    float* sBest = reinterpret_cast<float*>(sKleft + 1); // [0] best completed hypothesis so far
    const LLWatch watch{P.status, P.fault, P.spin_limit};
    // exchange buffers (grid_barrier.h, flag-in-data words)
    const __amdgpu_buffer_rsrc_t h1rs = __builtin_amdgcn_make_buffer_rsrc((void*)P.x_h1, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t h2rs = __builtin_amdgcn_make_buffer_rsrc((void*)P.x_h2, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t a2rs = __builtin_amdgcn_make_buffer_rsrc((void*)P.x_att2, 0, B * A * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t fcrs = __builtin_amdgcn_make_buffer_rsrc((void*)P.x_fc, 0, B * G * 32, 0x00027000);
    const __amdgpu_buffer_rsrc_t fbrs = __builtin_amdgcn_make_buffer_rsrc(BEAM ? P.x_fcb : P.x_fc, 0, BEAM ? B * G * PW_BEAM_W * 8 : 32, 0x00027000);

    // ---- initial state: h1 = h2 = 0, every row is fed <start>
    for (int i = tid; i < 2 * B * LDH; i += PDEC_THREADS) smem[i] = 0.f;
    for (int i = tid; i < A; i += PDEC_THREADS) { sCon[i] = P.ca_dec_b[i]; sCon[A + i] = P.ca_full_w[i]; }
    const float bf = P.ca_full_b[0];
    if (tid < B) { sTok[tid] = P.start_idx; sUnf[tid] = 1; }
    if constexpr (BEAM) {
        if (tid < PW_BEAM_K) { sPar[tid] = tid; sScore[tid] = tid == 0 ? 0.f : -INFINITY; }   // pick 1: all rows are identical, only row 0 counts
        for (int i = tid; i < 4 * 256; i += PDEC_THREADS) sRedP[i] = 0.f;                     // W_hh h2 of the zero initial state
        if (tid == 0) {
            sKleft[0] = B; sBest[0] = -INFINITY;
            if (wg == 0) { P.bm_best_score[0] = -INFINITY; P.bm_best_word[0] = 0; P.bm_result[0] = -1; P.bm_result[1] = -1; P.bm_result[2] = B; P.bm_result[3] = 0; }
        }
    }
    __syncthreads();

    // ---- weight tiles of this lane: gate row of output column r = gate (r >> 2) of unit u0 + (r & 3)
    const long long grow = (long long)(r >> 2) * D + u0 + (r & 3);
    const int kcol = kq * KQ + 4 * g;
    const float* pT0 = P.al_wih_h2 + grow * P.ld_al + kcol;
    const float* pT1 = P.al_whh + grow * D + kcol;
    const float* pT2 = P.ll_whh + grow * D + kcol;
    const float* pT3 = P.ll_wih + grow * P.ld_ll + kcol;
    // cap_decoder_att: A / G rows of the (A, D) projection per workgroup, full K (lanes r >= apw hold zeros)
    const int apw = A / G;                               // host: A % G == 0, apw <= 16
    const bool vD = r < apw;
    const float* pT4 = P.ca_dec_w + (long long)(vD ? wg * apw + r : 0) * D + kcol;
    const int row0 = wg * P.rpw;
    const float* pF[PDEC_FC_TILES];
    bool vF[PDEC_FC_TILES];
#pragma unroll
    for (int j = 0; j < PDEC_FC_TILES; ++j) {
        const int row = row0 + 16 * j + r;
        vF[j] = (16 * j + r < P.rpw) && row < V;
        pF[j] = P.fc_w + (long long)(vF[j] ? row : 0) * D + kcol;
    }
    const float fcb_lane = (lane < 16 * PDEC_FC_TILES && lane < P.rpw && row0 + lane < V) ? P.fc_b[row0 + lane] : 0.f;   // fc.bias of the row lane l scores
    const int arow = (r < B ? r : B - 1) * LDH;          // rows >= B repeat the last one: their outputs are never read
    const float* aH1 = sH1 + arow + kcol;
    const float* aH2 = sH2 + arow + kcol;

    // ---- thread roles
    const bool pair = tid < B * 4;                       // (batch row, unit) of the two cell updates
    const int pb = tid >> 2, pu = tid & 3;
    const bool gcol = tid < B * 16;                      // (batch row, gate row) of the hoisted-context gather
    const int cb = tid >> 4, crr = tid & 15;
    const long long ccol = (long long)(crr >> 2) * D + u0 + (crr & 3);
    float c1 = 0.f, c2 = 0.f, pre[4] = {0.f, 0.f, 0.f, 0.f};
    float b2 = 0.f;
    if (pair) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[q] = P.pre1[(long long)pb * 4 * D + (long long)q * D + u0 + pu];
    }
    if (gcol) b2 = P.ll_bih[ccol] + P.ll_bhh[ccol];

    // weight tiles rotate through two register buffers:  X1: wb<-T3 wa<-T4 | S2 (wb<-F1, wa<-F0) | S5 (wa<-F2, wb<-T0', wa<-T1')
    // | S1' (wb<-T2')
    f32x4 wa[PDEC_KB], wb[PDEC_KB];
    // loop-invariant operands of the attention phase: the hoisted context products of this thread's gate row ...
    if (gcol)
        for (int tt = 0; tt < PDEC_TMAX; ++tt) sPc[tid * PDEC_TS + tt] = tt < T ? P.pc[((long long)cb * T + tt) * 4 * D + ccol] : 0.f;
    __syncthreads();
    // ... and (RES) this wave's row of cap_features_att
    f32x4 a1r[RES ? PDEC_TREG : 1][2];
    float mk_res = 1.f;                                  // (RES) ... and its mask word
    if constexpr (RES) {
        const int brow = kq < B ? kq : B - 1;
        if (lane < T) mk_res = P.mask[(long long)brow * T + lane];
#pragma unroll
        for (int tt = 0; tt < PDEC_TREG; ++tt) {
            const int t2 = tt < T ? tt : T - 1;
            a1r[tt][0] = *reinterpret_cast<const f32x4*>(P.att1_c + ((long long)brow * T + t2) * A + lane * 4);
            a1r[tt][1] = *reinterpret_cast<const f32x4*>(P.att1_c + ((long long)brow * T + t2) * A + lane * 4 + 256);
        }
    }
    unsigned tag = 0;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // the h-dependent gate products of timestep t do not depend on the word chosen at t - 1: they are contracted at the END
    // of timestep t - 1, while its fc triples travel (S1' below; the F/A merge of the per-step loop).  t = 0: h1 = h2 = 0.
    f32x4 acc1 = zero4, acc2 = zero4;
    for (int t = 0; t < P.max_len; ++t) {
        // ================= S1: attention_lstm cell (h1) from the products of S1'
        PD_STAMP(0);
        float tg[4] = {0.f, 0.f, 0.f, 0.f};
        int bt = B;                                              // teacher-forced: rows whose caption is still running (sorted batch)
        if (!BEAM && !SAMPLE && P.caps) {
            bt = 0;
            for (int b = 0; b < B; ++b) bt += P.dlen[b] > t ? 1 : 0;
            if (bt == 0) break;
        }
        if (pair) {
            long long tok = (!BEAM && !SAMPLE && P.caps) ? P.caps[(long long)pb * P.caps_stride + t] : sTok[pb];
            tok = pd_clamp_tok(tok, V);
            const float* trow = P.tok_table + tok * P.ld_tab + u0 + pu;
#pragma unroll
            for (int q = 0; q < 4; ++q) tg[q] = trow[(long long)q * D];
        }
        PD_STAMP(1);
#pragma unroll
        for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = acc1[e];
        if constexpr (BEAM) {
            if (pair) { sCst[pb * 4 + pu] = c1; sCst[PW_BEAM_K * 4 + pb * 4 + pu] = c2; }
        }
        __syncthreads();
        // beam mode: slot pb continues hypothesis sPar[pb] of the previous timestep — its cell states and the gate products
        // that were contracted before the pick (S1' of the previous timestep) are read through the parent map
        int par = pb;
        if constexpr (BEAM) {
            par = sPar[pair ? pb : 0];
            if (pair) { c1 = sCst[par * 4 + pu]; c2 = sCst[PW_BEAM_K * 4 + par * 4 + pu]; }
        }
        ++tag;                                                   // X1: h1
        if (pair && !(P.test_stall && wg == 0)) {
            float gq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = par * 16 + q * 4 + pu;
                gq[q] = (pd_sum4(sRed, 0, o) + pre[q]) + tg[q];
            }
            ll_put(h1rs, pb * D + u0 + pu, pd_cell(gq[0], gq[1], gq[2], gq[3], c1), tag);
        }
        PD_STAMP(2);
        pd_load(wb, pT3);
        pd_load_if(wa, pT4, vD);
        PD_STAMP(3);
        ll_stage<256, 8>(h1rs, sH1, B, D, LDH, tag, watch, tid);
        __syncthreads();
        // ================= S2: language_lstm W_ih[:, :D] h1, this workgroup's rows of cap_decoder_att(h1)
        PD_STAMP(4);
        pd_mma(acc2, wb, aH1);
        f32x4 accd = zero4;
        pd_mma(accd, wa, aH1);
        PD_STAMP(5);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = accd[e];
            sRed[(kq * 3 + 2) * 256 + (4 * g + e) * 16 + r] = acc2[e];
        }
        __syncthreads();
        ++tag;                                                   // X2: cap_decoder_att(h1) (without its bias)
        float g2 = 0.f;
        if (gcol) {
            const int o = cb * 16 + crr;
            if (crr < apw) {
                ll_put(a2rs, cb * A + wg * apw + crr, pd_sum4(sRed, 1, o), tag);
            }
            g2 = pd_sum4(sRed, 2, o);
            if constexpr (BEAM) g2 += pd_sum4p(sRedP, sPar[cb] * 16 + crr);   // + language_lstm.W_hh h2 of the PARENT hypothesis (S1' of the previous timestep)
        }
        PD_STAMP(6);
        ll_stage<256, 8>(a2rs, sA2, B, A, A, tag, watch, tid);
        __syncthreads();
        pd_load_if(wa, pF[0], vF[0]);                            // fc's first tile streams under the attention's arithmetic ...
        // ================= S3: caption attention of every row, in every workgroup (dcnet.py:261-268)
        // (RES: one row per wave and no loop around it — the compiler drains every outstanding request at a loop header, and
        // fc's tiles are meant to stream under this arithmetic)
        auto attend = [&](const int b) {
            const int a_lo = lane * 4, a_hi = lane * 4 + 256;
            f32x4 a2[2], wf[2];
            a2[0] = *reinterpret_cast<const f32x4*>(sA2 + b * A + a_lo);
            a2[1] = *reinterpret_cast<const f32x4*>(sA2 + b * A + a_hi);
            const float mk = RES ? mk_res : (lane < T ? P.mask[(long long)b * T + lane] : 1.f);
            a2[0] += *reinterpret_cast<const f32x4*>(sCon + a_lo); a2[1] += *reinterpret_cast<const f32x4*>(sCon + a_hi);
            wf[0] = *reinterpret_cast<const f32x4*>(sCon + A + a_lo); wf[1] = *reinterpret_cast<const f32x4*>(sCon + A + a_hi);
            constexpr int RB = 10;
            float mine = 0.f;                                   // lane tt keeps the score of position tt
            const unsigned long long live = __ballot(lane < T && mk != 0.f);
            const float* a1 = P.att1_c + (long long)b * T * A;
            for (int t0 = 0; t0 < (RES ? PDEC_TREG : T); t0 += RB) {
                f32x4 v[RB][2];
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    if constexpr (RES) {
                        v[u][0] = a1r[t0 + u < PDEC_TREG ? t0 + u : 0][0];     // (static indices: t0 is a multiple of RB, PDEC_TREG too)
                        v[u][1] = a1r[t0 + u < PDEC_TREG ? t0 + u : 0][1];
                    } else {
                        const int tt = t0 + u < T ? t0 + u : T - 1;
                        v[u][0] = *reinterpret_cast<const f32x4*>(a1 + (long long)tt * A + a_lo);
                        v[u][1] = *reinterpret_cast<const f32x4*>(a1 + (long long)tt * A + a_hi);
                    }
                }
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    const int tt = t0 + u;
                    // masked position (or past T): its score is -1e10 whatever it is.  Not in the resident variant: a branch here makes
                    // the compiler wait for fc's tile (requested above to stream under this arithmetic) before the first score
                    if (!RES && !((live >> tt) & 1ull)) continue;
                    const float sc = pw_wsum(pd_score8(v[u][0] + a2[0], v[u][1] + a2[1], wf[0], wf[1]));
                    if (lane == tt) mine = sc;
                }
            }
            // masked softmax over the T <= 32 scores inside the wave (one score per lane)
            const float sc = lane < T ? ((mk == 0.f) ? -1e10f : (mine + bf)) : -INFINITY;
            const float m = pw_wmax(sc);
            const float ex = lane < T ? expf(sc - m) : 0.f;
            const float sum = pw_wsum(ex);
            if (lane < T) sAl[b * PDEC_TMAX + lane] = ex / sum;
        };
        if constexpr (RES) { if (kq < B) attend(kq); }
        else { for (int b = kq; b < B; b += 4) attend(b); }
        pd_load_if(wb, pF[1], vF[1]);                            // ... the second under the cell update and the h2 exchange
        __syncthreads();
        PD_STAMP(7);
        if (gcol) {
            float s = 0.f;
            for (int tt = 0; tt < T; ++tt) s += sAl[cb * PDEC_TMAX + tt] * sPc[tid * PDEC_TS + tt];
            sG[cb * 16 + crr] = (g2 + s) + b2;
        }
        __syncthreads();
        ++tag;                                                   // X3: h2
        if (pair) {
            const float* gp = sG + pb * 16 + pu;
            const float ai = pd_sigm(gp[0]), af = pd_sigm(gp[4]), ag = tanhf(gp[8]), ao = pd_sigm(gp[12]);
            c2 = af * c2 + ai * ag;
            const float h2v = ao * tanhf(c2);
            ll_put(h2rs, pb * D + u0 + pu, h2v, tag);
            if constexpr (LH) {                                  // h2 before the output dropout (dcnet_with_mse.py:341)
                if (P.dlen[pb] == t + 1) P.last_h2[(long long)pb * D + u0 + pu] = h2v;
            }
        }
        PD_STAMP(8);
        ll_stage<256, 8>(h2rs, sH2, B, D, LDH, tag, watch, tid);
        __syncthreads();
        PD_STAMP(9);
        // ================= S5: fc over this workgroup's vocabulary rows, local (max, first arg-max, sum exp) per batch row
        const bool more = t + 1 < P.max_len;
        f32x4 accf0 = zero4, accf1 = zero4, accf2 = zero4;
        pd_mma(accf0, wa, aH2);
        pd_load_if(wa, pF[2], vF[2]);
        pd_mma(accf1, wb, aH2);
        if (more) pd_load(wb, pT0);
        pd_mma(accf2, wa, aH2);
        if (more) pd_load(wa, pT1);
        PD_STAMP(10);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = accf0[e];
            sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = accf1[e];
            sRed[(kq * 3 + 2) * 256 + (4 * g + e) * 16 + r] = accf2[e];
        }
        __syncthreads();
        if (!BEAM && !SAMPLE && P.caps) {
            // teacher-forced: the scores themselves, rows 0 .. bt - 1 (dcnet.py:347: predictions[:batch_size_t, t, :] = preds)
            for (int b = kq; b < bt; b += 4) {
                const int row = row0 + lane;
                if (lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V)
                    P.predictions[(long long)b * P.ld_pred_b + (long long)t * V + row] = pd_fc_score(sRed, b, lane, fcb_lane);
            }
            if (more) {                                          // S1' (see below)
                acc1 = zero4; acc2 = zero4;
                pd_mma(acc1, wb, aH2);
                pd_load(wb, pT2);
                pd_mma(acc1, wa, aH1);
                pd_mma(acc2, wb, aH2);
            }
            __syncthreads();                                     // sRed is rewritten by the next timestep's S1
            continue;
        }
        if constexpr (BEAM) {
            // ================= beam mode (dcnet.py:447-514; the pick of beam_persistent.h): X4 carries, per row and vocabulary
            // slice, (max, sum exp) and the slice's B best (score, word) pairs — a global top-B over B x V candidates takes at
            // most B from one slice
            ++tag;
            if (kq < B) {
                const int b = kq;
                const int row = row0 + lane;
                const bool ok = lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V;
                float x = -INFINITY;
                if (ok) x = pd_fc_score(sRed, b, lane, fcb_lane);
                pb_vals cvv;
                pb_idxs cii;
                pb_slice_topk(x, row, ok, B, cvv, cii);
                const float mx = cvv[0];
                float se = (ok && mx > -INFINITY) ? expf(x - mx) : 0.f;
                se = pw_wsum(se);
                pb_publish(fbrs, (b * G + wg) * PW_BEAM_W, lane, mx, se, cvv, cii, tag);
            }
            PD_STAMP(11);
            // S1' (see the greedy path); language_lstm.W_hh h2 goes to LDS: the next timestep adds it through the parent map
            if (more) {
                acc1 = zero4;
                pd_mma(acc1, wb, aH2);
                pd_load(wb, pT2);
                pd_mma(acc1, wa, aH1);
                f32x4 accp = zero4;
                pd_mma(accp, wb, aH2);
#pragma unroll
                for (int e = 0; e < 4; ++e) sRedP[kq * 256 + (4 * g + e) * 16 + r] = accp[e];
                acc2 = zero4;
            }
            PD_STAMP(12);
            ll_stage<256, 8>(fbrs, sFB, B * G, PW_BEAM_W, PW_BEAM_W, tag, watch, tid);
            __syncthreads();
            // ---- every workgroup runs the same pick.  Wave j: log-sum-exp of row j and its B best candidates (G = 256 slices:
            // four per lane)
            if (kq < B) {
                const int j = kq;
                const float scj = sScore[j];
                pb_vals ov;
                pb_idxs oi;
                pb_none(ov, oi);
                if (scj > -INFINITY) {                           // (uniform in the wave; dead slots take no part)
                    float cv[16];
                    int ci[16];
                    float pm[4], ps[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float* e = sFB + ((j * G + lane + 64 * i) * PW_BEAM_W);
                        pm[i] = e[0]; ps[i] = e[1];
#pragma unroll
                        for (int q = 0; q < 4; ++q) { cv[4 * i + q] = e[2 + 2 * q]; ci[4 * i + q] = __float_as_int(e[3 + 2 * q]); }
                    }
                    const float m = pw_wmax(fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3])));
                    float ssum = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) ssum += (pm[i] == -INFINITY) ? 0.f : ps[i] * expf(pm[i] - m);
                    ssum = pw_wsum(ssum);
                    const float lse = m + logf(ssum);
#pragma unroll
                    for (int c = 0; c < 16; ++c) {
                        const bool have = ci[c] != 0x7fffffff;
                        cv[c] = have ? scj + (cv[c] - lse) : -INFINITY;       // score + log-prob, as beam_pick_k forms it
                        ci[c] = have ? j * V + ci[c] : 0x7fffffff;
                    }
                    pb_row_merge(cv, ci, B, ov, oi);
                }
                if (lane == 0) pb_row_store(sCand, j, ov, oi);
            }
            __syncthreads();
            if (tid == 0)                                        // the pick itself and its bookkeeping (beam_persistent.h)
                pb_pick(sCand, sScore, sTok, sPar, &sKleft[0], &sBest[0], P.bm_hist_par, P.bm_hist_word, P.bm_best_score, P.bm_best_word,
                        P.bm_result, V, P.end_idx, t, B, wg == 0, P.bm_hist_score);
            __syncthreads();
            PD_STAMP(13);
            if (sKleft[0] == 0) break;                           // every hypothesis has ended (dcnet.py:507-508)
            continue;
        }
        if constexpr (SAMPLE) {
            // ================= sampled mode: the word of row b is the first maximum of s[v] = y[v] + g[v], y = fl(x inv_t), g = the
            // noise keyed by (seed, offset, b, t, v) — the per-step pick's (epilogue.hip gumbel_pick_k) and
            // editnet_persistent_wide_k<SAMPLE>'s definition, word for word.  X4 keeps its four words per (row, slice) and its
            // region; they carry [log-sum-exp of y over the slice (max y and sum exp folded into one word) | first arg-max of s |
            // max s | y there].  A lane owns ONE vocabulary row; the slice boundaries are not quad-aligned, so every lane calls
            // Philox for its own quad and selects its word.  (After the timestep's last fc MFMA and before S1': only the two
            // tiles of S1' are in flight.)
            ++tag;
            {   // (resident variant: one row per wave, no loop — see the attention phase)
                auto row_work = [&](const int b) {
                    const int row = row0 + lane;
                    const bool ok = lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V;
                    float y = -INFINITY, sv = -INFINITY;
                    if (ok) {
                        const float x = pd_fc_score(sRed, b, lane, fcb_lane);
                        y = __fmul_rn(x, P.gm_inv_t);
                        sv = y + gumbel_at(P.gm_seed, P.gm_offset, b, t, row);
                    }
                    const float my = pw_wmax(y);
                    float se = (ok && my > -INFINITY) ? expf(y - my) : 0.f;
                    if (ok && my == -INFINITY) se = y;                   // no finite score here: NaN scores reach the sum, as in the greedy path
                    se = pw_wsum(se);
                    const float lse = my == -INFINITY ? (se == 0.f ? -INFINITY : se) : my + logf(se);
                    float best = -INFINITY;
                    int bi = 0x7fffffff;
                    if (sv > best) { best = sv; bi = row; }
                    pw_wargmax(best, bi);
                    const float yw = bi == 0x7fffffff ? 0.f : pw_lane(y, bi - row0);
                    if (lane < 4) ll_put(fcrs, (b * G + wg) * 4 + lane, lane == 0 ? lse : (lane == 1 ? __int_as_float(bi) : (lane == 2 ? best : yw)), tag);
                };
                if constexpr (RES) { if (kq < B) row_work(kq); }
                else { for (int b = kq; b < B; b += 4) row_work(b); }
            }
            PD_STAMP(11);
            if (more) {                                              // S1' (see the greedy path)
                acc1 = zero4; acc2 = zero4;
                pd_mma(acc1, wb, aH2);
                pd_load(wb, pT2);
                pd_mma(acc1, wa, aH1);
                pd_mma(acc2, wb, aH2);
            }
            PD_STAMP(12);
            ll_stage<256, 8>(fcrs, sF, B * G, 4, 4, tag, watch, tid);
            __syncthreads();
            // ---- every workgroup combines the G entries of every row in slice order: same word everywhere
            {
                auto row_work = [&](const int b) {
                    float pl[4], ps[4], py[4];
                    int pi[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int wi = lane + 64 * i;
                        const bool have = wi < G;
                        const f32x4 e4 = have ? *reinterpret_cast<const f32x4*>(sF + (b * G + wi) * 4) : zero4;
                        pl[i] = have ? e4[0] : -INFINITY;
                        pi[i] = have ? __float_as_int(e4[1]) : 0x7fffffff;
                        ps[i] = have ? e4[2] : -INFINITY;
                        py[i] = e4[3];
                    }
                    float best = -INFINITY, yb = 0.f;
                    int bi = 0x7fffffff;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (ps[i] > best || (ps[i] == best && pi[i] < bi)) { best = ps[i]; bi = pi[i]; yb = py[i]; }
                    const int mine = bi;                             // this lane's candidate; the winner's y travels from its lane
                    pw_wargmax(best, bi);
                    const unsigned long long own = __ballot(mine == bi && bi != 0x7fffffff);
                    const float yw = own ? pw_lane(yb, __ffsll((long long)own) - 1) : 0.f;
                    const float m = pw_wmax(fmaxf(fmaxf(pl[0], pl[1]), fmaxf(pl[2], pl[3])));
                    float tot = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) tot += (pl[i] == -INFINITY) ? 0.f : (m == -INFINITY ? pl[i] : expf(pl[i] - m));
                    tot = pw_wsum(tot);
                    if (lane == 0) {
                        float logp = yw - (m + logf(tot));           // log_softmax(y) at the drawn word
                        if (bi == 0x7fffffff) { bi = 0; logp = __builtin_nanf(""); }   // all-NaN row: word 0 and a NaN log-prob
                        long long it = bi;
                        if (it == P.end_idx) it = 0;
                        const int unf = (t == 0) ? (it > 0) : (sUnf[b] && it > 0);
                        it = unf ? it : 0;
                        if (wg == 0) {
                            P.seq[(long long)b * P.max_len + t] = it;
                            P.seq_logp[(long long)b * P.max_len + t] = logp;
                            P.unfinished[b] = unf;
                            P.it[b] = it;
                        }
                        sTok[b] = it;
                        sUnf[b] = unf;
                    }
                };
                if constexpr (RES) { if (kq < B) row_work(kq); }
                else { for (int b = kq; b < B; b += 4) row_work(b); }
            }
            __syncthreads();
            PD_STAMP(13);
            int alive = 0;
            for (int b = 0; b < B; ++b) alive += sUnf[b];
            if (wg == 0 && tid == 0) P.alive[t] = alive;
            if (alive == 0) break;                                    // dcnet_rl.py:341-342: every caption has ended
            continue;
        }
        ++tag;                                                   // X4: (max, arg-max, sum exp) of every workgroup's rows
        {   // (resident variant: one row per wave, no loop — see the attention phase)
            auto row_work = [&](const int b) {
                const int row = row0 + lane;
                const bool ok = lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V;
                float x = -INFINITY;
                if (ok) x = pd_fc_score(sRed, b, lane, fcb_lane);
                float best, se;
                int bi;
                pd_fc_triple(x, row, ok, best, bi, se);
                if (lane < 4) ll_put(fcrs, (b * G + wg) * 4 + lane, lane == 0 ? best : (lane == 1 ? __int_as_float(bi) : (lane == 2 ? se : 0.f)), tag);
            };
            if constexpr (RES) { if (kq < B) row_work(kq); }
            else { for (int b = kq; b < B; b += 4) row_work(b); }
        }
        PD_STAMP(11);
        // ================= S1': [W_ih[:, h2] | W_hh] of attention_lstm and language_lstm.W_hh for timestep t + 1, while the
        // triples travel: nothing here waits for the word
        if (more) {
            acc1 = zero4; acc2 = zero4;
            pd_mma(acc1, wb, aH2);
            pd_load(wb, pT2);
            pd_mma(acc1, wa, aH1);
            pd_mma(acc2, wb, aH2);
        }
        PD_STAMP(12);
        ll_stage<256, 8>(fcrs, sF, B * G, 4, 4, tag, watch, tid);
        __syncthreads();
        // ================= S6: every workgroup combines the G triples of every row: same word everywhere
        {   // (resident variant: one row per wave, no loop — see the attention phase)
            auto row_work = [&](const int b) {
                float best = -INFINITY, tot = 0.f;
                int bi = 0x7fffffff;
                float pm[4], ps[4];
                int pi[4];
    #pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int wi = lane + 64 * i;
                    const bool have = wi < G;
                    const f32x4 e4 = have ? *reinterpret_cast<const f32x4*>(sF + (b * G + wi) * 4) : zero4;
                    pm[i] = have ? e4[0] : -INFINITY;
                    pi[i] = have ? __float_as_int(e4[1]) : 0x7fffffff;
                    ps[i] = have ? e4[2] : 0.f;
                }
    #pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (pm[i] > best || (pm[i] == best && pi[i] < bi)) { best = pm[i]; bi = pi[i]; }
                    pw_wargmax(best, bi);
    #pragma unroll
                for (int i = 0; i < 4; ++i) tot += (pm[i] == -INFINITY) ? ps[i] : ps[i] * expf(pm[i] - best);
                tot = pw_wsum(tot);
                if (lane == 0) {
                    float logp = (best - best) - logf(tot);           // log_softmax at the arg-max, as greedy_pick_k writes it
                    if (bi == 0x7fffffff) { bi = 0; logp = __builtin_nanf(""); }   // all-NaN row: word 0 and a NaN log-prob
                    long long it = bi;
                    if (it == P.end_idx) it = 0;
                    const int unf = (t == 0) ? (it > 0) : (sUnf[b] && it > 0);
                    it = unf ? it : 0;
                    if (wg == 0) {
                        P.seq[(long long)b * P.max_len + t] = it;
                        P.seq_logp[(long long)b * P.max_len + t] = logp;
                        P.unfinished[b] = unf;
                        P.it[b] = it;
                    }
                    sTok[b] = it;
                    sUnf[b] = unf;
                }
            };
            if constexpr (RES) { if (kq < B) row_work(kq); }
            else { for (int b = kq; b < B; b += 4) row_work(b); }
        }
        __syncthreads();
        PD_STAMP(13);
        int alive = 0;
        for (int b = 0; b < B; ++b) alive += sUnf[b];
        if (wg == 0 && tid == 0) P.alive[t] = alive;
        if (alive == 0) break;                                    // dcnet_rl.py:341-342: every caption has ended
    }
    // ---- an exchange of this launch timed out: never hand the result out as a decode (see encoder_persistent.hip)
    __shared__ unsigned s_bad;
    if (tid == 0) s_bad = __hip_atomic_load(P.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_bad) {
        const float qnan = __builtin_nanf("");
        if constexpr (BEAM) {
            if (wg == 0 && tid == 0) pb_poison(P.bm_best_score, P.bm_result);
        } else if (!SAMPLE && P.caps) {
            // teacher-forced: EVERY score this workgroup wrote (its vocabulary rows, all rows and timesteps) — each workgroup
            // poisons its own region after its own loop, so no later store of another workgroup can undo it
            const int row0 = wg * P.rpw;
            for (int i = tid; i < B * P.max_len * P.rpw; i += PDEC_THREADS) {
                const int row = row0 + i % P.rpw, bt_ = i / P.rpw;
                if (row < V) P.predictions[(long long)(bt_ / P.max_len) * P.ld_pred_b + (long long)(bt_ % P.max_len) * V + row] = qnan;
            }
        } else if (wg == 0) {
            for (int i = tid; i < B * P.max_len; i += PDEC_THREADS) { P.seq_logp[i] = qnan; P.seq[i] = 0; }
        }
    }
}

static int pdec_lds_floats(int B, int D, int A, bool beam = false) {
    const int base = 2 * B * (D + 4) + 4 * 3 * 256 + PDEC_MAXB * PDEC_TMAX + PDEC_MAXB * 16 + B * A + B * (D / 4) * 4 + 2 * A + B * 16 * PDEC_TS;
    // beam mode: candidates of every slice, W_hh h2 tiles, c1 | c2 table, candidate lists, scores, parents, k_left, best
    return base + (beam ? B * (D / 4) * PW_BEAM_W + 4 * 256 + 2 * PW_BEAM_K * 4 + PW_BEAM_K * PW_BEAM_K * 2 + 2 * PW_BEAM_K + 4 : 0);
}


bool dcnet_persistent_ok(const SetDcnetDims* d, int max_len) {
    const int on = env_int("SET_DEC_PERSISTENT", 1);                 // (read per call: tests and A/B runs flip it inside one process)
    const int maxb = env_int("SET_DEC_PERSISTENT_MAXB", PDEC_MAXB);
    if (!on || d->B > maxb || d->B > PDEC_MAXB || max_len < 1) return false;
    if (d->D != 64 * PDEC_KB || d->E != d->D || 2 * d->C != d->D || d->A != 512 || d->T > PDEC_TMAX) return false;   // A = 2 rows of cap_decoder_att per workgroup, 512 scores per wave pass
    const int G = d->D / 4;
    if ((d->V + G - 1) / G > 16 * PDEC_FC_TILES) return false;
    if (pdec_lds_floats(PDEC_MAXB, d->D, d->A) * (int)sizeof(float) > persistent_lds_limit()) return false;   // (a 64-KB-LDS device)
    return !persistent_disabled();
}

// exchange region of one decode: [status line | h1 | h2 | cap_decoder_att(h1) | fc triples | beam candidates] as 8-byte
// flag-in-data words.  The candidate words exist for B <= PW_BEAM_K only (B x 24 KB at D = 1024): no size for B > 4 changed
size_t dcnet_persistent_xbytes(int B, int D, int A) {
    if (B > PDEC_MAXB) return 0;
    return 128 + (size_t)B * D * 8 * 2 + (size_t)B * A * 8 + (size_t)B * (D / 4) * 32 +
           (B <= PW_BEAM_K ? (size_t)B * (D / 4) * PW_BEAM_W * 8 : 0);
}

// set_dcnet_beam_persistent: the k <= 4 hypotheses of one image as the rows of one launch (flat index k V must fit an int)
bool dcnet_persistent_beam_ok(const SetDcnetDims* d, int max_picks) {
    return d->B <= PW_BEAM_K && (long long)d->B * d->V < 0x7fffffffLL && dcnet_persistent_ok(d, max_picks);
}

// the eight instantiations: [resident (B <= 4 and T <= PDEC_TREG), general][beam, teacher-forced with last_h2, every other launch,
// Gumbel-max sampled].  (The first three columns keep the order in which the kernels have always been instantiated; the sampled
// column is appended: the instructions of the six earlier kernels stay as they were.)
#define PDEC_K(...) {reinterpret_cast<const void*>(&dcnet_persistent_k<__VA_ARGS__>)}
static PersistentKernel g_pdec_k[2][4] = {{PDEC_K(true, false, true), PDEC_K(true, true), PDEC_K(true), PDEC_K(true, false, false, true)},
                                          {PDEC_K(false, false, true), PDEC_K(false, true), PDEC_K(false), PDEC_K(false, false, false, true)}};
#undef PDEC_K

// the greedy loop after set_dcnet_begin's prologue.  `pc` = the hoisted context products (B, T, 4D), `xbuf` = exchange region
// (dcnet_persistent_xbytes).  SET_ERR_UNSUPPORTED: nothing was touched, the caller runs the per-step loop.
// samp: the sampled mode (set_dcnet_gumbel_persistent), free-running only — not with teach or beam.
int dcnet_persistent_greedy(const SetDcnetWeights* w, const SetDcnetDims* d, const float* pre1, const float* att1_c,
                            const float* mask, const float* pc, void* xbuf, long long* it, int* unfinished, int* alive,
                            long long start_idx, long long end_idx, int max_len, long long* seq, float* seq_logp,
                            hipStream_t s, const PDecTeacher* teach, const PDecBeam* beam, const PDecSample* samp) {
    if (!dcnet_persistent_ok(d, max_len)) return SET_ERR_UNSUPPORTED;
    if (samp && (teach || beam)) return SET_ERR_UNSUPPORTED;
    if (beam && (teach || !dcnet_persistent_beam_ok(d, max_len))) return SET_ERR_UNSUPPORTED;
    const int B = d->B, D = d->D, G = D / 4;
    PDecDcnetArgs P{};
    pdec_dcnet_fill(P, w, d);
    P.pre1 = pre1; P.att1_c = att1_c; P.mask = mask; P.pc = pc;
    P.status = (unsigned*)xbuf;
    char* x = pdec_dcnet_layout(P, (char*)xbuf + 128, B, D, d->A);
    P.x_fc = x; x += (size_t)B * G * 32;
    P.x_fcb = x;                                     // (B <= PW_BEAM_K: dcnet_persistent_xbytes)
    P.it = it; P.unfinished = unfinished; P.alive = alive; P.seq = seq; P.seq_logp = seq_logp;
    P.B = B; P.D = D; P.T = d->T; P.A = d->A; P.V = d->V; P.max_len = max_len; P.rpw = (d->V + G - 1) / G;
    P.start_idx = start_idx; P.end_idx = end_idx;
    if (teach) { pdec_teacher_fill(P, *teach); P.last_h2 = teach->last_h2; }
    if (beam) pdec_beam_fill(P, *beam);
    if (samp) { P.gm_seed = samp->seed; P.gm_offset = samp->offset; P.gm_inv_t = samp->inv_t; }
    const bool lh = P.caps && P.last_h2, bm = beam != nullptr, res = B <= 4 && d->T <= PDEC_TREG;
    PersistentGuard guard;
    if (guard.rc != SET_OK) return guard.rc;
    pdec_guard_fill(P, guard);
    // (beam mode: its own LDS size, at most PW_BEAM_K rows)
    const int lds = pdec_lds_floats(B, D, d->A, bm) * (int)sizeof(float);
    const int lds_max = pdec_lds_floats(bm ? PW_BEAM_K : PDEC_MAXB, D, d->A, bm) * (int)sizeof(float);
    const double wbytes = 4.0 * ((double)d->V * D + 4.0 * 4 * D * D + (double)d->A * D);
    // no word of an earlier decode may carry a tag of this one (the candidate words at the end are the beam mode's alone; the
    // sampled mode's words are the greedy launch's)
    return pdec_launch(g_pdec_k[res ? 0 : 1][bm ? 0 : lh ? 1 : samp ? 3 : 2], guard, G, lds, lds_max, &P, xbuf,
                       bm ? dcnet_persistent_xbytes(B, D, d->A) : (size_t)((char*)P.x_fcb - (char*)xbuf), s,
                       {bm ? "persistent_beam" : samp ? "persistent_gumbel" : "persistent_decode", 2.0 * B * wbytes / 4.0 * max_len, wbytes * max_len},
                       {&P.stamps, &P.stamp_wg, 13, max_len});
}

}  // namespace set
