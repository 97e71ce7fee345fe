// Persistent greedy decode of EditNet for 1 .. 16 rows (editnet_rl.py:485-549): ONE launch of D / 4 workgroups for the whole
// free-running loop, the construction of decode_persistent.hip (DCNet) (a workgroup OWNS four hidden units, streams their
// weight rows as B operands of v_mfma_f32_16x16x4_f32 — the tile has 16 batch rows, all of them used here — and finishes every
// pointwise stage itself; what other workgroups need travels as flag-in-data words, grid_barrier.h) re-cut for the things
// that grow with the batch:
//   * ONE activation buffer in LDS instead of two.  attention_lstm's W_hh h1 product of timestep t + 1 is contracted right
//     after h1 arrives (S2, with the other two products that read h1) instead of at the end of the timestep, so h1 is dead
//     after S2 and one (B, D) buffer carries h1 -> attend_cap -> c_new -> h2 -> the fc triples in turn (a wave polls the two
//     projection rows it scores with straight into registers): 66 KB at 16 rows, where two buffers + the projections + the
//     triples would need 260 KB;
//   * the caption attention is NOT recomputed by every workgroup (256 x B x T x A tanh per timestep and B x T x A floats of
//     cap_features_att from L2 per workgroup: fine at 4 rows, 10 us of a timestep at 8): its B x T scores are spread over the
//     grid exactly like the B x R visual scores — at most one of each per wave, whose cap_features_att / features_att row
//     stays in registers — and travel in one more exchange; every workgroup then runs the two (tiny) softmaxes itself;
//   * wave reductions (two softmaxes, three arg-max / sum-exp passes for four rows per wave) run on DPP row permutations +
//     four v_readlane instead of ds_bpermute butterflies (25 dependent LDS round trips per softmax: 8 us of a timestep at
//     16 rows), and the hoisted-product tables in LDS have odd row strides (no bank conflicts in the 256-thread gathers).
// (Tried and removed: "courier" waves 4-5 that do every poll / LDS fill so that the compute waves' weight requests stay in
// flight across LDS-only barriers — six waves leave 256 registers per wave, the compute path spills and it measured 20 %
// slower, EXPERIMENTS.md 5.3.)
// Per timestep (eval mode, token table):
//   S1   attention_lstm cell from the products of S2(t-1) + S1'(t-1) and the token-table row      -> h1            X1 (B, D)
//   S2   copy_lstm.x2h[:, :D] h1; the mixed tile (4 rows each of context_gate, tc_affine, [cap_decoder_att ; decoder_att]);
//        attention_lstm.W_hh h1 for timestep t + 1                                               -> projections   X2 (B, 2A)
//   S3a  this wave's caption score e_c[b, t] and visual score e[b, r]                            -> scores        X3a (B, T + R)
//   S3b  both softmaxes of every row, SelectC's arg-max; context gate of the owned columns from the hoisted P; sel /
//        gate_cmem(sel) from Mem / Q rows j*                                                     -> attend_cap    X3b (B, D)
//   S4   copy_lstm.x2h[:, D:2D] attend_cap + sum_r alpha_r Pv[b, r]                              -> c_new         X4 (B, D)
//   S5   gate_cnew rows of the owned units, copy gate                                            -> h2            X5 (B, D)
//   S6   fc rows of this workgroup, (max, first arg-max, sum exp) per batch row                   -> triples       X6 (B, G)
//   S1'  attention_lstm.W_ih[:, h2] h2 and copy_lstm.h2h h2 for timestep t + 1, while the triples travel
//   S7   every workgroup combines the G triples: same word everywhere; workgroup 0 writes seq / seq_logp
// Buffer reuse without a barrier (grid_barrier.h): every workgroup contributes to X1 and consumes exchanges in order, so a
// word of any exchange of timestep t is overwritten (timestep t + 1) only after every workgroup consumed it.
// Teacher-forced mode (set_editnet_xe_forward): words from the captions, scores written by the owners of the vocabulary rows.
// Beam mode (BEAM): the pick — slice top-k, candidate words, row merge, bookkeeping, poison — is beam_persistent.h, shared with
// DCNet's kernel and the ensemble's.  On the host the launch itself (decode_persistent.h: PersistentKernel, pdec_launch, the
// fills of the beam / teacher-forced / guard fields) and, with the ensemble launch, the fill of PDecEditArgs and the layout of
// its seven exchange regions (pdec_edit_fill / pdec_edit_layout below) are shared too.  The schedule of the phases — the order
// of the loads, the three rotating weight buffers, the exchanges and barriers — is deliberately this kernel's own (the ensemble
// kernel carries a copy); of the arithmetic between those lines pd_sum4 / pd_sum4p, pd_clamp_tok, pw_cap_softmax,
// pw_vis_softmax64, pw_cnew_gates and pw_copy_gate are leaves of decode_persistent.h, shared.  The cell update of S1, the poll and
// the scores of S3a, the context gate and the fc score / triple stay written out here: as leaves each of them moved the AGPR
// count of an instantiation of this kernel (profiles/pdec_leaves_resources.json).
#include "beam_persistent.h"
#include "philox.h"

namespace set {

namespace {

constexpr int PW_U = 16;           // 16-byte requests a lane keeps in flight while it fills LDS from an exchange buffer
// (PW_BEAM_K, PW_BEAM_W, the candidate layout of the beam mode: decode_persistent.h — DCNet's kernel publishes the same words)
// visual scores per row in LDS and in the exchange: 64, or the region capacity above that
constexpr int pw_vcols(int rreg) { return rreg > 64 ? rreg : 64; }

}  // namespace

// BEAM: the rows are the k <= PW_BEAM_K hypotheses of ONE image and the loop is the reference's beam search (editnet.py:643-713)
// instead of the greedy loop — see "beam mode" below.
// RREG: region capacity of the hoisted region products in LDS.  PDEC_RREG (36) for fixed features; PDEC_RREG_WIDE (128) for the
// beam search over adaptive features (editnet_adaptive.py:614-735): up to 128 zero-padded regions whose scores are masked to
// -1e10 where P.rmask == 0 (step_attention_k), two scores per lane in the softmax.  The masked weights underflow to exactly 0,
// which is the reference's truncation to max(att_masks.sum(1)): all rows of a beam launch are the same image.
// SAMPLE: the greedy loop with the Gumbel-max draw (philox.h; set_editnet_gumbel_persistent) in place of the arg-max — "sampled
// mode" below.  An arg-max over perturbed scores, so the grid combines it exactly as it combines the greedy one.
template <bool BEAM, int RREG, bool SAMPLE = false>
__global__ void __launch_bounds__(PDEC_THREADS, 1) editnet_persistent_wide_k(const PDecEditArgs P) {
    constexpr int RS = pdec_rs(RREG), VC = pw_vcols(RREG);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ long long sTok[PDW_MAXB];
    __shared__ int sUnf[PDW_MAXB], sJs[PDW_MAXB];
    __shared__ float sWj[PDW_MAXB];
    const int tid = threadIdx.x, lane = tid & 63, kq = tid >> 6, r = lane & 15, g = lane >> 4;
    constexpr bool worker = true;
    const int B = P.B, D = P.D, T = P.T, R = P.R, A = P.A, V = P.V;
    const int KQ = D >> 2, LDH = D + 4;
    const int wg = (int)blockIdx.x, u0 = wg * 4, G = (int)gridDim.x;
    float* sX = smem;                                    // (B, LDH): h1 -> attend_cap -> c_new -> h2 -> triples (B, G, 4) in turn
    float* sRed = sX + B * LDH;                          // [4 waves][3 tiles][16][16]
    float* sAlc = sRed + 4 * 3 * 256;                    // (B, TMAX) caption scores -> weights
    float* sAlv = sAlc + PDW_MAXB * PDEC_TMAX;           // (B, VC) visual scores -> weights
    float* sG = sAlv + PDW_MAXB * VC;                    // (B, 16) copy_lstm gate pre-activations
    float* sZ = sG + PDW_MAXB * 16;                      // (B, 8) [sum alpha P_z (4) | sum alpha P_s (4)] of the owned columns
    float* sM = sZ + PDW_MAXB * 8;                       // (B, 8) [context_gate.W h1 (4) | tc_affine.W h1 (4)]
    float* sPv = sM + PDW_MAXB * 8;                      // (B, 16, RREG) hoisted region products of the owned gate rows
    float* sPz = sPv + B * 16 * RS;                   // (B, 8, TMAX) hoisted caption-context products of the owned columns
    float* sCon = sPz + B * 8 * PDEC_TS;               // [cap_decoder_att.b | cap_full_att.w | decoder_att.b | full_att.w] (4, A)
    const float* sF = sX;
    // beam mode only: every workgroup's per-slice candidates, the previous timestep's h2h products (added through the parent
    // map), the cell states on their way through the parent map, the per-row candidate lists of the pick
    float* sFB = sCon + 4 * A;                           // (B, G, PW_BEAM_W)
    float* sRedP = sFB + (BEAM ? B * G * PW_BEAM_W : 0); // [4 waves][16][16]
    float* sCst = sRedP + (BEAM ? 4 * 256 : 0);          // (2, B, 4) c1 | c2 of the owned units
    float* sCand = sCst + (BEAM ? 2 * PW_BEAM_K * 4 : 0);// (B, K, 2) (score, flat index) of every row's best K candidates
    __shared__ int sPar[PW_BEAM_K];                      // parent slot of every slot (identity before the first pick)
    __shared__ float sScore[PW_BEAM_K];                  // running scores of the slots (-inf = dead)
    __shared__ int sKleft;
    __shared__ float sBest;                              // best completed hypothesis so far
    const LLWatch watch{P.status, P.fault, P.spin_limit};

#define PW_SYNC() __syncthreads()
#define PW_STAGE(RS, DST, ROWS, COLS, LD) ll_stage<PDEC_THREADS, PW_U>(RS, DST, ROWS, COLS, LD, tag, watch, tid)

    // ---- weight tiles of this lane (workers)
    const long long grow = (long long)(r >> 2) * D + u0 + (r & 3);       // gate row of the 4D-row matrices
    const int kcol = (kq & 3) * KQ + 4 * g;
    const float* pT0 = P.al_wih + grow * P.ld_ih + 2 * D + kcol;
    const float* pT1 = P.al_whh + grow * D + kcol;
    const float* pT2 = P.cl_h2h_w + grow * D + kcol;
    const float* pT3 = P.cl_x2h_w + grow * P.ld_x2h + kcol;
    const float* pT5 = P.cl_x2h_w + grow * P.ld_x2h + D + kcol;
    const float* pT4;                                    // mixed tile: rows 0-3 context_gate, 4-7 tc_affine, 8-11 attention projections
    {
        const int j = wg * 4 + (r & 3);                  // row of the stacked [cap_decoder_att ; decoder_att] (2A rows)
        pT4 = r < 4 ? P.ca_gate_w + (long long)(u0 + r) * 3 * D + D + kcol
            : r < 8 ? P.ca_tc_w + (long long)(u0 + r - 4) * 2 * D + D + kcol
                    : (j < A ? P.ca_dec_w + (long long)j * D : P.va_dec_w + (long long)(j - A) * D) + kcol;
    }
    const bool v4 = r < 12;
    const bool v6 = r < 4;
    const float* pT6 = P.cl_cnew_w + (long long)(u0 + (r & 3)) * D + kcol;
    const int row0 = wg * P.rpw;
    const float* pF[PDEC_FC_TILES];
    bool vF[PDEC_FC_TILES];
#pragma unroll
    for (int j = 0; j < PDEC_FC_TILES; ++j) {
        const int row = row0 + 16 * j + r;
        vF[j] = (16 * j + r < P.rpw) && row < V;
        pF[j] = P.fc_w + (long long)(vF[j] ? row : 0) * D + kcol;
    }
    const float fcb_lane = (lane < 16 * PDEC_FC_TILES && lane < P.rpw && row0 + lane < V) ? P.fc_b[row0 + lane] : 0.f;
    const int arow = (r < B ? r : B - 1) * LDH;          // rows >= B repeat the last one: their outputs are never read
    const float* aX = sX + arow + kcol;

    // ---- thread roles (workers) and their loop-invariant operands
    const bool pair = worker && tid < B * 4;             // (batch row, owned unit): the two cells, the context gate, the copy gate
    const int pb = tid >> 2, pu = tid & 3, pd = u0 + pu;
    const bool gcol = worker && tid < B * 16;            // (batch row, gate row) of copy_lstm's hoisted region products
    const int cb = tid >> 4, crr = tid & 15;
    const long long ccol = (long long)(crr >> 2) * D + u0 + (crr & 3);
    const bool zrole = worker && tid < B * 8;            // (batch row, [z | s] column) of the hoisted caption-context products
    const int zb = tid >> 3, zc8 = tid & 7;
    float c1 = 0.f, c2 = 0.f, pre[4] = {0.f, 0.f, 0.f, 0.f};
    float bg = 0.f, bsc = 0.f, btc = 0.f, bcn = 0.f, bcm = 0.f, b2 = 0.f;
    if (pair) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[q] = P.pre1[(long long)pb * 4 * D + (long long)q * D + pd];
        bg = P.ca_gate_b[pd]; bsc = P.ca_sc_b[pd]; btc = P.ca_tc_b[pd]; bcn = P.cl_cnew_b[pd]; bcm = P.cl_cmem_b[pd];
    }
    if (gcol) {
        for (int rr = 0; rr < RREG; ++rr) sPv[tid * RS + rr] = rr < R ? P.pv[((long long)cb * R + rr) * 4 * D + ccol] : 0.f;
        b2 = P.cl_x2h_b[ccol] + P.cl_h2h_b[ccol];
    }
    if (zrole)
        for (int tt = 0; tt < PDEC_TMAX; ++tt)
            sPz[tid * PDEC_TS + tt] = tt < T ? P.capP[((long long)zb * T + tt) * 2 * D + (zc8 < 4 ? u0 + zc8 : D + u0 + zc8 - 4)] : 0.f;
    if (worker)
        for (int i = tid; i < A; i += PDEC_THREADS) {
            sCon[i] = P.ca_dec_b[i]; sCon[A + i] = P.ca_full_w[i]; sCon[2 * A + i] = P.va_dec_b[i]; sCon[3 * A + i] = P.va_full_w[i];
        }
    const int a_lo = lane * 4, a_hi = lane * 4 + 256;
    const float cbf = P.ca_full_b[0], vbf = P.va_full_b[0];
    // the ONE caption score and the ONE visual score this wave owns: index s = wg + G * wave over (b, t) / (b, r); the
    // cap_features_att / features_att rows they need are loop-invariant and stay in registers
    const int s_idx = wg + G * (kq & 3);
    const bool cs_on = worker && s_idx < B * T, vs_on = worker && s_idx < B * R;
    const int cs_b = cs_on ? s_idx / T : 0, cs_t = cs_on ? s_idx % T : 0;
    const int vs_b = vs_on ? s_idx / R : 0, vs_r = vs_on ? s_idx % R : 0;
    const f32x4 ca1_0 = *reinterpret_cast<const f32x4*>(P.att1_c + ((long long)cs_b * T + cs_t) * A + a_lo);
    const f32x4 ca1_1 = *reinterpret_cast<const f32x4*>(P.att1_c + ((long long)cs_b * T + cs_t) * A + a_hi);
    const float cs_mask = P.mask[(long long)cs_b * T + cs_t];
    const f32x4 va1_0 = *reinterpret_cast<const f32x4*>(P.att1 + ((long long)vs_b * R + vs_r) * A + a_lo);
    const f32x4 va1_1 = *reinterpret_cast<const f32x4*>(P.att1 + ((long long)vs_b * R + vs_r) * A + a_hi);
    bool vs_pad = false;                                 // adaptive features: this wave's region is padding (editnet_adaptive.py:453)
    if constexpr (RREG > 64) vs_pad = vs_on && P.rmask[(long long)vs_b * R + vs_r] == 0.f;
    // exchange buffers
    const __amdgpu_buffer_rsrc_t h1rs = __builtin_amdgcn_make_buffer_rsrc(P.x_h1, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t a2rs = __builtin_amdgcn_make_buffer_rsrc(P.x_a2, 0, B * 2 * A * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t gtrs = __builtin_amdgcn_make_buffer_rsrc(P.x_gt, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t csrs = __builtin_amdgcn_make_buffer_rsrc(P.x_cs, 0, B * PDEC_TMAX * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t vsrs = __builtin_amdgcn_make_buffer_rsrc(P.x_vs, 0, B * (RREG > 64 ? pw_vcols(R) : 64) * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t cnrs = __builtin_amdgcn_make_buffer_rsrc(P.x_cn, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t h2rs = __builtin_amdgcn_make_buffer_rsrc(P.x_h2, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t fcrs = __builtin_amdgcn_make_buffer_rsrc(P.x_fc, 0, B * G * 32, 0x00027000);
    const __amdgpu_buffer_rsrc_t fbrs = __builtin_amdgcn_make_buffer_rsrc(BEAM ? P.x_fcb : P.x_fc, 0, BEAM ? B * G * PW_BEAM_W * 8 : 32, 0x00027000);

    // ---- initial state (init_hidden_state, editnet.py:494-495): zeros; every row is fed <start>
    if (tid < B) { sTok[tid] = P.start_idx; sUnf[tid] = 1; }
    if (BEAM && tid < PW_BEAM_K) { sPar[tid] = tid; sScore[tid] = tid == 0 ? 0.f : -INFINITY; }   // step 1: all rows are identical, only row 0 counts
    if (BEAM) for (int i = tid; i < 4 * 256; i += PDEC_THREADS) sRedP[i] = 0.f;                   // h2h h2 of the zero initial state
    if (BEAM && tid == 0) {
        sKleft = B; sBest = -INFINITY;
        if (wg == 0) { P.bm_best_score[0] = -INFINITY; P.bm_best_word[0] = 0; P.bm_result[0] = -1; P.bm_result[1] = -1; P.bm_result[2] = B; P.bm_result[3] = 0; }
    }
    __syncthreads();

    // weight tiles rotate through three register buffers (one workgroup per CU: 512 registers per lane):
    //   X1: wb<-T3 wa<-T4 wc<-T1 | after the projections' poll: wb<-T5 | after the scores' poll: wa<-T6 wc<-F0 | S4: wb<-F1 |
    //   S5: wa<-F2 | S6: wc<-T0' wb<-T2'
    f32x4 wa[PDEC_KB], wb[PDEC_KB], wc[PDEC_KB];
    unsigned tag = 0;
    {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // gate products of the NEXT timestep that do not depend on the word: acc1n = W_hh h1 (S2), acc1 = acc1n + W_ih[:, h2] h2
    // and acc2 = h2h h2 (S1', while the fc triples travel).  t = 0: h1 = h2 = 0.
    f32x4 acc1 = zero4, acc2 = zero4, acc1n = zero4;
    for (int t = 0; t < P.max_len; ++t) {
        // ================= S1: attention_lstm cell (h1)
        PD_STAMP(0);
        float tg[4] = {0.f, 0.f, 0.f, 0.f}, ttc = 0.f, tcg = 0.f;
        int bt = B;                                              // teacher-forced: rows whose caption is still running (sorted batch)
        if (P.caps) {
            bt = 0;
            for (int b = 0; b < B; ++b) bt += P.dlen[b] > t ? 1 : 0;
            if (bt == 0) break;
        }
        if (pair) {
            long long tok = P.caps ? P.caps[(long long)pb * P.caps_stride + t] : sTok[pb];
            tok = pd_clamp_tok(tok, V);
            const float* trow = P.tok_table + tok * P.ld_tab + pd;
#pragma unroll
            for (int q = 0; q < 4; ++q) tg[q] = trow[(long long)q * D];
            ttc = trow[4LL * D];
            tcg = trow[5LL * D];
        }
        if (worker) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = acc1[e];
        }
        if (BEAM && pair) { sCst[pb * 4 + pu] = c1; sCst[PW_BEAM_K * 4 + pb * 4 + pu] = c2; }
        PW_SYNC();
        // beam mode: slot pb continues hypothesis sPar[pb] of the previous timestep — its cell states and the gate products
        // that were contracted before the pick (S2 / S1' of the previous timestep) are read through the parent map
        const int par = BEAM ? sPar[pair ? pb : 0] : pb;
        if (BEAM && pair) { c1 = sCst[par * 4 + pu]; c2 = sCst[PW_BEAM_K * 4 + par * 4 + pu]; }
        ++tag;                                                   // X1: h1
        if (pair && !(P.test_stall && wg == 0)) {
            float gq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = par * 16 + q * 4 + pu;
                gq[q] = ((((sRed[o] + sRed[3 * 256 + o]) + sRed[6 * 256 + o]) + sRed[9 * 256 + o]) + pre[q]) + tg[q];
            }
            const float ai = pd_sigm(gq[0]), af = pd_sigm(gq[1]), ag = tanhf(gq[2]), ao = pd_sigm(gq[3]);
            c1 = af * c1 + ai * ag;
            ll_put(h1rs, pb * D + pd, ao * tanhf(c1), tag);
        }
        if (worker) {
            pd_load(wb, pT3);
            pd_load_if(wa, pT4, v4);
            pd_load(wc, pT1);
        }
        PD_STAMP(1);
        PW_STAGE(h1rs, sX, B, D, LDH);
        PW_SYNC();
        // ================= S2: copy_lstm.x2h[:, :D] h1; context_gate / tc_affine rows of the owned columns, 4 projection rows;
        // attention_lstm.W_hh h1 for the next timestep (h1's last reader: the buffer is free after this)
        PD_STAMP(2);
        if (worker) {
            pd_mma(acc2, wb, aX);
            f32x4 accm = zero4;
            pd_mma(accm, wa, aX);
            acc1n = zero4;
            pd_mma(acc1n, wc, aX);
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = accm[e];
        }
        PW_SYNC();
        PD_STAMP(3);
        ++tag;                                                   // X2: [cap_decoder_att(h1) | decoder_att(h1)]
        if (gcol && crr < 12) {
            const int o = cb * 16 + crr;
            const float v = pd_sum4(sRed, 1, o);
            if (crr < 8) sM[cb * 8 + crr] = v;
            else ll_put(a2rs, cb * 2 * A + wg * 4 + crr - 8, v, tag);
        }
        // ================= S3a: this wave's caption score (editnet.py:370-374) and visual score (:443-445).  The two projection
        // rows it needs (8 floats per lane each) are polled straight into registers — nothing of this wave is in flight ahead
        // of the poll — and only then are the next weight tiles requested: they stream under X3a / X3b
        f32x4 pc0 = zero4, pc1 = zero4, pv0 = zero4, pv1 = zero4;
        if (cs_on || vs_on) {
            const int wc_ = cs_b * 2 * A, wv_ = vs_b * 2 * A + A;
            unsigned spins = 0;
            unsigned long long t0 = 0;
            gb_u32x4 q[8];
            for (;;) {
                asm volatile("" ::: "memory");
                q[0] = ll_req2(a2rs, wc_ + a_lo); q[1] = ll_req2(a2rs, wc_ + a_lo + 2);
                q[2] = ll_req2(a2rs, wc_ + a_hi); q[3] = ll_req2(a2rs, wc_ + a_hi + 2);
                q[4] = ll_req2(a2rs, wv_ + a_lo); q[5] = ll_req2(a2rs, wv_ + a_lo + 2);
                q[6] = ll_req2(a2rs, wv_ + a_hi); q[7] = ll_req2(a2rs, wv_ + a_hi + 2);
                bool ok = true;
#pragma unroll
                for (int i = 0; i < 8; ++i) ok = ok && ll_ok2(q[i], tag);
                if (__all(ok) || ll_giveup(spins, t0, watch)) break;
            }
            pc0 = (f32x4){__uint_as_float(q[0].x), __uint_as_float(q[0].z), __uint_as_float(q[1].x), __uint_as_float(q[1].z)};
            pc1 = (f32x4){__uint_as_float(q[2].x), __uint_as_float(q[2].z), __uint_as_float(q[3].x), __uint_as_float(q[3].z)};
            pv0 = (f32x4){__uint_as_float(q[4].x), __uint_as_float(q[4].z), __uint_as_float(q[5].x), __uint_as_float(q[5].z)};
            pv1 = (f32x4){__uint_as_float(q[6].x), __uint_as_float(q[6].z), __uint_as_float(q[7].x), __uint_as_float(q[7].z)};
        }
        pd_load(wb, pT5);                                        // S4's tile: one tile ahead of the (small) score exchange
        PD_STAMP(4);
        float cs_val = 0.f, vs_val = 0.f;
        if (cs_on) {
            const f32x4 x0 = ca1_0 + (pc0 + *reinterpret_cast<const f32x4*>(sCon + a_lo));
            const f32x4 x1 = ca1_1 + (pc1 + *reinterpret_cast<const f32x4*>(sCon + a_hi));
            const f32x4 cfw0 = *reinterpret_cast<const f32x4*>(sCon + A + a_lo), cfw1 = *reinterpret_cast<const f32x4*>(sCon + A + a_hi);
            const float sc = pw_wsum(pd_score8(x0, x1, cfw0, cfw1));
            cs_val = (cs_mask == 0.f) ? -1e10f : (sc + cbf);
        }
        if (vs_on) {
            const f32x4 x0 = va1_0 + (pv0 + *reinterpret_cast<const f32x4*>(sCon + 2 * A + a_lo));
            const f32x4 x1 = va1_1 + (pv1 + *reinterpret_cast<const f32x4*>(sCon + 2 * A + a_hi));
            const f32x4 vfw0 = *reinterpret_cast<const f32x4*>(sCon + 3 * A + a_lo), vfw1 = *reinterpret_cast<const f32x4*>(sCon + 3 * A + a_hi);
            float sc = vfw0[0] * fmaxf(x0[0], 0.f) + vfw0[1] * fmaxf(x0[1], 0.f) + vfw0[2] * fmaxf(x0[2], 0.f) + vfw0[3] * fmaxf(x0[3], 0.f);
            sc += vfw1[0] * fmaxf(x1[0], 0.f) + vfw1[1] * fmaxf(x1[1], 0.f) + vfw1[2] * fmaxf(x1[2], 0.f) + vfw1[3] * fmaxf(x1[3], 0.f);
            vs_val = pw_wsum(sc) + vbf;
            if (vs_pad) vs_val = -1e10f;
        }
        ++tag;                                                   // X3a: caption scores + visual scores
        if (cs_on && lane == 0) ll_put(csrs, cs_b * T + cs_t, cs_val, tag);
        if (vs_on && lane == 0) ll_put(vsrs, vs_b * R + vs_r, vs_val, tag);
        PD_STAMP(5);
        PW_STAGE(csrs, sAlc, B, T, PDEC_TMAX);                   // (T and R are even: editnet_persistent_wide_ok)
        PW_STAGE(vsrs, sAlv, B, R, VC);
        pd_load_if(wa, pT6, v6);                                 // S5's (short) tile and fc's first one stream under the softmaxes
        pd_load_if(wc, pF[0], vF[0]);                            // and the attend_cap exchange
        PW_SYNC();
        PD_STAMP(6);
        // ================= S3b: both softmaxes of every row, SelectC's arg-max (editnet.py:375-376, :409-416, :446)
        if (worker) {
            for (int b = kq; b < B; b += 4) {
                pw_cap_softmax(sAlc + b * PDEC_TMAX, T, lane, &sJs[b], &sWj[b]);
                if constexpr (RREG <= 64) {
                    pw_vis_softmax64(sAlv + b * 64, R, lane);
                } else {                                         // up to 128 scores: lane l holds regions l and l + 64
                    const int l1 = lane + 64;
                    const float sc0 = lane < R ? sAlv[b * VC + lane] : -INFINITY, sc1 = l1 < R ? sAlv[b * VC + l1] : -INFINITY;
                    const float m = pw_wmax(fmaxf(sc0, sc1));
                    const float ex0 = lane < R ? expf(sc0 - m) : 0.f, ex1 = l1 < R ? expf(sc1 - m) : 0.f;
                    const float sum = pw_wsum(ex0 + ex1);
                    if (lane < R) sAlv[b * VC + lane] = ex0 / sum;
                    if (l1 < R) sAlv[b * VC + l1] = ex1 / sum;
                }
            }
        }
        PW_SYNC();
        if (zrole) {
            float s = 0.f;
            for (int tt = 0; tt < T; ++tt) s += sAlc[zb * PDEC_TMAX + tt] * sPz[tid * PDEC_TS + tt];
            sZ[zb * 8 + zc8] = s;
        }
        PW_SYNC();
        PD_STAMP(7);
        ++tag;                                                   // X3b: attend_cap columns
        float selv = 0.f, cmemv = 0.f;
        if (pair) {
            // context gate of column pd (editnet.py:378-380; operand order as caption_attention_body in attention.hip)
            const float z = ((sM[pb * 8 + pu] + tcg) + sZ[pb * 8 + pu]) + bg;
            const float zt = pd_sigm(z);
            const float o = zt * tanhf(sZ[pb * 8 + 4 + pu] + bsc) + (1.f - zt) * tanhf((sM[pb * 8 + 4 + pu] + ttc) + btc);
            ll_put(gtrs, pb * D + pd, o, tag);
            const int js = sJs[pb];
            const float wj = sWj[pb];
            selv = P.Mem[((long long)pb * T + js) * D + pd] * wj;
            cmemv = P.memQ[((long long)pb * T + js) * D + pd] * wj;
        }
        PW_STAGE(gtrs, sX, B, D, LDH);
        PW_SYNC();
        PD_STAMP(8);
        // ================= S4: copy_lstm.x2h[:, D:2D] attend_cap; hoisted region products -> c_new
        if (worker) {
            pd_mma(acc2, wb, aX);
            pd_load_if(wb, pF[1], vF[1]);
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 2) * 256 + (4 * g + e) * 16 + r] = acc2[e];
        }
        PW_SYNC();
        if (gcol) {
            const int o = cb * 16 + crr;
            float s = 0.f;
            for (int rr = 0; rr < R; ++rr) s += sAlv[cb * VC + rr] * sPv[tid * RS + rr];
            float g2 = pd_sum4(sRed, 2, o);
            if (BEAM) g2 += pd_sum4p(sRedP, sPar[cb] * 16 + crr);   // + copy_lstm.h2h h2 of the PARENT hypothesis (S1' of the previous timestep)
            sG[o] = (g2 + s) + b2;
        }
        PW_SYNC();
        PD_STAMP(9);
        ++tag;                                                   // X4: c_new
        float cnv = 0.f, ogv = 0.f;
        if (pair) {
            pw_cnew_gates(sG + pb * 16 + pu, c2, cnv, ogv);
            ll_put(cnrs, pb * D + pd, cnv, tag);
        }
        PW_STAGE(cnrs, sX, B, D, LDH);
        PW_SYNC();
        PD_STAMP(10);
        // ================= S5: gate_cnew rows of the owned units, copy gate (editnet.py:281-283) -> c2, h2
        if (worker) {
            f32x4 acc5 = zero4;
            pd_mma(acc5, wa, aX);
            pd_load_if(wa, pF[2], vF[2]);
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = acc5[e];
        }
        PW_SYNC();
        ++tag;                                                   // X5: h2
        if (pair) {
            const float a = pd_sum4(sRed, 0, pb * 16 + pu) + bcn;
            ll_put(h2rs, pb * D + pd, pw_copy_gate(a, cmemv, bcm, selv, cnv, ogv, c2), tag);
        }
        PD_STAMP(11);
        PW_STAGE(h2rs, sX, B, D, LDH);
        PW_SYNC();
        PD_STAMP(12);
        // ================= S6: fc over this workgroup's vocabulary rows, local (max, first arg-max, sum exp) per batch row
        const bool more = t + 1 < P.max_len;
        if (worker) {
            f32x4 accf0 = zero4, accf1 = zero4, accf2 = zero4;
            pd_mma(accf0, wc, aX);
            if (more) pd_load(wc, pT0);
            pd_mma(accf1, wb, aX);
            if (more) pd_load(wb, pT2);
            pd_mma(accf2, wa, aX);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = accf0[e];
                sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = accf1[e];
                sRed[(kq * 3 + 2) * 256 + (4 * g + e) * 16 + r] = accf2[e];
            }
        }
        PW_SYNC();
        PD_STAMP(13);
        if (P.caps) {
            // teacher-forced: the scores themselves, rows 0 .. bt - 1 (editnet.py:546: predictions[:batch_size_t, t, :] = preds)
            if (worker) {
                for (int b = kq; b < bt; b += 4) {
                    const int j = lane >> 4, rr = lane & 15, row = row0 + lane;
                    if (lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V) {
                        const int o = j * 256 + b * 16 + rr;
                        P.predictions[(long long)b * P.ld_pred_b + (long long)t * V + row] =
                            (((sRed[o] + sRed[3 * 256 + o]) + sRed[6 * 256 + o]) + sRed[9 * 256 + o]) + fcb_lane;
                    }
                }
                if (more) {                                      // S1' (see below)
                    acc1 = acc1n;
                    pd_mma(acc1, wc, aX);
                    acc2 = zero4;
                    pd_mma(acc2, wb, aX);
                }
            }
            PW_SYNC();                                           // sRed is rewritten by the next timestep's S1
            continue;
        }
        if constexpr (BEAM) {
            // ================= beam mode (editnet.py:654-699; the pick of beam_persistent.h):
            // X6 carries, per row and vocabulary slice, (max, sum exp) and the slice's B best (score, word) pairs — a global
            // top-B over B x V candidates takes at most B from one slice
            ++tag;
            if (kq < B) {
                const int b = kq;
                const int j = lane >> 4, rr = lane & 15, row = row0 + lane;
                const bool ok = lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V;
                float x = -INFINITY;
                if (ok) {
                    const int o = j * 256 + b * 16 + rr;
                    x = (((sRed[o] + sRed[3 * 256 + o]) + sRed[6 * 256 + o]) + sRed[9 * 256 + o]) + fcb_lane;
                }
                pb_vals cvv;
                pb_idxs cii;
                pb_slice_topk(x, row, ok, B, cvv, cii);
                const float mx = cvv[0];
                float se = (ok && mx > -INFINITY) ? expf(x - mx) : 0.f;
                se = pw_wsum(se);
                pb_publish(fbrs, (b * G + wg) * PW_BEAM_W, lane, mx, se, cvv, cii, tag);
            }
            // S1' (see the greedy path); copy_lstm.h2h h2 goes to LDS: the next timestep adds it through the parent map
            if (more) {
                acc1 = acc1n;
                pd_mma(acc1, wc, aX);
                f32x4 accp = zero4;
                pd_mma(accp, wb, aX);
#pragma unroll
                for (int e = 0; e < 4; ++e) sRedP[kq * 256 + (4 * g + e) * 16 + r] = accp[e];
                acc2 = zero4;
            }
            PW_SYNC();
            PW_STAGE(fbrs, sFB, B * G, PW_BEAM_W, PW_BEAM_W);
            PW_SYNC();
            // ---- every workgroup runs the same pick.  Wave j: log-sum-exp of row j and its B best candidates
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
            PW_SYNC();
            if (tid == 0)                                        // the pick itself and its bookkeeping (beam_persistent.h)
                pb_pick(sCand, sScore, sTok, sPar, &sKleft, &sBest, P.bm_hist_par, P.bm_hist_word, P.bm_best_score, P.bm_best_word,
                        P.bm_result, V, P.end_idx, t, B, wg == 0, P.bm_hist_score);
            PW_SYNC();
            PD_STAMP(16);
            if (sKleft == 0) break;                              // every hypothesis has ended (editnet.py:700-701)
            continue;
        }
        if constexpr (SAMPLE) {
            // ================= sampled mode: the word of row b is the first maximum of s[v] = y[v] + g[v], y = fl(x inv_t), g = the
            // noise keyed by (seed, offset, b, t, v) — the per-step pick's (epilogue.hip gumbel_pick_k) definition, word for word.
            // X6 carries per (row, slice) the four words the combine needs, in the greedy triple's region (its pad word is used):
            // [log-sum-exp of y over the slice (max y and sum exp folded into one word) | first arg-max of s | max s | y there].
            // A lane owns ONE vocabulary row; the slice boundaries are not quad-aligned, so every lane calls Philox for its own
            // quad and selects its word.
            ++tag;
            for (int b = kq; b < B; b += 4) {
                const int row = row0 + lane;
                const bool ok = lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V;
                float y = -INFINITY, sv = -INFINITY;
                if (ok) {
                    const int j = lane >> 4, rr = lane & 15, o = j * 256 + b * 16 + rr;
                    const float x = (((sRed[o] + sRed[3 * 256 + o]) + sRed[6 * 256 + o]) + sRed[9 * 256 + o]) + fcb_lane;
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
            }
            if (more) {                                              // S1' (see the greedy path)
                acc1 = acc1n;
                pd_mma(acc1, wc, aX);
                acc2 = zero4;
                pd_mma(acc2, wb, aX);
            }
            PW_SYNC();
            PD_STAMP(14);
            PW_STAGE(fcrs, sX, B * G, 4, 4);
            PW_SYNC();
            PD_STAMP(15);
            // ---- every workgroup combines the G entries of every row in slice order: same word everywhere
            for (int b = kq; b < B; b += 4) {
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
                const int mine = bi;                                 // this lane's candidate; the winner's y travels from its lane
                pw_wargmax(best, bi);
                const unsigned long long own = __ballot(mine == bi && bi != 0x7fffffff);
                const float yw = own ? pw_lane(yb, __ffsll((long long)own) - 1) : 0.f;
                const float m = pw_wmax(fmaxf(fmaxf(pl[0], pl[1]), fmaxf(pl[2], pl[3])));
                float tot = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) tot += (pl[i] == -INFINITY) ? 0.f : (m == -INFINITY ? pl[i] : expf(pl[i] - m));
                tot = pw_wsum(tot);
                if (lane == 0) {
                    float logp = yw - (m + logf(tot));               // log_softmax(y) at the drawn word
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
            }
            PW_SYNC();
            PD_STAMP(16);
            int alive = 0;
            for (int b = 0; b < B; ++b) alive += sUnf[b];
            if (wg == 0 && tid == 0) P.alive[t] = alive;
            if (alive == 0) break;
            continue;
        }
        ++tag;                                                   // X6: triples
        if (worker) {
            for (int b = kq; b < B; b += 4) {
                const int j = lane >> 4, rr = lane & 15, row = row0 + lane;
                const bool ok = lane < 16 * PDEC_FC_TILES && lane < P.rpw && row < V;
                float x = -INFINITY;
                if (ok) {
                    const int o = j * 256 + b * 16 + rr;
                    x = (((sRed[o] + sRed[3 * 256 + o]) + sRed[6 * 256 + o]) + sRed[9 * 256 + o]) + fcb_lane;
                }
                float best = -INFINITY;
                int bi = 0x7fffffff;
                if (x > best) { best = x; bi = row; }
                pw_wargmax(best, bi);
                // (a NaN score never wins a comparison: it reaches the sum instead and the row's log-prob is NaN)
                float se = ok ? expf(x - best) : 0.f;
                if (best == -INFINITY) se = ok ? x : 0.f;            // no finite score here: 0 for an empty range, NaN for NaN scores
                se = pw_wsum(se);
                if (lane < 4) ll_put(fcrs, (b * G + wg) * 4 + lane, lane == 0 ? best : (lane == 1 ? __int_as_float(bi) : (lane == 2 ? se : 0.f)), tag);
            }
            // ================= S1': attention_lstm.W_ih[:, h2] h2 (+ W_hh h1 from S2) and copy_lstm.h2h h2 for timestep t + 1,
            // while the triples travel: nothing here waits for the word
            if (more) {
                acc1 = acc1n;
                pd_mma(acc1, wc, aX);
                acc2 = zero4;
                pd_mma(acc2, wb, aX);
            }
        }
        PW_SYNC();                                               // (h2's last readers are done: the buffer takes the triples)
        PD_STAMP(14);
        PW_STAGE(fcrs, sX, B * G, 4, 4);
        PW_SYNC();
        PD_STAMP(15);
        // ================= S7: every workgroup combines the G triples of every row: same word everywhere
        if (worker) {
            for (int b = kq; b < B; b += 4) {
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
            }
        }
        PW_SYNC();
        PD_STAMP(16);
        int alive = 0;
        for (int b = 0; b < B; ++b) alive += sUnf[b];
        if (wg == 0 && tid == 0) P.alive[t] = alive;
        if (alive == 0) break;                                    // editnet_rl.py:546: every caption has ended
    }
    }
#undef PW_STAGE
#undef PW_SYNC
    __shared__ unsigned s_bad;
    if (tid == 0) s_bad = __hip_atomic_load(P.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_bad && worker) {                                        // an exchange timed out: never hand this out as a decode
        const float qnan = __builtin_nanf("");
        if (P.caps) {                                              // teacher-forced: every score this workgroup wrote (see decode_persistent.hip)
            const int row0_ = wg * P.rpw;
            for (int i = tid; i < B * P.max_len * P.rpw; i += PDEC_THREADS) {
                const int row = row0_ + i % P.rpw, bt_ = i / P.rpw;
                if (row < V) P.predictions[(long long)(bt_ / P.max_len) * P.ld_pred_b + (long long)(bt_ % P.max_len) * V + row] = qnan;
            }
        } else if (BEAM) {
            if (wg == 0 && tid == 0) pb_poison(P.bm_best_score, P.bm_result);
        } else if (wg == 0) {
            for (int i = tid; i < B * P.max_len; i += PDEC_THREADS) { P.seq_logp[i] = qnan; P.seq[i] = 0; }
        }
    }
}

static int pwide_lds_floats(int B, int D, int A, bool beam = false, int rreg = PDEC_RREG) {
    const int base = B * (D + 4) + 4 * 3 * 256 + PDW_MAXB * (PDEC_TMAX + pw_vcols(rreg) + 16 + 8 + 8) + B * 16 * pdec_rs(rreg) + B * 8 * PDEC_TS + 4 * A;
    return base + (beam ? B * (D / 4) * PW_BEAM_W + 4 * 256 + 2 * PW_BEAM_K * 4 + PW_BEAM_K * PW_BEAM_K * 2 : 0);
}

// EditNet's part of an exchange region, the same in this file's launches and in the ensemble's: [status line | h1 | attend_cap |
// c_new | h2 | projections | caption scores | visual scores] as flag-in-data words of 8 bytes (visual scores: 64 per row, R per
// row above 64 regions).  P.B / D / A / R must be set; returns the end.  pdec_edit_xbytes = its size.
char* pdec_edit_layout(PDecEditArgs& P, char* x) {
    const size_t B = P.B;
    P.status = (unsigned*)x; x += 128;
    P.x_h1 = x; x += B * P.D * 8;
    P.x_gt = x; x += B * P.D * 8;
    P.x_cn = x; x += B * P.D * 8;
    P.x_h2 = x; x += B * P.D * 8;
    P.x_a2 = x; x += B * 2 * P.A * 8;
    P.x_cs = x; x += B * PDEC_TMAX * 8;
    P.x_vs = x; x += B * pw_vcols(P.R) * 8;
    return x;
}
size_t pdec_edit_xbytes(int B, int D, int A, int R) {
    return 128 + 8 * ((size_t)B * D * 4 + (size_t)B * 2 * A + (size_t)B * PDEC_TMAX + (size_t)B * pw_vcols(R));
}

// ... | fc triples | the beam mode's candidate words]
size_t editnet_persistent_wide_xbytes(int B, int D, int A, int R) {
    if (B > PDW_MAXB) return 0;
    return pdec_edit_xbytes(B, D, A, R) + (size_t)B * (D / 4) * 32 + (B <= PW_BEAM_K ? (size_t)B * (D / 4) * PW_BEAM_W * 8 : 0);
}

// the weights in place, their leading dimensions, the dimensions and the vocabulary rows per workgroup of one EditNet launch
void pdec_edit_fill(PDecEditArgs& P, const SetEditNetWeights* w, const SetEditNetDims* d, int max_len) {
    const int D = d->D, F = d->F, G = D / 4;
    P.al_wih = w->al_wih; P.ld_ih = 3LL * D + F; P.al_whh = w->al_whh; P.cl_h2h_w = w->cl_h2h_w;
    P.cl_x2h_w = w->cl_x2h_w; P.ld_x2h = 2LL * D + F; P.cl_x2h_b = w->cl_x2h_b; P.cl_h2h_b = w->cl_h2h_b;
    P.ca_gate_w = w->ca_gate_w; P.ca_gate_b = w->ca_gate_b; P.ca_tc_w = w->ca_tc_w; P.ca_tc_b = w->ca_tc_b; P.ca_sc_b = w->ca_sc_b;
    P.ca_dec_w = w->ca_dec_w; P.ca_dec_b = w->ca_dec_b; P.ca_full_w = w->ca_full_w; P.ca_full_b = w->ca_full_b;
    P.va_dec_w = w->va_dec_w; P.va_dec_b = w->va_dec_b; P.va_full_w = w->va_full_w; P.va_full_b = w->va_full_b;
    P.cl_cnew_w = w->cl_cnew_w; P.cl_cnew_b = w->cl_cnew_b; P.cl_cmem_b = w->cl_cmem_b;
    P.fc_w = w->fc_w; P.fc_b = w->fc_b; P.tok_table = w->tok_table; P.ld_tab = 10LL * D;
    P.B = d->B; P.D = D; P.T = d->T; P.R = d->R; P.A = d->A; P.V = d->V; P.max_len = max_len; P.rpw = (d->V + G - 1) / G;
}

// wide_regions: the PDEC_RREG_WIDE instantiation (adaptive beam search), otherwise the PDEC_RREG one
bool editnet_persistent_wide_ok(int B, int D, int A, int T, int R, int V, bool wide_regions) {
    if (B < 1 || B > PDW_MAXB) return false;
    const int rreg = wide_regions ? PDEC_RREG_WIDE : PDEC_RREG;
    if (D != 64 * PDEC_KB || A != 512 || 2 * A != D || T > PDEC_TMAX || R > rreg || R > pw_vcols(rreg) || (R & 1) || (T & 1)) return false;
    const int G = D / 4;
    if ((V + G - 1) / G > 16 * PDEC_FC_TILES) return false;
    if (B * R > 4 * G || B * T > 4 * G) return false;               // one score of each kind per wave
    if (4 * G != 2 * A) return false;                                // the triples (B, G, 4) take the projections' place
    const int lds = pwide_lds_floats(B, D, A, false, rreg) * (int)sizeof(float);
    if (lds > 156 * 1024 || lds + 4096 > persistent_lds_limit()) return false;
    return true;
}

// the four instantiations: [0] beam over up to 128 masked regions, [1] beam, [2] greedy / teacher-forced, [3] Gumbel-max sampled.  (Listed in the order in
// which the kernels have always been instantiated: the device code object stays byte for byte the same.)
#define PWIDE_K(...) {reinterpret_cast<const void*>(&editnet_persistent_wide_k<__VA_ARGS__>)}
static PersistentKernel g_pwide_k[4] = {PWIDE_K(true, PDEC_RREG_WIDE), PWIDE_K(true, PDEC_RREG), PWIDE_K(false, PDEC_RREG),
                                        PWIDE_K(false, PDEC_RREG, true)};      // [3] Gumbel-max sampled (appended: see above)
#undef PWIDE_K

int editnet_persistent_wide_launch(PDecEditArgs& P, void* xbuf, PersistentGuard& guard, hipStream_t s, bool* unsupported, bool beam,
                                   bool wide_regions, bool sample) {
    *unsupported = true;
    const int B = P.B, D = P.D, A = P.A, G = D / 4;
    if (wide_regions && (!beam || !P.rmask)) return SET_OK;          // the wide instantiation is the adaptive beam search only
    if (sample && (beam || P.caps)) return SET_OK;                   // the sampled mode is the free-running loop's only
    if (!editnet_persistent_wide_ok(B, D, A, P.T, P.R, P.V, wide_regions)) return SET_OK;
    if (beam && (B > PW_BEAM_K || P.caps || (long long)B * P.V >= 0x7fffffffLL)) return SET_OK;
    {
        char* x = pdec_edit_layout(P, (char*)xbuf);
        P.x_fc = x; x += (size_t)B * G * 32;
        P.x_fcb = x;
    }
    const int rreg = wide_regions ? PDEC_RREG_WIDE : PDEC_RREG;
    const int lds = pwide_lds_floats(B, D, A, beam, rreg) * (int)sizeof(float);
    int lds_max = pwide_lds_floats(beam ? PW_BEAM_K : PDW_MAXB, D, A, beam, rreg) * (int)sizeof(float);
    if (lds_max > 156 * 1024) lds_max = 156 * 1024;
    if (lds > lds_max) return SET_OK;
    const double wbytes = 4.0 * ((double)P.V * D + 5.0 * 4 * D * D + 3.0 * D * D + 2.0 * A * D);
    const int rc = pdec_launch(g_pwide_k[sample ? 3 : wide_regions ? 0 : beam ? 1 : 2], guard, G, lds, lds_max, &P, xbuf, editnet_persistent_wide_xbytes(B, D, A, P.R),
                               s, {beam ? "persistent_beam" : sample ? "persistent_gumbel" : "persistent_decode", 2.0 * B * wbytes / 4.0 * P.max_len, wbytes * P.max_len},
                               {&P.stamps, &P.stamp_wg, 16, P.max_len});
    *unsupported = rc == SET_ERR_UNSUPPORTED;
    return *unsupported ? SET_OK : rc;
}


// ---------------------------------------------------------------------------------------------
// Host side of EditNet's persistent greedy / teacher-forced / beam decode: the argument block of one launch and the dispatch to
// the kernel above, which since round 5 serves every batch of 1 .. 16 rows (it measured faster than the <= 8-row kernel of round
// 4 at every row count — B = 4: 1.24 vs 1.28 ms, B = 8: 1.41 vs 1.67 ms — so that kernel was removed).
// ---------------------------------------------------------------------------------------------
// exchange region of one decode (laid out by decode_persistent_wide.hip)
size_t editnet_persistent_xbytes(int B, int D, int A, int R) { return B > PDW_MAXB ? 0 : editnet_persistent_wide_xbytes(B, D, A, R); }

bool editnet_persistent_ok(const SetEditNetDims* d, int max_len) {
    const int on = env_int("SET_DEC_PERSISTENT", 1);                 // (read per call: tests and A/B runs flip it inside one process)
    const int maxb = env_int("SET_DEC_PERSISTENT_MAXB", PDW_MAXB);
    if (!on || d->B > maxb || max_len < 1 || d->adaptive) return false;
    return editnet_persistent_wide_ok(d->B, d->D, d->A, d->T, d->R, d->V) && !persistent_disabled();
}

// set_editnet_beam_persistent: the k <= 4 hypotheses of one image as the rows of one launch.  Fixed features under the same
// conditions as the greedy launch; adaptive features (greedy and XE stay on the per-step kernels) on the instantiation with
// room for 128 masked regions
bool editnet_persistent_beam_ok(const SetEditNetDims* d) {
    if (d->B > PW_BEAM_K) return false;
    if (!d->adaptive) return editnet_persistent_ok(d, 1);
    if (!env_int("SET_DEC_PERSISTENT", 1) || d->B > env_int("SET_DEC_PERSISTENT_MAXB", PDW_MAXB) || persistent_disabled()) return false;
    return editnet_persistent_wide_ok(d->B, d->D, d->A, d->T, d->R, d->V, true);
}

// the greedy loop after the prologue (set_editnet_begin).  pv = X x2h[:, 2D:]^T (B, R, 4D), xbuf = exchange region.
// SET_ERR_UNSUPPORTED: nothing was touched, the caller runs the per-step loop.
int editnet_persistent_greedy(const SetEditNetWeights* w, const SetEditNetDims* d, const float* pre1, const float* att1,
                              const float* att1_c, const float* mask, const float* capP, const float* memQ, const float* Mem,
                              const float* pv, void* xbuf, long long* it, int* unfinished, int* alive, long long start_idx,
                              long long end_idx, int max_len, long long* seq, float* seq_logp, hipStream_t s,
                              const PDecTeacher* teach, const PDecBeam* beam, const PDecSample* samp) {
    const bool wide = beam && d->adaptive;              // adaptive beam search: region mask, up to 128 regions
    if (beam) {         // beam mode lives in the wide variant, whatever the row count
        if (!env_int("SET_DEC_PERSISTENT", 1) || max_len < 1 || (d->adaptive && !beam->rmask) || persistent_disabled() ||
            !editnet_persistent_wide_ok(d->B, d->D, d->A, d->T, d->R, d->V, wide)) return SET_ERR_UNSUPPORTED;
    } else if (!editnet_persistent_ok(d, max_len)) return SET_ERR_UNSUPPORTED;
    PDecEditArgs P{};
    pdec_edit_fill(P, w, d, max_len);
    P.pre1 = pre1; P.att1 = att1; P.att1_c = att1_c; P.mask = mask; P.capP = capP; P.memQ = memQ; P.Mem = Mem; P.pv = pv;
    P.it = it; P.unfinished = unfinished; P.alive = alive; P.seq = seq; P.seq_logp = seq_logp;
    P.start_idx = start_idx; P.end_idx = end_idx;
    if (teach) pdec_teacher_fill(P, *teach);
    if (beam) { pdec_beam_fill(P, *beam); if (wide) P.rmask = beam->rmask; }
    if (samp) { P.gm_seed = samp->seed; P.gm_offset = samp->offset; P.gm_inv_t = samp->inv_t; }
    PersistentGuard guard;
    if (guard.rc != SET_OK) return guard.rc;
    pdec_guard_fill(P, guard);
    bool unsupported = true;
    const int rc = editnet_persistent_wide_launch(P, xbuf, guard, s, &unsupported, beam != nullptr, wide, samp != nullptr);      // (lays out the exchange region)
    return rc != SET_OK ? rc : (unsupported ? SET_ERR_UNSUPPORTED : SET_OK);
}

}  // namespace set
