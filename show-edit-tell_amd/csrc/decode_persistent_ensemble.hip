// Persistent beam search of the EditNet + DCNet ENSEMBLE for one image (the reference's eval_full.py:132-202: both models step
// on the same words, their softmax probabilities are averaged and the beam is picked from log((softmax_e + softmax_d) / 2)):
// ONE launch of D / 4 workgroups for the whole search.  Two one-per-CU grids cannot be resident at once, so this kernel holds
// BOTH models' state: a workgroup owns four hidden units of EditNet's two cells and of DCNet's two cells, and the SAME
// vocabulary rows [v0, v1) of both fc layers — both models' logits of a slice meet in one workgroup and no logits travel.
// What is COPIED from editnet_persistent_wide_k<BEAM, 36> (decode_persistent_wide.hip) and from the general BEAM instantiation of
// dcnet_persistent_k (decode_persistent.hip) is the schedule of the phases: the weight requests (pd_load / pd_load_if) and the
// rotation of the three weight buffers, the exchanges (ll_put / ll_stage), the barriers, the stamps and the tags, in their
// order — moving those out of the loop bodies changes the kernels' instructions.  What is SHARED with those two kernels is the
// arithmetic between those lines, one definition each in decode_persistent.h: pd_sum4 / pd_sum4p (the four waves' partial sums),
// pd_fc_score, pd_clamp_tok, pd_cell (all four cells), and EditNet's pw_cap_softmax (with SelectC's first arg-max),
// pw_vis_softmax64, pw_cnew_gates, pw_copy_gate.  Still this kernel's own copies, because as leaves they moved an AGPR count of
// one of the three kernels (profiles/pdec_leaves_resources.json): the poll of the projections and the two attention scores
// (E3a), the context gate (E3b) and DCNet's masked row softmax (D3).  Shared further: the tail of the pick (slice top-k, candidate words, row merge,
// bookkeeping, poison: beam_persistent.h) and, on the host, the launch itself (PersistentKernel / pdec_launch,
// decode_persistent.h) and the fills and exchange layouts of both models' argument blocks (pdec_edit_fill / pdec_edit_layout,
// decode_persistent_wide.hip; pdec_dcnet_fill / pdec_dcnet_layout, pdec_beam_fill, decode_persistent.h).  The rows are the
// k <= PW_BEAM_K hypotheses, fixed features (R <= 36), both token tables active.
// Per pick:
//   S1    both attention_lstm cells from the products contracted ahead of the previous pick, read through the parent map
//                                                                                       -> h1 of EditNet X1e, h1 of DCNet X1d
//   E2-E6 EditNet's timestep (S2 .. S6 of decode_persistent_wide.hip: five more exchanges), its fc slice -> a register per lane;
//         S1' of EditNet (gate products of the next timestep that do not depend on the word)
//   D2-D5 DCNet's timestep (S2 .. S5 of decode_persistent.hip: two more exchanges; its h1 has been travelling since S1), its fc
//         slice -> a register per lane.  The two models share one weight-register set, one partial-tile region and one h1 buffer
//         in LDS: EditNet's activations are dead when DCNet's arrive
//   P1    per live row and model (max, sum exp) of the slice                            -> XL (B, G, 4); S1' of DCNet meanwhile
//         every workgroup combines the G pairs in the same order: lse_e[j], lse_d[j] are the same everywhere, no broadcast round
//   P2    per live row and word of the slice lp = logf((expf(le - lse_e) + expf(ld - lse_d)) * 0.5f) and score[j] + lp — the float
//         operations of beam_pick_k (beam.hip) in that form: the two routes differ only by the summation order inside the
//         normalisers — and the slice's 4 best (value, flat index j V + v) per row        -> XC (B, G, PW_BEAM_W)
//   P3    the merge and the bookkeeping of the two single-model launches (beam_persistent.h: value descending, flat index
//         ascending, parent = index / V), completed hypotheses leave, k shrinks, the (parent, word) history is written by workgroup 0
// A single round of per-slice candidates is not enough here: the order of the candidates INSIDE a slice depends on both
// models' global normalisers, hence P1 before P2.  Ten exchanges per pick, all flag-in-data words with vector stores
// (grid_barrier.h); every wait is wall-clock bounded by the same spin_limit / fault machinery (a time-out poisons best_score with
// NaN and sets result[2..3] = -1; the host answers SET_ERR_FAULT at its next call); the launch is serialised with the other
// persistent launches by PersistentGuard.
#include "beam_persistent.h"

namespace set {

struct PDecEnsArgs {
    PDecEditArgs e;                              // EditNet: weights, prologue products, its seven exchanges, dims, beam outputs, stamps
    struct {                                     // DCNet (the fields of decode_persistent.hip's argument block this launch reads)
        const float* al_wih_h2; long long ld_al;
        const float *al_whh, *ll_whh, *ll_wih; long long ld_ll;
        const float *ll_bih, *ll_bhh;
        const float *ca_dec_w, *ca_dec_b, *ca_full_w, *ca_full_b;
        const float *fc_w, *fc_b;
        const float* tok_table; long long ld_tab;
        const float *pre1, *att1_c, *mask, *pc;
        void *x_h1, *x_h2, *x_att2;              // (B, D), (B, D), (B, A)
    } d;
    void* x_lse;                                 // (B, G, 4) per-slice (max_e, sum exp_e, max_d, sum exp_d)
    void* x_cand;                                // (B, G, PW_BEAM_W) per-slice candidates of the joint pick
};

namespace {

constexpr int PE_U = 16;               // 16-byte requests a lane keeps in flight while it fills LDS from an exchange buffer
constexpr int PE_K = PW_BEAM_K;

#define PE_STAMP(i) if (P.e.stamps && t < PD_STAMP_STEPS && (int)blockIdx.x == P.e.stamp_wg && threadIdx.x == 0) P.e.stamps[t * PD_STAMPS + (i)] = __builtin_amdgcn_s_memrealtime()

}  // namespace

__global__ void __launch_bounds__(PDEC_THREADS, 1) ensemble_persistent_k(const PDecEnsArgs P) {
    constexpr int RS = pdec_rs(PDEC_RREG);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ long long sTok[PE_K];
    __shared__ int sJs[PE_K];
    __shared__ float sWj[PE_K];
    __shared__ int sPar[PE_K];                           // parent slot of every slot (identity before the first pick)
    __shared__ float sScore[PE_K];                       // running scores of the slots (-inf = dead)
    __shared__ int sKleft;
    __shared__ float sBest;                              // best completed hypothesis so far
    const int tid = threadIdx.x, lane = tid & 63, kq = tid >> 6, r = lane & 15, g = lane >> 4;
    const int B = P.e.B, D = P.e.D, T = P.e.T, R = P.e.R, A = P.e.A, V = P.e.V;
    const int KQ = D >> 2, LDH = D + 4;
    const int wg = (int)blockIdx.x, u0 = wg * 4, G = (int)gridDim.x;
    // ---- LDS.  Shared by the two models: sX, sRed (EditNet's timestep is over when DCNet's h1 is staged)
    float* sX = smem;                                    // (B, LDH) EditNet: h1 -> attend_cap -> c_new -> h2; then DCNet's h1
    float* sH2 = sX + B * LDH;                           // (B, LDH) DCNet's h2; then the pick's (B, G, 4) normaliser words
    float* sRed = sH2 + B * LDH;                         // [4 waves][3 tiles][16][16]
    float* sAlc = sRed + 4 * 3 * 256;                    // EditNet (K, TMAX) caption scores -> weights
    float* sAlv = sAlc + PE_K * PDEC_TMAX;               // (K, 64) visual scores -> weights
    float* sG = sAlv + PE_K * 64;                        // (K, 16) copy_lstm gate pre-activations
    float* sZ = sG + PE_K * 16;                          // (K, 8)
    float* sM = sZ + PE_K * 8;                           // (K, 8)
    float* sPv = sM + PE_K * 8;                          // (B, 16, RREG) hoisted region products of the owned gate rows
    float* sPz = sPv + B * 16 * RS;                      // (B, 8, TMAX) hoisted caption-context products of the owned columns
    float* sCon = sPz + B * 8 * PDEC_TS;                   // [cap_decoder_att.b | cap_full_att.w | decoder_att.b | full_att.w] (4, A)
    float* sRedP = sCon + 4 * A;                         // [4 waves][16][16] copy_lstm.h2h h2 of the previous timestep
    float* sCst = sRedP + 4 * 256;                       // (2, K, 4) c1 | c2 of the owned units
    float* dAl = sCst + 2 * PE_K * 4;                    // DCNet (K, TMAX) attention weights
    float* dG = dAl + PE_K * PDEC_TMAX;                  // (K, 16) gate pre-activations of language_lstm
    float* dA2 = dG + PE_K * 16;                         // (B, A) cap_decoder_att(h1)
    float* dCon = dA2 + B * A;                           // [cap_decoder_att.bias | cap_full_att.weight] (2, A)
    float* dPc = dCon + 2 * A;                           // (B, 16, TMAX) hoisted context products of the owned gate rows
    float* dRedP = dPc + B * 16 * PDEC_TS;                 // [4 waves][16][16] language_lstm.W_hh h2 of the previous timestep
    float* dCst = dRedP + 4 * 256;                       // (2, K, 4)
    float* sFB = dCst + 2 * PE_K * 4;                    // (B, G, PW_BEAM_W) every slice's candidates
    float* sCand = sFB + B * G * PW_BEAM_W;              // (K, K, 2) (score, flat index) of every row's best K candidates
    float* sLse = sH2;
    const LLWatch watch{P.e.status, P.e.fault, P.e.spin_limit};

#define PE_SYNC() __syncthreads()
#define PE_STAGE(RSRC, DST, ROWS, COLS, LD, TAG) ll_stage<PDEC_THREADS, PE_U>(RSRC, DST, ROWS, COLS, LD, TAG, watch, tid)

    // ---- weight tiles of this lane: gate row of output column r = gate (r >> 2) of unit u0 + (r & 3)
    const long long grow = (long long)(r >> 2) * D + u0 + (r & 3);
    const int kcol = kq * KQ + 4 * g;
    // EditNet
    const float* pT0 = P.e.al_wih + grow * P.e.ld_ih + 2 * D + kcol;
    const float* pT1 = P.e.al_whh + grow * D + kcol;
    const float* pT2 = P.e.cl_h2h_w + grow * D + kcol;
    const float* pT3 = P.e.cl_x2h_w + grow * P.e.ld_x2h + kcol;
    const float* pT5 = P.e.cl_x2h_w + grow * P.e.ld_x2h + D + kcol;
    const float* pT4;                                    // mixed tile: rows 0-3 context_gate, 4-7 tc_affine, 8-11 attention projections
    {
        const int j = wg * 4 + (r & 3);                  // row of the stacked [cap_decoder_att ; decoder_att] (2A rows)
        pT4 = r < 4 ? P.e.ca_gate_w + (long long)(u0 + r) * 3 * D + D + kcol
            : r < 8 ? P.e.ca_tc_w + (long long)(u0 + r - 4) * 2 * D + D + kcol
                    : (j < A ? P.e.ca_dec_w + (long long)j * D : P.e.va_dec_w + (long long)(j - A) * D) + kcol;
    }
    const bool v4 = r < 12;
    const bool v6 = r < 4;
    const float* pT6 = P.e.cl_cnew_w + (long long)(u0 + (r & 3)) * D + kcol;
    // DCNet
    const float* qT0 = P.d.al_wih_h2 + grow * P.d.ld_al + kcol;
    const float* qT1 = P.d.al_whh + grow * D + kcol;
    const float* qT2 = P.d.ll_whh + grow * D + kcol;
    const float* qT3 = P.d.ll_wih + grow * P.d.ld_ll + kcol;
    const int apw = A / G;                               // host: A % G == 0, apw <= 16
    const bool vD = r < apw;
    const float* qT4 = P.d.ca_dec_w + (long long)(vD ? wg * apw + r : 0) * D + kcol;
    // fc: the same vocabulary rows of both models
    const int row0 = wg * P.e.rpw;
    const float *pF[PDEC_FC_TILES], *qF[PDEC_FC_TILES];
    bool vF[PDEC_FC_TILES];
#pragma unroll
    for (int j = 0; j < PDEC_FC_TILES; ++j) {
        const int row = row0 + 16 * j + r;
        vF[j] = (16 * j + r < P.e.rpw) && row < V;
        pF[j] = P.e.fc_w + (long long)(vF[j] ? row : 0) * D + kcol;
        qF[j] = P.d.fc_w + (long long)(vF[j] ? row : 0) * D + kcol;
    }
    const bool fc_ok = lane < 16 * PDEC_FC_TILES && lane < P.e.rpw && row0 + lane < V;   // lane l scores vocabulary row row0 + l
    const float fcb_e = fc_ok ? P.e.fc_b[row0 + lane] : 0.f;
    const float fcb_d = fc_ok ? P.d.fc_b[row0 + lane] : 0.f;
    const int arow = (r < B ? r : B - 1) * LDH;          // rows >= B repeat the last one: their outputs are never read
    const float* aX = sX + arow + kcol;
    const float* aH2 = sH2 + arow + kcol;

    // ---- thread roles (the same in both models) and their loop-invariant operands
    const bool pair = tid < B * 4;                       // (row, owned unit): the four cells, the context gate, the copy gate
    const int pb = tid >> 2, pu = tid & 3, pd = u0 + pu;
    const bool gcol = tid < B * 16;                      // (row, gate row) of the hoisted region / context products
    const int cb = tid >> 4, crr = tid & 15;
    const long long ccol = (long long)(crr >> 2) * D + u0 + (crr & 3);
    const bool zrole = tid < B * 8;                      // (row, [z | s] column) of EditNet's hoisted caption-context products
    const int zb = tid >> 3, zc8 = tid & 7;
    float c1 = 0.f, c2 = 0.f, pre[4] = {0.f, 0.f, 0.f, 0.f};
    float dc1 = 0.f, dc2 = 0.f, dpre[4] = {0.f, 0.f, 0.f, 0.f};
    float bg = 0.f, bsc = 0.f, btc = 0.f, bcn = 0.f, bcm = 0.f, b2 = 0.f, db2 = 0.f;
    if (pair) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            pre[q] = P.e.pre1[(long long)pb * 4 * D + (long long)q * D + pd];
            dpre[q] = P.d.pre1[(long long)pb * 4 * D + (long long)q * D + pd];
        }
        bg = P.e.ca_gate_b[pd]; bsc = P.e.ca_sc_b[pd]; btc = P.e.ca_tc_b[pd]; bcn = P.e.cl_cnew_b[pd]; bcm = P.e.cl_cmem_b[pd];
    }
    if (gcol) {
        for (int rr = 0; rr < PDEC_RREG; ++rr) sPv[tid * RS + rr] = rr < R ? P.e.pv[((long long)cb * R + rr) * 4 * D + ccol] : 0.f;
        for (int tt = 0; tt < PDEC_TMAX; ++tt) dPc[tid * PDEC_TS + tt] = tt < T ? P.d.pc[((long long)cb * T + tt) * 4 * D + ccol] : 0.f;
        b2 = P.e.cl_x2h_b[ccol] + P.e.cl_h2h_b[ccol];
        db2 = P.d.ll_bih[ccol] + P.d.ll_bhh[ccol];
    }
    if (zrole)
        for (int tt = 0; tt < PDEC_TMAX; ++tt)
            sPz[tid * PDEC_TS + tt] = tt < T ? P.e.capP[((long long)zb * T + tt) * 2 * D + (zc8 < 4 ? u0 + zc8 : D + u0 + zc8 - 4)] : 0.f;
    for (int i = tid; i < A; i += PDEC_THREADS) {
        sCon[i] = P.e.ca_dec_b[i]; sCon[A + i] = P.e.ca_full_w[i]; sCon[2 * A + i] = P.e.va_dec_b[i]; sCon[3 * A + i] = P.e.va_full_w[i];
        dCon[i] = P.d.ca_dec_b[i]; dCon[A + i] = P.d.ca_full_w[i];
    }
    const int a_lo = lane * 4, a_hi = lane * 4 + 256;
    const float cbf = P.e.ca_full_b[0], vbf = P.e.va_full_b[0], dbf = P.d.ca_full_b[0];
    // EditNet: the ONE caption score and the ONE visual score this wave owns (index s = wg + G * wave over (b, t) / (b, r)); the
    // cap_features_att / features_att rows they need are loop-invariant and stay in registers
    const int s_idx = wg + G * kq;
    const bool cs_on = s_idx < B * T, vs_on = s_idx < B * R;
    const int cs_b = cs_on ? s_idx / T : 0, cs_t = cs_on ? s_idx % T : 0;
    const int vs_b = vs_on ? s_idx / R : 0, vs_r = vs_on ? s_idx % R : 0;
    const f32x4 ca1_0 = *reinterpret_cast<const f32x4*>(P.e.att1_c + ((long long)cs_b * T + cs_t) * A + a_lo);
    const f32x4 ca1_1 = *reinterpret_cast<const f32x4*>(P.e.att1_c + ((long long)cs_b * T + cs_t) * A + a_hi);
    const float cs_mask = P.e.mask[(long long)cs_b * T + cs_t];
    const f32x4 va1_0 = *reinterpret_cast<const f32x4*>(P.e.att1 + ((long long)vs_b * R + vs_r) * A + a_lo);
    const f32x4 va1_1 = *reinterpret_cast<const f32x4*>(P.e.att1 + ((long long)vs_b * R + vs_r) * A + a_hi);
    // exchange buffers (grid_barrier.h, flag-in-data words)
    const __amdgpu_buffer_rsrc_t h1rs = __builtin_amdgcn_make_buffer_rsrc(P.e.x_h1, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t a2rs = __builtin_amdgcn_make_buffer_rsrc(P.e.x_a2, 0, B * 2 * A * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t gtrs = __builtin_amdgcn_make_buffer_rsrc(P.e.x_gt, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t csrs = __builtin_amdgcn_make_buffer_rsrc(P.e.x_cs, 0, B * PDEC_TMAX * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t vsrs = __builtin_amdgcn_make_buffer_rsrc(P.e.x_vs, 0, B * 64 * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t cnrs = __builtin_amdgcn_make_buffer_rsrc(P.e.x_cn, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t h2rs = __builtin_amdgcn_make_buffer_rsrc(P.e.x_h2, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t dh1rs = __builtin_amdgcn_make_buffer_rsrc(P.d.x_h1, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t dh2rs = __builtin_amdgcn_make_buffer_rsrc(P.d.x_h2, 0, B * D * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t da2rs = __builtin_amdgcn_make_buffer_rsrc(P.d.x_att2, 0, B * A * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t lsrs = __builtin_amdgcn_make_buffer_rsrc(P.x_lse, 0, B * G * 4 * 8, 0x00027000);
    const __amdgpu_buffer_rsrc_t fbrs = __builtin_amdgcn_make_buffer_rsrc(P.x_cand, 0, B * G * PW_BEAM_W * 8, 0x00027000);

    // ---- initial state: zeros in all four cells; every row is fed <start>; pick 1 counts row 0 only (all rows are identical)
    if (tid < PE_K) { sTok[tid] = P.e.start_idx; sPar[tid] = tid; sScore[tid] = tid == 0 ? 0.f : -INFINITY; }
    for (int i = tid; i < 4 * 256; i += PDEC_THREADS) { sRedP[i] = 0.f; dRedP[i] = 0.f; }   // h2h h2 / W_hh h2 of the zero state
    if (tid == 0) {
        sKleft = B; sBest = -INFINITY;
        if (wg == 0) { P.e.bm_best_score[0] = -INFINITY; P.e.bm_best_word[0] = 0; P.e.bm_result[0] = -1; P.e.bm_result[1] = -1; P.e.bm_result[2] = B; P.e.bm_result[3] = 0; }
    }
    __syncthreads();

    // weight tiles rotate through three register buffers, EditNet's schedule (decode_persistent_wide.hip) followed by DCNet's
    // (decode_persistent.hip, on wa / wb)
    f32x4 wa[PDEC_KB], wb[PDEC_KB], wc[PDEC_KB];
    unsigned tag = 0;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // gate products of the NEXT timestep that do not depend on the word.  EditNet: acc1n = W_hh h1 (E2), acc1 = acc1n +
    // W_ih[:, h2] h2 (S1'e).  DCNet: dacc1 = W_ih[:, h2] h2 + W_hh h1 (S1'd).  t = 0: h1 = h2 = 0.
    f32x4 acc1 = zero4, acc1n = zero4, dacc1 = zero4;
    for (int t = 0; t < P.e.max_len; ++t) {
        // ================= S1: both attention_lstm cells
        PE_STAMP(0);
        float tg[4] = {0.f, 0.f, 0.f, 0.f}, ttc = 0.f, tcg = 0.f, dtg[4] = {0.f, 0.f, 0.f, 0.f};
        if (pair) {
            long long tok = sTok[pb];
            tok = pd_clamp_tok(tok, V);
            const float* trow = P.e.tok_table + tok * P.e.ld_tab + pd;
            const float* drow = P.d.tok_table + tok * P.d.ld_tab + pd;
#pragma unroll
            for (int q = 0; q < 4; ++q) { tg[q] = trow[(long long)q * D]; dtg[q] = drow[(long long)q * D]; }
            ttc = trow[4LL * D];
            tcg = trow[5LL * D];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = acc1[e];
            sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = dacc1[e];
        }
        if (pair) {
            sCst[pb * 4 + pu] = c1; sCst[PE_K * 4 + pb * 4 + pu] = c2;
            dCst[pb * 4 + pu] = dc1; dCst[PE_K * 4 + pb * 4 + pu] = dc2;
        }
        PE_SYNC();
        // slot pb continues hypothesis sPar[pb] of the previous timestep — the cell states of both models and the gate
        // products that were contracted before the pick are read through the ONE parent map
        const int par = sPar[pair ? pb : 0];
        if (pair) {
            c1 = sCst[par * 4 + pu]; c2 = sCst[PE_K * 4 + par * 4 + pu];
            dc1 = dCst[par * 4 + pu]; dc2 = dCst[PE_K * 4 + par * 4 + pu];
        }
        ++tag;                                                   // X1e, X1d: h1 of both models
        const unsigned tag_h1 = tag;
        if (pair && !(P.e.test_stall && wg == 0)) {
            float gq[4], dq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = par * 16 + q * 4 + pu;
                gq[q] = (pd_sum4(sRed, 0, o) + pre[q]) + tg[q];
                dq[q] = (pd_sum4(sRed, 1, o) + dpre[q]) + dtg[q];
            }
            ll_put(h1rs, pb * D + pd, pd_cell(gq[0], gq[1], gq[2], gq[3], c1), tag);
            ll_put(dh1rs, pb * D + pd, pd_cell(dq[0], dq[1], dq[2], dq[3], dc1), tag);
        }
        pd_load(wb, pT3);
        pd_load_if(wa, pT4, v4);
        pd_load(wc, pT1);
        PE_STAMP(1);
        PE_STAGE(h1rs, sX, B, D, LDH, tag);
        PE_SYNC();
        // ================= E2: copy_lstm.x2h[:, :D] h1; context_gate / tc_affine rows of the owned columns, 4 projection rows;
        // attention_lstm.W_hh h1 for the next timestep
        PE_STAMP(2);
        f32x4 acc2 = zero4;
        {
            pd_mma(acc2, wb, aX);
            f32x4 accm = zero4;
            pd_mma(accm, wa, aX);
            acc1n = zero4;
            pd_mma(acc1n, wc, aX);
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = accm[e];
        }
        PE_SYNC();
        ++tag;                                                   // X2e: [cap_decoder_att(h1) | decoder_att(h1)]
        if (gcol && crr < 12) {
            const int o = cb * 16 + crr;
            const float v = pd_sum4(sRed, 1, o);
            if (crr < 8) sM[cb * 8 + crr] = v;
            else ll_put(a2rs, cb * 2 * A + wg * 4 + crr - 8, v, tag);
        }
        // ================= E3a: this wave's caption score and visual score; the two projection rows it needs are polled straight
        // into registers
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
        pd_load(wb, pT5);                                        // E4's tile: one tile ahead of the (small) score exchange
        PE_STAMP(3);
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
        }
        ++tag;                                                   // X3a: caption scores + visual scores
        if (cs_on && lane == 0) ll_put(csrs, cs_b * T + cs_t, cs_val, tag);
        if (vs_on && lane == 0) ll_put(vsrs, vs_b * R + vs_r, vs_val, tag);
        PE_STAMP(4);
        PE_STAGE(csrs, sAlc, B, T, PDEC_TMAX, tag);              // (T and R are even: editnet_persistent_wide_ok)
        PE_STAGE(vsrs, sAlv, B, R, 64, tag);
        pd_load_if(wa, pT6, v6);                                 // E5's (short) tile and fc's first one stream under the softmaxes
        pd_load_if(wc, pF[0], vF[0]);                            // and the attend_cap exchange
        PE_SYNC();
        PE_STAMP(5);
        // ================= E3b: both softmaxes of every row, SelectC's arg-max (editnet.py:375-376, :409-416, :446)
        if (kq < B) {
            const int b = kq;
            pw_cap_softmax(sAlc + b * PDEC_TMAX, T, lane, &sJs[b], &sWj[b]);
            pw_vis_softmax64(sAlv + b * 64, R, lane);
        }
        PE_SYNC();
        if (zrole) {
            float s = 0.f;
            for (int tt = 0; tt < T; ++tt) s += sAlc[zb * PDEC_TMAX + tt] * sPz[tid * PDEC_TS + tt];
            sZ[zb * 8 + zc8] = s;
        }
        PE_SYNC();
        PE_STAMP(6);
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
            selv = P.e.Mem[((long long)pb * T + js) * D + pd] * wj;
            cmemv = P.e.memQ[((long long)pb * T + js) * D + pd] * wj;
        }
        PE_STAGE(gtrs, sX, B, D, LDH, tag);
        PE_SYNC();
        PE_STAMP(7);
        // ================= E4: copy_lstm.x2h[:, D:2D] attend_cap; hoisted region products -> c_new
        {
            pd_mma(acc2, wb, aX);
            pd_load_if(wb, pF[1], vF[1]);
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 2) * 256 + (4 * g + e) * 16 + r] = acc2[e];
        }
        PE_SYNC();
        if (gcol) {
            const int o = cb * 16 + crr;
            float s = 0.f;
            for (int rr = 0; rr < R; ++rr) s += sAlv[cb * 64 + rr] * sPv[tid * RS + rr];
            float g2 = pd_sum4(sRed, 2, o);
            g2 += pd_sum4p(sRedP, sPar[cb] * 16 + crr);          // + copy_lstm.h2h h2 of the PARENT hypothesis (S1'e of the previous timestep)
            sG[o] = (g2 + s) + b2;
        }
        PE_SYNC();
        ++tag;                                                   // X4e: c_new
        float cnv = 0.f, ogv = 0.f;
        if (pair) {
            pw_cnew_gates(sG + pb * 16 + pu, c2, cnv, ogv);
            ll_put(cnrs, pb * D + pd, cnv, tag);
        }
        PE_STAGE(cnrs, sX, B, D, LDH, tag);
        PE_SYNC();
        PE_STAMP(8);
        // ================= E5: gate_cnew rows of the owned units, copy gate (editnet.py:281-283) -> c2, h2
        {
            f32x4 acc5 = zero4;
            pd_mma(acc5, wa, aX);
            pd_load_if(wa, pF[2], vF[2]);
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = acc5[e];
        }
        PE_SYNC();
        ++tag;                                                   // X5e: h2
        if (pair) {
            const float a = pd_sum4(sRed, 0, pb * 16 + pu) + bcn;
            ll_put(h2rs, pb * D + pd, pw_copy_gate(a, cmemv, bcm, selv, cnv, ogv, c2), tag);
        }
        PE_STAGE(h2rs, sX, B, D, LDH, tag);
        PE_SYNC();
        PE_STAMP(9);
        // ================= E6: EditNet's fc over this workgroup's vocabulary rows
        const bool more = t + 1 < P.e.max_len;
        {
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
        PE_SYNC();
        // wave b keeps EditNet's scores of row b: lane l holds vocabulary row row0 + l of the slice
        float xe = -INFINITY;
        if (kq < B && fc_ok) xe = pd_fc_score(sRed, kq, lane, fcb_e);
        // S1'e: attention_lstm.W_ih[:, h2] h2 (+ W_hh h1 from E2) and copy_lstm.h2h h2 for timestep t + 1; the latter goes to LDS:
        // the next timestep adds it through the parent map
        if (more) {
            acc1 = acc1n;
            pd_mma(acc1, wc, aX);
            f32x4 accp = zero4;
            pd_mma(accp, wb, aX);
#pragma unroll
            for (int e = 0; e < 4; ++e) sRedP[kq * 256 + (4 * g + e) * 16 + r] = accp[e];
        }
        pd_load(wb, qT3);                                        // DCNet's first two tiles
        pd_load_if(wa, qT4, vD);
        PE_SYNC();                                               // (EditNet's h2 and its fc tiles have been read: sX and sRed are DCNet's)
        PE_STAMP(10);
        // ================= D2: DCNet.  h1 has been travelling since S1
        PE_STAGE(dh1rs, sX, B, D, LDH, tag_h1);
        PE_SYNC();
        PE_STAMP(11);
        // language_lstm W_ih[:, :D] h1, this workgroup's rows of cap_decoder_att(h1)
        {
            f32x4 dacc2 = zero4, accd = zero4;
            pd_mma(dacc2, wb, aX);
            pd_mma(accd, wa, aX);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = accd[e];
                sRed[(kq * 3 + 2) * 256 + (4 * g + e) * 16 + r] = dacc2[e];
            }
        }
        PE_SYNC();
        ++tag;                                                   // X2d: cap_decoder_att(h1) (without its bias)
        float dg2 = 0.f;
        if (gcol) {
            const int o = cb * 16 + crr;
            if (crr < apw) {
                ll_put(da2rs, cb * A + wg * apw + crr, pd_sum4(sRed, 1, o), tag);
            }
            dg2 = pd_sum4(sRed, 2, o);
            dg2 += pd_sum4p(dRedP, sPar[cb] * 16 + crr);         // + language_lstm.W_hh h2 of the PARENT hypothesis (S1'd of the previous timestep)
        }
        PE_STAGE(da2rs, dA2, B, A, A, tag);
        PE_SYNC();
        PE_STAMP(12);
        pd_load_if(wa, qF[0], vF[0]);                            // fc's first tile streams under the attention's arithmetic ...
        // ================= D3: caption attention of every row, in every workgroup (dcnet.py:261-268); wave b scores row b
        if (kq < B) {
            const int b = kq;
            f32x4 a2[2], wf[2];
            a2[0] = *reinterpret_cast<const f32x4*>(dA2 + b * A + a_lo);
            a2[1] = *reinterpret_cast<const f32x4*>(dA2 + b * A + a_hi);
            const float mk = lane < T ? P.d.mask[(long long)b * T + lane] : 1.f;
            a2[0] += *reinterpret_cast<const f32x4*>(dCon + a_lo); a2[1] += *reinterpret_cast<const f32x4*>(dCon + a_hi);
            wf[0] = *reinterpret_cast<const f32x4*>(dCon + A + a_lo); wf[1] = *reinterpret_cast<const f32x4*>(dCon + A + a_hi);
            constexpr int RB = 10;
            float mine = 0.f;                                   // lane tt keeps the score of position tt
            const unsigned long long live = __ballot(lane < T && mk != 0.f);
            const float* a1 = P.d.att1_c + (long long)b * T * A;
            for (int t0 = 0; t0 < T; t0 += RB) {
                f32x4 v[RB][2];
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    const int tt = t0 + u < T ? t0 + u : T - 1;
                    v[u][0] = *reinterpret_cast<const f32x4*>(a1 + (long long)tt * A + a_lo);
                    v[u][1] = *reinterpret_cast<const f32x4*>(a1 + (long long)tt * A + a_hi);
                }
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    const int tt = t0 + u;
                    if (!((live >> tt) & 1ull)) continue;       // masked position (or past T): its score is -1e10 whatever it is
                    const float sc = pw_wsum(pd_score8(v[u][0] + a2[0], v[u][1] + a2[1], wf[0], wf[1]));
                    if (lane == tt) mine = sc;
                }
            }
            // masked softmax over the T <= 32 scores inside the wave (one score per lane)
            const float sc = lane < T ? ((mk == 0.f) ? -1e10f : (mine + dbf)) : -INFINITY;
            const float m = pw_wmax(sc);
            const float ex = lane < T ? expf(sc - m) : 0.f;
            const float sum = pw_wsum(ex);
            if (lane < T) dAl[b * PDEC_TMAX + lane] = ex / sum;
        }
        pd_load_if(wb, qF[1], vF[1]);                            // ... the second under the cell update and the h2 exchange
        PE_SYNC();
        PE_STAMP(13);
        if (gcol) {
            float s = 0.f;
            for (int tt = 0; tt < T; ++tt) s += dAl[cb * PDEC_TMAX + tt] * dPc[tid * PDEC_TS + tt];
            dG[cb * 16 + crr] = (dg2 + s) + db2;
        }
        PE_SYNC();
        ++tag;                                                   // X3d: h2
        if (pair) {
            const float* gp = dG + pb * 16 + pu;
            ll_put(dh2rs, pb * D + pd, pd_cell(gp[0], gp[4], gp[8], gp[12], dc2), tag);
        }
        PE_STAGE(dh2rs, sH2, B, D, LDH, tag);
        PE_SYNC();
        PE_STAMP(14);
        // ================= D5: DCNet's fc over the same vocabulary rows
        {
            f32x4 accf0 = zero4, accf1 = zero4, accf2 = zero4;
            pd_mma(accf0, wa, aH2);
            pd_load_if(wa, qF[2], vF[2]);
            pd_mma(accf1, wb, aH2);
            if (more) pd_load(wb, qT0);
            pd_mma(accf2, wa, aH2);
            if (more) pd_load(wa, qT1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sRed[(kq * 3 + 0) * 256 + (4 * g + e) * 16 + r] = accf0[e];
                sRed[(kq * 3 + 1) * 256 + (4 * g + e) * 16 + r] = accf1[e];
                sRed[(kq * 3 + 2) * 256 + (4 * g + e) * 16 + r] = accf2[e];
            }
        }
        PE_SYNC();
        PE_STAMP(15);
        // ================= P1: per row and model, (max, sum exp) of the slice (eval_full.py:150-153: two softmaxes over V)
        ++tag;
        float xd = -INFINITY;
        if (kq < B) {
            const int b = kq;
            if (fc_ok) xd = pd_fc_score(sRed, b, lane, fcb_d);
            const float me = pw_wmax(xe), md = pw_wmax(xd);
            const float se = pw_wsum((fc_ok && me > -INFINITY) ? expf(xe - me) : 0.f);
            const float sd = pw_wsum((fc_ok && md > -INFINITY) ? expf(xd - md) : 0.f);
            if (lane < 4) ll_put(lsrs, (b * G + wg) * 4 + lane, lane == 0 ? me : (lane == 1 ? se : (lane == 2 ? md : sd)), tag);
        }
        // S1'd: [W_ih[:, h2] | W_hh] of attention_lstm and language_lstm.W_hh for timestep t + 1, while the normaliser words
        // travel: nothing here waits for the word.  language_lstm.W_hh h2 goes to LDS: added through the parent map
        if (more) {
            dacc1 = zero4;
            pd_mma(dacc1, wb, aH2);
            pd_load(wb, qT2);
            pd_mma(dacc1, wa, aX);
            f32x4 accp = zero4;
            pd_mma(accp, wb, aH2);
#pragma unroll
            for (int e = 0; e < 4; ++e) dRedP[kq * 256 + (4 * g + e) * 16 + r] = accp[e];
        }
        PE_SYNC();                                               // (h2's last readers are done: its buffer takes the normaliser words)
        PE_STAMP(16);
        PE_STAGE(lsrs, sLse, B * G, 4, 4, tag);
        PE_SYNC();
        PE_STAMP(17);
        // ================= P2: every workgroup combines the G pairs of both models (the same lse everywhere), then scores its own
        // slice: log of the averaged probabilities + the running score, the slice's B best per row
        ++tag;
        if (kq < B) {
            const int j = kq;
            const float scj = sScore[j];
            pb_vals cvv;
            pb_idxs cii;
            pb_none(cvv, cii);
            if (scj > -INFINITY) {                               // (uniform in the wave; dead slots publish empty lists)
                float pme[4], pse[4], pmd[4], psd[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* e = sLse + (j * G + lane + 64 * i) * 4;
                    pme[i] = e[0]; pse[i] = e[1]; pmd[i] = e[2]; psd[i] = e[3];
                }
                const float me = pw_wmax(fmaxf(fmaxf(pme[0], pme[1]), fmaxf(pme[2], pme[3])));
                const float md = pw_wmax(fmaxf(fmaxf(pmd[0], pmd[1]), fmaxf(pmd[2], pmd[3])));
                float sse = 0.f, ssd = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sse += (pme[i] == -INFINITY) ? 0.f : pse[i] * expf(pme[i] - me);
                    ssd += (pmd[i] == -INFINITY) ? 0.f : psd[i] * expf(pmd[i] - md);
                }
                sse = pw_wsum(sse); ssd = pw_wsum(ssd);
                const float lse_e = me + logf(sse), lse_d = md + logf(ssd);
                float xx = -INFINITY;
                if (fc_ok) {
                    const float lp = logf((expf(xe - lse_e) + expf(xd - lse_d)) * 0.5f);   // as beam_pick_k forms it
                    xx = scj + lp;
                }
                pb_slice_topk(xx, j * V + row0 + lane, fc_ok, B, cvv, cii);
            }
            pb_publish(fbrs, (j * G + wg) * PW_BEAM_W, lane, 0.f, 0.f, cvv, cii, tag);   // (the normalisers travelled in P1)
        }
        PE_STAMP(18);
        PE_STAGE(fbrs, sFB, B * G, PW_BEAM_W, PW_BEAM_W, tag);
        PE_SYNC();
        PE_STAMP(19);
        // ================= P3: every workgroup runs the same merge.  Wave j: the B best of row j's G x 4 candidates (four slices
        // per lane)
        if (kq < B) {
            const int j = kq;
            pb_vals ov;
            pb_idxs oi;
            pb_none(ov, oi);
            if (sScore[j] > -INFINITY) {
                float cv[16];
                int ci[16];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* e = sFB + ((j * G + lane + 64 * i) * PW_BEAM_W);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        ci[4 * i + q] = __float_as_int(e[3 + 2 * q]);
                        cv[4 * i + q] = ci[4 * i + q] != 0x7fffffff ? e[2 + 2 * q] : -INFINITY;
                    }
                }
                pb_row_merge(cv, ci, B, ov, oi);
            }
            if (lane == 0) pb_row_store(sCand, j, ov, oi);
        }
        PE_SYNC();
        if (tid == 0)                                            // the pick itself and its bookkeeping (beam_persistent.h)
            pb_pick(sCand, sScore, sTok, sPar, &sKleft, &sBest, P.e.bm_hist_par, P.e.bm_hist_word, P.e.bm_best_score, P.e.bm_best_word,
                    P.e.bm_result, V, P.e.end_idx, t, B, wg == 0, P.e.bm_hist_score);
        PE_SYNC();
        PE_STAMP(20);
        if (sKleft == 0) break;                                  // every hypothesis has ended (eval_full.py:197-198)
    }
#undef PE_STAGE
#undef PE_SYNC
    // ---- an exchange of this launch timed out: never hand the result out as a search (see encoder_persistent.hip)
    __shared__ unsigned s_bad;
    if (tid == 0) s_bad = __hip_atomic_load(P.e.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_bad && wg == 0 && tid == 0) pb_poison(P.e.bm_best_score, P.e.bm_result);
}

namespace {

int pens_lds_floats(int B, int D, int A) {
    const int G = D / 4;
    const int shared = 2 * B * (D + 4) + 4 * 3 * 256;
    const int edit = PE_K * (PDEC_TMAX + 64 + 16 + 8 + 8) + B * 16 * pdec_rs(PDEC_RREG) + B * 8 * PDEC_TS + 4 * A + 4 * 256 + 2 * PE_K * 4;
    const int dcn = PE_K * (PDEC_TMAX + 16) + B * A + 2 * A + B * 16 * PDEC_TS + 4 * 256 + 2 * PE_K * 4;
    return shared + edit + dcn + B * G * PW_BEAM_W + PE_K * PE_K * 2;
}

// [status line | EditNet: h1, attend_cap, c_new, h2, projections, caption scores, visual scores | DCNet: h1, h2, projection |
//  normaliser words | candidate words] as flag-in-data words of 8 bytes
size_t pens_xbytes(int B, int D, int A) {
    const size_t G = D / 4;
    return pdec_edit_xbytes(B, D, A, 0) + 8 * ((size_t)B * D * 2 + (size_t)B * A + (size_t)B * G * 4 + (size_t)B * G * PW_BEAM_W);
}

bool pens_dims_ok(const SetEditNetDims* de, const SetDcnetDims* dd) {
    return de->B == dd->B && de->T == dd->T && de->V == dd->V && de->D == dd->D && de->A == dd->A && !de->adaptive && de->B >= 1 &&
           de->B <= PE_K;
}

}  // namespace

}  // namespace set

using namespace set;

extern "C" {

size_t set_ensemble_beam_xbuf_bytes(const SetEditNetDims* de, const SetDcnetDims* dd) {
    if (!de || !dd || !pens_dims_ok(de, dd) || de->D <= 0 || de->A <= 0) return 0;
    return pens_xbytes(de->B, de->D, de->A);
}

// hist_score: NULL for set_ensemble_beam_persistent (nothing written), the n-best entry's array otherwise
static int ensemble_beam_persistent(const SetEditNetWeights* we, const SetEditNetDims* de, const SetDcnetWeights* wd,
                                    const SetDcnetDims* dd, const float* X, const int64_t* prev, const int64_t* prevlen,
                                    int64_t start_idx, int64_t end_idx, int max_picks, int32_t* hist_parent, int64_t* hist_word,
                                    float* hist_score, float* best_score, int64_t* best_word, int32_t* result, void* ws_e,
                                    size_t ws_e_bytes, void* ws_d, size_t ws_d_bytes, void* xbuf, size_t xbuf_bytes, void* stream) {
    if (!we || !de || !wd || !dd || !X || !prev || !prevlen || !hist_parent || !hist_word || !best_score || !best_word || !result ||
        !ws_e || !ws_d || !xbuf || max_picks < 1)
        return SET_ERR_ARG;
    if (start_idx < 0 || start_idx >= de->V || start_idx >= dd->V) return SET_ERR_ARG;
    // (nothing is touched before the checks that can answer SET_ERR_UNSUPPORTED)
    if (!pens_dims_ok(de, dd)) return SET_ERR_UNSUPPORTED;       // rows, T or vocabulary differ; adaptive features; k > 4
    SET_TRY(editnet_ensemble_check(we, de, ws_e, ws_e_bytes));
    SET_TRY(dcnet_ensemble_check(wd, dd, max_picks, ws_d, ws_d_bytes));
    const int B = de->B, D = de->D, A = de->A, G = D / 4;
    if (!aligned16(xbuf)) return SET_ERR_ARG;
    if (xbuf_bytes < pens_xbytes(B, D, A)) return SET_ERR_WORKSPACE;
    const int lds = pens_lds_floats(B, D, A) * (int)sizeof(float);
    const int lds_max = pens_lds_floats(PE_K, D, A) * (int)sizeof(float);
    if (lds_max > 156 * 1024 || lds_max + 4096 > persistent_lds_limit()) return SET_ERR_UNSUPPORTED;   // (a 64-KB-LDS device)
    hipStream_t st = (hipStream_t)stream;
    PEnsEditPro pe;
    PEnsDcnetPro pd;
    SET_TRY(editnet_ensemble_prologue(we, de, X, prev, prevlen, ws_e, st, &pe));
    SET_TRY(dcnet_ensemble_prologue(wd, dd, prev, prevlen, ws_d, st, &pd));

    PDecEnsArgs P{};
    pdec_edit_fill(P.e, we, de, max_picks);
    P.e.pre1 = pe.pre1; P.e.att1 = pe.att1; P.e.att1_c = pe.att1_c; P.e.mask = pe.mask; P.e.capP = pe.capP; P.e.memQ = pe.memQ;
    P.e.Mem = pe.Mem; P.e.pv = pe.pv;
    P.e.start_idx = start_idx; P.e.end_idx = end_idx;
    pdec_beam_fill(P.e, PDecBeam{hist_parent, hist_word, best_score, best_word, result, nullptr, hist_score});
    pdec_dcnet_fill(P.d, wd, dd);
    P.d.pre1 = pd.pre1; P.d.att1_c = pd.att1_c; P.d.mask = pd.mask; P.d.pc = pd.pc;
    char* x = pdec_edit_layout(P.e, (char*)xbuf);            // (R <= 36 here: 64 visual scores per row, as the kernel reads them)
    x = pdec_dcnet_layout(P.d, x, B, D, A);
    P.x_lse = x; x += (size_t)B * G * 4 * 8;
    P.x_cand = x;
    PersistentGuard guard;
    if (guard.rc != SET_OK) return guard.rc;
    pdec_guard_fill(P.e, guard);
    static PersistentKernel kern = {reinterpret_cast<const void*>(&ensemble_persistent_k)};
    const double wbytes = 4.0 * (2.0 * (double)de->V * D + 9.0 * 4 * D * D + 3.0 * D * D + 3.0 * A * D);
    return pdec_launch(kern, guard, G, lds, lds_max, &P, xbuf, pens_xbytes(B, D, A), st,
                       {"persistent_beam_ensemble", 2.0 * B * wbytes / 4.0 * max_picks, wbytes * max_picks},
                       {&P.e.stamps, &P.e.stamp_wg, 20, max_picks});
}

int set_ensemble_beam_persistent(const SetEditNetWeights* we, const SetEditNetDims* de, const SetDcnetWeights* wd,
                                 const SetDcnetDims* dd, const float* X, const int64_t* prev, const int64_t* prevlen,
                                 int64_t start_idx, int64_t end_idx, int max_picks, int32_t* hist_parent, int64_t* hist_word,
                                 float* best_score, int64_t* best_word, int32_t* result, void* ws_e, size_t ws_e_bytes, void* ws_d,
                                 size_t ws_d_bytes, void* xbuf, size_t xbuf_bytes, void* stream) {
    return ensemble_beam_persistent(we, de, wd, dd, X, prev, prevlen, start_idx, end_idx, max_picks, hist_parent, hist_word, nullptr,
                                    best_score, best_word, result, ws_e, ws_e_bytes, ws_d, ws_d_bytes, xbuf, xbuf_bytes, stream);
}

int set_ensemble_beam_persistent_nbest(const SetEditNetWeights* we, const SetEditNetDims* de, const SetDcnetWeights* wd,
                                       const SetDcnetDims* dd, const float* X, const int64_t* prev, const int64_t* prevlen,
                                       int64_t start_idx, int64_t end_idx, int max_picks, int32_t* hist_parent, int64_t* hist_word,
                                       float* best_score, int64_t* best_word, int32_t* result, void* ws_e, size_t ws_e_bytes,
                                       void* ws_d, size_t ws_d_bytes, void* xbuf, size_t xbuf_bytes, void* stream,
                                       float* hist_score) {
    if (!hist_score) return SET_ERR_ARG;
    return ensemble_beam_persistent(we, de, wd, dd, X, prev, prevlen, start_idx, end_idx, max_picks, hist_parent, hist_word, hist_score,
                                    best_score, best_word, result, ws_e, ws_e_bytes, ws_d, ws_d_bytes, xbuf, xbuf_bytes, stream);
}

}  // extern "C"
