/*
 * set_hip.h — C ABI of libset_hip.so: the EditNet / DCNet per-timestep decode path of
 * show-edit-tell as hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference (fawazsammani/show-edit-tell) has no FFI: its boundary for this path is the
 * Python nn.Module surface.  Each entry point below replaces the PyTorch ops
 * behind one of those module calls; the reference file:line it replaces is cited on each.  The
 * Python host side (show-edit-tell_amd/*.py) binds these with ctypes and keeps the reference's
 * class names, constructor signatures, attribute names and state_dict keys.
 *
 * Conventions
 *   - all tensors fp32 row-major contiguous unless a leading stride is given; ids/lengths int64
 *   - weights are PyTorch (out,in) row-major and are used IN PLACE (no repacking)
 *   - every pointer is a DEVICE pointer unless named host_*; nothing is allocated or freed here:
 *     the caller supplies a workspace sized by the matching *_workspace_bytes() query
 *   - all work is enqueued on `stream` (a hipStream_t); functions never synchronise
 *   - return value: SET_OK or an error code; nothing throws across the ABI
 *   - re-entrant per (workspace, stream) pair.  State outside the caller's workspace, all of it listed here:
 *       thread-local (per calling host thread): the last hipError_t (set_last_hip_error), the row-limit pointer
 *         (set_decode_row_limits), the loop gate the decode loops set around each timestep for their own launchers, the
 *         opt-in profiler's records (set_profile_enable);
 *       process-wide, per device: one mutex + completion-event chain that admits ONE persistent launch at a time (caption
 *         encoder, small-batch decode loop: their workgroups must all be resident), the sticky host-mapped fault word and
 *         "persistent kernels disabled" flag behind SET_ERR_FAULT, cached answers of occupancy / LDS-limit queries and of
 *         "dynamic-LDS cap raised for kernel X on device d";
 *       machine-wide, per device: an advisory lock on /tmp/set_hip_persistent_<pci bus id>.lock (SET_PERSISTENT_LOCK_DIR
 *         moves it, SET_PERSISTENT_IPC_LOCK=0 switches it off) held until exit by the FIRST process that makes a persistent
 *         launch on the device; every other process sharing that GPU is answered SET_ERR_UNSUPPORTED by the persistent
 *         entry points (the per-step kernels; asked again at each call) — two half-resident grids of two processes would
 *         otherwise wait for each other until the time-out;
 *       environment: SET_* switches are read once per process, except SET_DEC_PERSISTENT / SET_DEC_PERSISTENT_MAXB, which
 *         the small-batch decode reads per call (tests flip them inside one process).
 *     None of it carries results between calls: outputs depend on the arguments only.
 *   - alignment: base pointers 16-byte aligned, leading strides and K multiples of 4 floats;
 *     every contraction length (D, A, F, 2D, ...) must be a multiple of 32 (SET_ERR_UNSUPPORTED)
 */
#ifndef SET_HIP_H
#define SET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SET_OK 0
#define SET_ERR_ARG 1          /* null pointer / non-positive size / misaligned */
#define SET_ERR_UNSUPPORTED 2  /* dimension not supported by the kernels (see alignment rules) */
#define SET_ERR_HIP 3          /* a HIP runtime call failed: see set_last_hip_error() */
#define SET_ERR_WORKSPACE 4    /* workspace too small */
#define SET_ERR_FAULT 5        /* an EARLIER call's persistent launch (caption encoder, small-batch decode loop) timed out
                                  waiting for its workgroups: that call's outputs were overwritten with NaN on the device;
                                  reported once, at the next call that would have used such a kernel; the library uses the
                                  per-step kernels from then on (retry succeeds) */

#define SET_ACT_NONE 0
#define SET_ACT_RELU 1
#define SET_ACT_TANH 2
#define SET_ACT_SIGMOID 3

int set_abi_version(void);
const char* set_error_string(int code);
/* last hipError_t seen by this thread inside the library (0 = none) and its text */
int set_last_hip_error(void);
const char* set_last_hip_error_string(void);
/* device the library was compiled for ("gfx950") */
const char* set_target_arch(void);

/* ------------------------------------------------------------------------------------------
 * Opt-in per-kernel timing (HIP events on the launch stream); used by bench.py.  Not part of the
 * reference's surface.  set_profile_enable(1) clears previous records; set_profile_report
 * synchronises the events and aggregates by kernel tag, returning the number of entries.
 * flops / bytes are the ALGORITHMIC work of the recorded launches, not counters.
 * ------------------------------------------------------------------------------------------ */
typedef struct SetProfileEntry {
    char tag[32];
    int launches;
    double ms;
    double flops;
    double bytes;
} SetProfileEntry;
int set_profile_enable(int on);
int set_profile_report(SetProfileEntry* out, int max_entries);

/* ------------------------------------------------------------------------------------------
 * EditNet (reference editnet.py:449-548 `DecoderC`, editnet_rl.py:455-549)
 * ------------------------------------------------------------------------------------------ */
typedef struct SetEditNetDims {
    int B;      /* batch rows held by the workspace                                    */
    int T;      /* padded previous-caption length (18 in the reference data, 20 in BASELINE) */
    int R;      /* regions per image (36; up to 100 for adaptive features)              */
    int F;      /* image_features_dim (2048)                                            */
    int D;      /* decoder_dim == emb_dim == caption_features_dim (1024)                */
    int A;      /* attention_dim (512)                                                  */
    int V;      /* vocabulary size                                                      */
    int maxT;   /* XE: max decode length (predictions.shape[1]); greedy: max_len + 1    */
    int adaptive; /* 1: adaptive-features visual attention (editnet_adaptive.py:438-457) */
} SetEditNetDims;

/* state_dict tensors of DecoderC, device pointers, used in place */
typedef struct SetEditNetWeights {
    const float* embed;                     /* embed.embedding.weight (V,D)                         */
    const float *enc_x2h_w, *enc_x2h_b;     /* caption_encoder.lstm_encoder_cell.x2h (4D,D)         */
    const float *enc_h2h_w, *enc_h2h_b;     /* caption_encoder.lstm_encoder_cell.h2h (4D,D)         */
    const float *enc_aff_w, *enc_aff_b;     /* caption_encoder.affine_hn (D,D)                      */
    const float *ca_feat_w, *ca_feat_b;     /* caption_attention.cap_features_att (A,D)             */
    const float *ca_dec_w, *ca_dec_b;       /* caption_attention.cap_decoder_att (A,D)              */
    const float *ca_full_w, *ca_full_b;     /* caption_attention.cap_full_att (1,A)                 */
    const float *ca_gate_w, *ca_gate_b;     /* caption_attention.context_gate (D,3D)                */
    const float *ca_sc_w, *ca_sc_b;         /* caption_attention.sc_affine (D,D)                    */
    const float *ca_tc_w, *ca_tc_b;         /* caption_attention.tc_affine (D,2D)                   */
    const float *va_emb_w, *va_emb_b;       /* visual_attention.att_embed.0 (D,F)                   */
    const float *va_feat_w, *va_feat_b;     /* visual_attention.features_att (A,D)                  */
    const float *va_dec_w, *va_dec_b;       /* visual_attention.decoder_att (A,D)                   */
    const float *va_full_w, *va_full_b;     /* visual_attention.full_att (1,A)                      */
    const float *al_wih, *al_whh;           /* attention_lstm.weight_ih (4D,3D+F), weight_hh (4D,D) */
    const float *al_bih, *al_bhh;           /* attention_lstm.bias_ih / bias_hh (4D)                */
    const float *cl_x2h_w, *cl_x2h_b;       /* copy_lstm.x2h (4D,2D+F)                              */
    const float *cl_h2h_w, *cl_h2h_b;       /* copy_lstm.h2h (4D,D)                                 */
    const float *cl_cnew_w, *cl_cnew_b;     /* copy_lstm.gate_cnew (D,D)                            */
    const float *cl_cmem_w, *cl_cmem_b;     /* copy_lstm.gate_cmem (D,D)                            */
    const float *fc_w, *fc_b;               /* fc (V,D)                                             */
    /* optional DERIVED tensor (NULL = unused): token table (V,10D) built by set_editnet_build_token_table,
     * row v = relu(E[v]) x [W_ih[:, :D] ; tc_affine.W[:, :D] ; context_gate.W[:, :D] ; enc.x2h.W]^T
     * (+ enc.x2h.bias on the last 4D columns) — the contractions whose input is only a token: three of
     * the decode step (editnet.py:527,378-379) and the encoder's input projection (editnet.py:335).
     * Valid while embed / attention_lstm.weight_ih / tc_affine / context_gate / lstm_encoder_cell.x2h
     * are unchanged (inference). */
    const float* tok_table;
} SetEditNetWeights;

size_t set_editnet_workspace_bytes(const SetEditNetDims* d);

/* Inference-time folding of the token-only contractions into a (V,10D) lookup table (see tok_table). */
size_t set_editnet_token_table_bytes(const SetEditNetDims* d);          /* bytes of the table itself   */
size_t set_editnet_token_table_workspace_bytes(const SetEditNetDims* d);
int set_editnet_build_token_table(const SetEditNetWeights* w, const SetEditNetDims* d, float* table,
                                  void* ws, size_t ws_bytes, void* stream);

/* Per-sequence prologue.  Replaces, for one batch: caption_encoder(prev, prevlen)
 * (editnet.py:319-348, called at :501), image_mean = X.mean(1) (:503), init_hidden_state (:494-495)
 * and — eval mode only — the loop-invariant projections that the reference recomputes every
 * timestep: features_att(att_embed(X)) (:441-442), cap_features_att(H) (:370) and the
 * final_hidden / image_mean columns of the attention_lstm input product (:527-532).
 * `image_mean` may be NULL (computed here) or a (B,F) tensor (adaptive variant, editnet_adaptive.py:501).
 * `prev` (B,T) int64, `prevlen` (B) int64, `X` (B,R,F).  Leaves the recurrent state zeroed.
 * Always the fp32 kernels.  Pairs with set_editnet_step and every consumer but set_editnet_greedy_begun. */
int set_editnet_begin(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                      const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                      void* ws, size_t ws_bytes, void* stream);

/* The same prologue as set_editnet_greedy runs it for these dims: from 65 rows on (fixed features) its grouped GEMM launches
 * run on the split-precision kernel (see set_editnet_greedy), below that and with adaptive features it is set_editnet_begin
 * bit for bit.  Pairs with set_editnet_greedy_begun, whose result on such a workspace has the bits of set_editnet_greedy. */
int set_editnet_begin_greedy(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                             const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                             void* ws, size_t ws_bytes, void* stream);

/* One decode timestep for rows [0,bt): embed -> attention_lstm -> caption_attention ->
 * visual_attention -> select -> copy_lstm -> fc  (editnet.py:513-546, editnet_rl.py:505-513),
 * eval mode.  `tokens` (bt) int64 device ids, or NULL to feed the token the previous
 * set_editnet_greedy_pick produced (its fused embedding gather).  `X` is the same (B,R,F) feature
 * tensor given to set_editnet_begin.  `logits` (bt,V) with leading stride ld_logits. */
int set_editnet_step(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                     const int64_t* tokens, int64_t tokens_stride, int bt, float* logits,
                     int64_t ld_logits, void* ws, size_t ws_bytes, void* stream);

/* Greedy epilogue of one free-running step (editnet_rl.py:514-543): log_softmax, argmax (first
 * index on ties), <end> -> 0, `unfinished` latch, seq[:,t] / seqLogprobs[:,t] stores; suppressed
 * once every row has finished (the reference's `break`, :546), and the next step's embedding
 * relu(E[it]) (editnet.py:300-304) gathered into the workspace.  seq (B,max_len) int64,
 * seq_logp (B,max_len) fp32, both pre-zeroed by the caller; call with t = 0,1,2,... in order. */
int set_editnet_greedy_pick(const SetEditNetWeights* w, const SetEditNetDims* d, const float* logits,
                            int64_t ld_logits, int t, int64_t end_idx, int64_t* seq, float* seq_logp,
                            int max_len, void* ws, size_t ws_bytes, void* stream);

/* Whole free-running greedy decode (editnet_rl.py:485-549 with sample_max=True): prologue +
 * (max_len+1) timesteps, no host synchronisation (the reference syncs every step at :546).
 * Outputs seq (B,max_len) int64 and seq_logp (B,max_len) fp32 (overwritten).
 * Numerics: from 65 rows on (fixed features) the grouped GEMM launches of this call's prologue (the caption projections with
 * their row list, att_embed, features_att, the attention LSTM's constant columns; not the caption encoder) and of its timestep
 * loop, of set_editnet_begin_greedy and of set_editnet_greedy_begun run on the split-precision kernel (fp32 operands as three
 * exact bf16 planes, fp32 accumulation; see set_gemm_nt_group_f32, set_gemm_nt_greedy_scope): logits agree with the fp32
 * kernels' to the 1e-4 target, not bit for bit; the same inputs give the same bits every time.  SET_GEMM_SPLIT=0 in the
 * environment keeps the fp32 kernels everywhere; SET_PRO_SPLIT=0 keeps them for the prologue alone.  Below 65 rows, with
 * adaptive features, and in every other entry point of this header (set_editnet_begin among them) nothing changes. */
int set_editnet_greedy(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                       const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                       int64_t start_idx, int64_t end_idx, int max_len, int64_t* seq,
                       float* seq_logp, void* ws, size_t ws_bytes, void* stream);

/* Per-row cap on the caption length of the free-running GREEDY loops (set_*_greedy) for the CALLING host thread: while
 * `row_limit_dev` (B int32 on the device; the pointer is read by the launches of later calls, keep it alive) is set, the
 * pick of timestep t takes <end> for every row b with t + 1 >= row_limit_dev[b] whatever the scores say — row b's caption has
 * at most row_limit_dev[b] words (the recorded log-prob of that step stays the arg-max's; every other row and every earlier
 * position is untouched, tests/test_hip_finished_rows.py).  NULL (default): off = the reference's loop (editnet_rl.py:503-547,
 * one global max_len).  While set, small batches take the per-step kernels (the persistent launch has no cap).  Also how
 * bench.py gives a random-weight model the finish times of real captions (secondary.realistic_lengths).
 * In every mode the GEMM / attention kernels of a timestep return at once after the reference's `break` (all rows finished). */
int set_decode_row_limits(const int* row_limit_dev);

/* The timestep loop of set_editnet_greedy alone (editnet_rl.py:503-547) on a workspace that already holds a completed
 * set_editnet_begin_greedy for the same (X, prev, prevlen): the per-sequence prologue (editnet_rl.py:499-501 and the hoisted
 * projections) of batch i+1 depends on nothing in the decode of batch i, so a caller that issues one decode after the
 * other can run set_editnet_begin_greedy for the NEXT batch on a second stream / workspace while this loop runs
 * (pipeline.DevicePrefetcher(begin_ahead=...) does).  The caller orders `stream` after the stream that ran the prologue.
 * Results are bit-identical to set_editnet_greedy.  (On a set_editnet_begin workspace the loop runs as well; from 65 rows on
 * its result then is that of SET_PRO_SPLIT=0: within the 1e-4 target of set_editnet_greedy, not its bits.) */
int set_editnet_greedy_begun(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X, int64_t start_idx,
                             int64_t end_idx, int max_len, int64_t* seq, float* seq_logp, void* ws,
                             size_t ws_bytes, void* stream);

/* Beam search of ONE image, the reference's own evaluate() shape (editnet.py:601-713: batch = 1 image, beam k = 3), as
 * prologue + ONE persistent launch (csrc/decode_persistent_wide.hip, beam mode): the d->B <= 4 rows of the workspace are the
 * k hypotheses — X (k, R, F), prev (k, T), prevlen (k) hold the image's inputs k times — and every timestep ends with the
 * reference's pick (editnet.py:654-699: log-softmax, + running scores, flat top-k over k V, parent / word split, completed
 * hypotheses leave, k shrinks) instead of the arg-max; recurrent state follows the parent map inside the launch.  The
 * search stops when every hypothesis has ended or after max_picks picks (the reference's 50-step limit: max_picks = 51).
 * Outputs (device): hist_parent / hist_word (max_picks, 4) = parent slot and appended word of every slot after every pick —
 * the host follows them back to read a sequence; best_score / best_word [1] and result [4] = {pick index of the best
 * completed hypothesis (-1: none), its parent slot, hypotheses still alive, picks made}.  A time-out poisons best_score with
 * NaN and result[2..3] = -1 (SET_ERR_FAULT at the next call).  Adaptive features (d->adaptive, the reference's
 * adaptive_features/editnet_adaptive.py:614-735): image_mean (k, F) is the image's own mean (NULL: the mean over all R
 * regions), R even and <= 128; the zero-padded regions are masked in the visual attention (scores -1e10, weights exactly 0),
 * on a kernel instantiation with room for 128 regions.  SET_ERR_UNSUPPORTED (take set_editnet_step +
 * set_beam_pick_f32): no token table, k > 4, an odd R or more than 128 adaptive regions (36 fixed ones), dimensions the
 * persistent launch does not cover, another
 * process owns the device's persistent launches — all answered BEFORE anything is touched; only a device whose LDS limit or
 * resident-workgroup capacity turns out too small is answered after the prologue has been written into `ws` (outputs
 * untouched; the answer is the same for every later call with these dims, so a caller remembers it).
 * Parity: tests/test_hip_beam.py against the reference's beam goldens. */
int set_editnet_beam_persistent(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                                const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                                int64_t start_idx, int64_t end_idx, int max_picks, int32_t* hist_parent,
                                int64_t* hist_word, float* best_score, int64_t* best_word, int32_t* result,
                                void* ws, size_t ws_bytes, void* stream);
/* The same search, the same launch and the same bytes in every output above, plus the N-BEST list: hist_score (max_picks, 4)
 * float, laid out like hist_word.  hist_score[t][s] = the value (sum of log-probabilities) of the pick behind slot s after pick t
 * if that pick COUNTED (it was among the first k_left of the pick: the hypothesis stays alive or has just completed), -inf
 * otherwise.  The hypotheses completed by pick t are therefore the slots with hist_word[t][s] == end_idx and hist_score[t][s] >
 * -inf (a slot whose word is <end> but whose pick did not count looks the same in hist_word alone); their score is
 * hist_score[t][s] and their words are read by following hist_parent back from (t, s), as for the best hypothesis.  COMPLETION
 * ORDER: by pick t ascending and, within a pick, by slot ascending — completed slots keep their pick-rank order (value
 * descending, flat index ascending among equals).  A search completes at most k hypotheses; one that stops at max_picks has
 * fewer, possibly none.  Rows of picks that were not made (t >= result[3]) and slots s >= k are not written, as in hist_word.  SET_ERR_ARG also for a NULL
 * hist_score; every other refusal is that of set_editnet_beam_persistent, answered at the same point.
 * Parity: tests/test_hip_nbest_beam.py. */
int set_editnet_beam_persistent_nbest(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                                      const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                                      int64_t start_idx, int64_t end_idx, int max_picks, int32_t* hist_parent,
                                      int64_t* hist_word, float* best_score, int64_t* best_word, int32_t* result,
                                      void* ws, size_t ws_bytes, void* stream, float* hist_score);

/* The same loop with multinomial sampling (editnet_rl.py:521-528, sample_rl=True, eval mode, no gradients):
 * it ~ Categorical(softmax(logits)) drawn on the device with Philox4x32-10 (counter = (row, timestep, offset),
 * key = seed): reproducible for a given (seed, offset), independent streams for different offsets.
 * seq_logp holds log_softmax(logits)[it].  No host synchronisation. */
int set_editnet_sample(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                       const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                       int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed, uint64_t offset,
                       int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream);

/* Temperature, top-k and nucleus (top-p) truncation of the sampled pick.  NULL and {1, 0, 1} are neutral: the call is then
 * the one without options, bit for bit.  For one row of logits x[v], v < V (slabs summed, bias added):
 *   1. y[v] = x[v] * (1.0f / temperature), the reciprocal formed once on the host in float.
 *   2. top_k (off when 0 or >= V): tk = the top_k-th largest y; kept = {v : y[v] >= tk}.  Every tie at tk is kept, so the
 *      set may hold more than top_k words.
 *   3. top_p (off when 1), over what step 2 kept: m[v] = exp(y[v] - max y), M = sum of m over the kept set; tp = the largest
 *      value whose set {v kept : y[v] >= tp} has mass >= top_p * M; kept = that set — the value group that crosses the mass
 *      is included with all of its ties.
 *   Comparisons are on float values (-0.0 == +0.0).  The kept set always contains the arg-max.
 *   Draw: inverse CDF over the kept set in the kernel's fixed enumeration, the same one Philox uniform per (seed, offset,
 *   row, t); words outside the kept set have mass 0.  step_logp / seq_logp = (y[w] - max y) - log(sum of m over the kept set),
 *   the log-probability under the distribution sampled from; lse = log-sum-exp of y over the kept set.  raw_ids, the <end>
 *   rewrite, the `unfinished` latch, alive, the embedding gather and the LSTM tail are those of the call without options.
 *   Selection is exact and deterministic (bitwise descent over the ordered key of the float: integer counts for top-k, a
 *   fixed-order mass for top-p; no floating-point atomics).
 *   SET_ERR_ARG (before any HIP call, nothing written): temperature not finite or outside [1e-3, 1e3], top_k < 0, top_p not
 *   finite or outside (0, 1]. */
typedef struct SetSampleOpts { float temperature; int32_t top_k; float top_p; int32_t pad_; } SetSampleOpts;
/* set_editnet_sample with the options applied at every timestep */
int set_editnet_sample_opts(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                            const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                            int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed, uint64_t offset,
                            int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                            const SetSampleOpts* opts);

/* Gumbel-max draw: the second sampler of the free-running loops (the inverse-CDF sampler above stays the default and keeps its
 * draws bit for bit).  For one row of logits x[v], v < V (slabs summed, bias added), at timestep t of batch row `row`:
 *   y[v] = fl32(x[v] * (1.0f / temperature))                   — the same inv_t as SetSampleOpts, the product rounded
 *   g[v] = -logf(E),  E = -log(u),  u = (r + 1/2) 2^-32,  r = output word (v & 3) of
 *          Philox4x32-10(key = (seed_lo, seed_hi), counter = (row, t + 256 ((v >> 2) + 1), offset_lo, offset_hi))
 *          E is formed without cancellation: r < 2^31: -logf((r + 0.5f) 2^-32); otherwise -log1pf(-vv) with
 *          vv = (float)(2^32 - r) 2^-32 - 2^-33 from the exact integer.  E is never 0 or infinite; g lies in about [-3.2, 22.9].
 *   s[v] = fl32(y[v] + g[v]);   word = the FIRST maximum of s (ties to the lowest index).
 * The word is exactly a draw from softmax(y).  step_logp / seq_logp = (y[w] - max y) - log sum exp(y - max y) and lse = the
 * log-sum-exp of y are taken over the unperturbed y, as in the untruncated sampled pick; raw_ids, the <end> rewrite, the
 * `unfinished` latch, alive, the embedding gather and the LSTM tail are those of set_sample_pick_f32.
 * The inverse-CDF sampler's uniform uses counter word 1 = t < 256, so the two streams share no counter.  The draw does not
 * depend on the launch geometry: the per-step kernel and the persistent launch draw the same word from the same (seed, offset).
 * SetSampleOpts carries the temperature only.  SET_ERR_ARG (before any HIP call, nothing written): options
 * set_sample_pick_opts_f32 refuses, top_k != 0, top_p != 1, max_len > 255 (or t > 255), V > 2^26 - 4 (the last quad's counter
 * word would wrap onto the uniform's; every V >= 2^26 is refused with it).
 * Float64 restatement: tests/gumbel_oracle.py.
 *
 * set_editnet_sample_gumbel: the free-running loop of set_editnet_sample_opts with this draw, on the per-step kernels. */
int set_editnet_sample_gumbel(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                              const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                              int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed, uint64_t offset,
                              int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                              const SetSampleOpts* opts);
/* The same loop as prologue + ONE persistent launch (csrc/decode_persistent_wide.hip, sampled mode) for 1 .. 16 rows, fixed
 * features and an active token table: every workgroup forms the noise of its own vocabulary rows and publishes, per (row,
 * slice), the slice's log-sum-exp of y, the first arg-max of s, max s and y there; every workgroup combines the slices in slice
 * order.  Tokens are those of set_editnet_sample_gumbel for the same (seed, offset) wherever the two routes' logits (equal to
 * 1e-4) do not bring the two largest perturbed scores within that distance; seq_logp agrees to 1e-4.  A timed-out exchange
 * poisons seq_logp with NaN and seq with 0 (SET_ERR_FAULT at the next call), as in the greedy launch.
 * SET_ERR_UNSUPPORTED (take set_editnet_sample_gumbel), answered BEFORE anything is touched: every case in which
 * set_editnet_beam_persistent answers it for fixed features (no token table, dimensions the launch does not cover, another
 * process owns the device's persistent launches), more than 16 rows, adaptive features, SET_DEC_PERSISTENT=0.  Only a device
 * whose LDS limit or resident-workgroup capacity turns out too small is answered after the prologue has been written into `ws`
 * and seq / seq_logp have been cleared.  SET_ERR_ARG: as above, and max_len > d->maxT.
 * Parity: tests/test_hip_gumbel_sampling.py. */
int set_editnet_gumbel_persistent(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                                  const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                                  int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed, uint64_t offset,
                                  int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                                  const SetSampleOpts* opts);

/* Teacher-forced XE forward (editnet.py:479-548, eval mode, use_ss=False) on a batch already
 * sorted by decreasing caption length.  caps (B,Lc) int64 sorted; host_decode_lengths[B] on the
 * HOST, non-increasing; predictions (B,maxT,V) is fully overwritten (zeros where not decoded). */
int set_editnet_xe_forward(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                           const float* image_mean, const int64_t* caps, int64_t caps_stride,
                           const int* host_decode_lengths, const int64_t* prev,
                           const int64_t* prevlen, float* predictions, void* ws, size_t ws_bytes,
                           void* stream);

/* Edit trace: the per-word record behind the reference's headline figure (demo.png) — the attention over the existing caption,
 * the one position SelectC's hard choice took (editnet.py:403-421) and how far the Copy-LSTM copied the selected memory instead
 * of editing it (editnet.py:281-283) — of a teacher-forced, no-grad decode of GIVEN token sequences.  The recurrent state depends
 * on the token prefix only, so the forced decode of the tokens a search returned (greedy, sampled, beam, ensemble) or of a
 * ground-truth caption repeats the steps that produced them; the persistent launches are not tapped.
 * Step t (0 <= t < S) feeds tokens[b, t] (tokens[b, 0] = <start>; row stride ld_tokens >= S + 1); its record describes how
 * tokens[b, t+1] was produced.  Row b is recorded for t < n_steps[b] (device, B int32, clamped to [0, S]); steps at or beyond
 * n_steps[b] hold 0, with select = -1.  All B rows step together (no sorting, no shrinking batch) on the per-step kernels:
 * set_editnet_begin, then S times set_editnet_step's kernels (token table when attached, region mask when adaptive) followed by
 * gate_cnew(c_new) as one grouped GEMM and ONE record launch (csrc/edit_trace.hip); no host synchronisation, fixed reduction
 * orders.  S <= d->maxT.  Outputs (device, fully overwritten): */
typedef struct {
  float*   alpha_c;    /* (B, S, T)  caption-attention weights; columns >= max prev length of the batch are 0 */
  int32_t* select;     /* (B, S)     arg-max position of alpha_c (first index on ties) = SelectC's hard choice */
  float*   copy_gate;  /* (B, S)     mean over D of sigmoid(gate_cnew(c_new) + gate_cmem(selected memory)) */
  float*   gate_full;  /* (B, S, D)  the gate itself; may be NULL */
  float*   alpha_v;    /* (B, S, R)  visual attention weights; masked / truncated regions 0 (adaptive); may be NULL */
  float*   logp;       /* (B, S)     log_softmax(logits of step t)[tokens[b, t+1]] */
} SetEditTrace;
/* `ws`: set_editnet_workspace_bytes(d) as for every decode (unchanged); `trace_ws`: the trace's own scratch (the gate product's
 * split-K partials), set_editnet_edit_trace_workspace_bytes(d, S) bytes (0: dims / S not admitted), 16-byte aligned.
 * SET_ERR_ARG (null pointers, S < 1, S > d->maxT, ld_tokens < S + 1), SET_ERR_UNSUPPORTED (dimensions the step does not admit)
 * and SET_ERR_WORKSPACE are answered before anything is touched.  Parity: tests/test_hip_edit_trace.py against the oracle's
 * per-step trace. */
size_t set_editnet_edit_trace_workspace_bytes(const SetEditNetDims* d, int S);
int set_editnet_edit_trace(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X, const float* image_mean,
                           const int64_t* prev, const int64_t* prevlen, const int64_t* tokens, int64_t ld_tokens,
                           const int32_t* n_steps, int S, const SetEditTrace* out, void* ws, size_t ws_bytes,
                           void* trace_ws, size_t trace_ws_bytes, void* stream);

/* Debug / module-API accessor: device pointer of a named workspace tensor (NULL if unknown).
 * names: "H" (B,T,D) "M" (B,T,D) "final_hidden" (B,D) "mask" (B,T) "att1" (B,R,A) "att1_c" (B,T,A)
 * "image_mean" (B,F) "h1" "c1" "h2" "c2" "emb" "ctx_cap" "attend_cap" "sel" (B,D) "attend_img" (B,F)
 * "alpha_c" (B,T) "alpha" (B,R) "logits" (B,V) "it" (B) int64 "unfinished" (B) int32
 * "cap_proj" (B,T,2D) = [context_gate.W[:,2D:3D] H | sc_affine.W H] and "mem_proj" (B,T,D) = gate_cmem.W M: the
 * per-sequence hoisted projections the step reads instead of contracting the attention context / selected row;
 * "fe" (B,R,D) = relu(att_embed(X)); "pd_pv" (B,R,4D) = X copy_lstm.x2h.W[:,2D:]^T of the persistent small-batch decode
 * (NULL for batches beyond its row limit, which carve no such buffer; written only where that decode takes the dims) */
void* set_editnet_ws_tensor(const SetEditNetDims* d, void* ws, const char* name);

/* ------------------------------------------------------------------------------------------
 * DCNet (reference dcnet.py:273-350 `DAE`, dcnet_rl.py:256-346) — text only, no image features
 * ------------------------------------------------------------------------------------------ */
typedef struct SetDcnetDims {
    int B, T;
    int D;      /* decoder_dim (1024)                       */
    int A;      /* attention_dim (512)                      */
    int C;      /* caption_features_dim (512); encoder output is 2C */
    int E;      /* emb_dim (1024)                           */
    int V;
    int maxT;
} SetDcnetDims;

typedef struct SetDcnetWeights {
    const float* embed;                          /* embed.embedding.weight (V,E)                  */
    const float *enc_wih_f, *enc_whh_f, *enc_bih_f, *enc_bhh_f;   /* lstm_encoder.*_l0          */
    const float *enc_wih_b, *enc_whh_b, *enc_bih_b, *enc_bhh_b;   /* lstm_encoder.*_l0_reverse  */
    const float *enc_cat_w, *enc_cat_b;          /* caption_encoder.concat (2C,2C)                */
    const float *ca_feat_w, *ca_feat_b;          /* caption_attention.cap_features_att (A,2C)     */
    const float *ca_dec_w, *ca_dec_b;            /* caption_attention.cap_decoder_att (A,D)       */
    const float *ca_full_w, *ca_full_b;          /* caption_attention.cap_full_att (1,A)          */
    const float *al_wih, *al_whh, *al_bih, *al_bhh;   /* attention_lstm (4D,3E),(4D,D)            */
    const float *ll_wih, *ll_whh, *ll_bih, *ll_bhh;   /* language_lstm (4D,2E),(4D,D)             */
    const float *fc_w, *fc_b;                    /* fc (V,D)                                      */
    /* Optional inference-time token table (V, 4D + 8C) or NULL, built by set_dcnet_build_token_table:
     *   [0, 4D)        attention_lstm.weight_ih[:, :E] relu(E[v])            (dcnet.py:336-337)
     *   [4D, 4D+4C)    lstm_encoder.weight_ih_l0 relu(E[v]) + bias_ih_l0      (dcnet.py:233, forward direction)
     *   [4D+4C, 4D+8C) lstm_encoder.weight_ih_l0_reverse relu(E[v]) + bias_ih_l0_reverse
     * Valid while embed / attention_lstm.weight_ih / lstm_encoder.weight_ih* / bias_ih* are unchanged. */
    const float* tok_table;
} SetDcnetWeights;

size_t set_dcnet_workspace_bytes(const SetDcnetDims* d);
size_t set_dcnet_token_table_bytes(const SetDcnetDims* d);
size_t set_dcnet_token_table_workspace_bytes(const SetDcnetDims* d);
int set_dcnet_build_token_table(const SetDcnetWeights* w, const SetDcnetDims* d, float* table, void* ws,
                                size_t ws_bytes, void* stream);
/* caption_encoder (dcnet.py:220-243) + hoisted cap_features_att(enc) (dcnet.py:261) + zero state */
int set_dcnet_begin(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                    const int64_t* prevlen, void* ws, size_t ws_bytes, void* stream);
/* one timestep (dcnet.py:336-347 / dcnet_rl.py:306-312), eval mode */
int set_dcnet_step(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* tokens,
                   int64_t tokens_stride, int bt, float* logits, int64_t ld_logits, void* ws,
                   size_t ws_bytes, void* stream);
/* greedy epilogue of one free-running step (dcnet_rl.py:313-340); see set_editnet_greedy_pick */
int set_dcnet_greedy_pick(const SetDcnetWeights* w, const SetDcnetDims* d, const float* logits,
                          int64_t ld_logits, int t, int64_t end_idx, int64_t* seq, float* seq_logp,
                          int max_len, void* ws, size_t ws_bytes, void* stream);
int set_dcnet_greedy(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                     const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_len,
                     int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream);
/* Beam search of ONE previous caption, the reference's own evaluate() shape (dcnet.py:405-541: batch = 1, beam k = 3), as
 * prologue + ONE persistent launch (csrc/decode_persistent.hip, beam mode): the d->B <= 4 rows of the workspace are the k
 * hypotheses — prev (k, T), prevlen (k) hold the caption's inputs k times, the prologue runs for all k rows — and every
 * timestep ends with the reference's pick (dcnet.py:447-514: log-softmax, + running scores, flat top-k over k V, parent / word
 * split with `//`, completed hypotheses leave, k shrinks) instead of the arg-max; recurrent state follows the parent map inside
 * the launch.  The search stops when every hypothesis has ended or after max_picks picks (the reference's 50-step limit:
 * max_picks = 51).  Outputs (device), the layout of set_editnet_beam_persistent: hist_parent / hist_word (max_picks, 4) = parent
 * slot and appended word of every slot after every pick — the host follows them back to read a sequence; best_score /
 * best_word [1] and result [4] = {pick index of the best completed hypothesis (-1: none), its parent slot, hypotheses still
 * alive, picks made}.  A time-out poisons best_score with NaN and result[2..3] = -1 (SET_ERR_FAULT at the next call).
 * SET_ERR_ARG: null pointers, max_picks < 1, start_idx outside the vocabulary — answered before any HIP call.
 * SET_ERR_UNSUPPORTED (take set_dcnet_step + set_beam_pick_f32): no token table, k > 4, dimensions the persistent launch
 * does not cover (D = E = 2C = 1024, A = 512, T <= 32, V <= 12288), SET_DEC_PERSISTENT=0, k V >= 2^31, another process owns the
 * device's persistent launches — all answered BEFORE anything is touched; only a device whose LDS limit or resident-workgroup
 * capacity turns out too small is answered after the prologue has been written into `ws` (outputs untouched).
 * set_dcnet_workspace_bytes covers the launch's exchange region (for B <= 4 it holds B x 24 KB of candidate words at D = 1024).
 * The ensemble's per-image search has a launch of its own that holds both models' state: set_ensemble_beam_persistent.
 * Parity: tests/test_hip_dcnet_beam.py against the reference's beam goldens and the batched per-step search. */
int set_dcnet_beam_persistent(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                              const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_picks,
                              int32_t* hist_parent, int64_t* hist_word, float* best_score, int64_t* best_word,
                              int32_t* result, void* ws, size_t ws_bytes, void* stream);
/* set_dcnet_beam_persistent plus the n-best list: hist_score (max_picks, 4), the convention and completion order of
 * set_editnet_beam_persistent_nbest (-inf = the slot's pick did not count).  Every other output holds the same bytes. */
int set_dcnet_beam_persistent_nbest(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                                    const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_picks,
                                    int32_t* hist_parent, int64_t* hist_word, float* best_score, int64_t* best_word,
                                    int32_t* result, void* ws, size_t ws_bytes, void* stream, float* hist_score);
/* Beam search of ONE image by the EditNet + DCNet ENSEMBLE, the protocol of the reference's published scores
 * (eval/eval xe/eval_full.py:132-202: batch = 1 image, beam k = 3; both models step on the same words, their softmax
 * probabilities are averaged and the beam is picked from log((softmax_e + softmax_d) / 2) + running scores), as both prologues +
 * ONE persistent launch (csrc/decode_persistent_ensemble.hip) that holds both models' state: the de->B = dd->B <= 4 rows of both
 * workspaces are the k hypotheses — X (k, R, F), prev (k, T), prevlen (k) hold the image's inputs k times, the prologues run as in
 * set_editnet_beam_persistent / set_dcnet_beam_persistent — and every timestep of both models ends with ONE joint pick: per-slice
 * (max, sum exp) of both models are exchanged first, then per-slice candidates of the averaged score (flat top-k over k V, value
 * descending, flat index ascending, parent / word split, completed hypotheses leave, k shrinks); both models' recurrent state
 * follows the one parent map inside the launch.  Fixed features only (the image mean is the mean over all R regions).  The
 * search stops when every hypothesis has ended or after max_picks picks (the reference's 50-step limit: max_picks = 51).
 * Outputs (device), the layout of set_editnet_beam_persistent: hist_parent / hist_word (max_picks, 4), best_score / best_word [1],
 * result [4] = {pick index of the best completed hypothesis (-1: none), its parent slot, hypotheses still alive, picks made}.  A
 * time-out poisons best_score with NaN and result[2..3] = -1 (SET_ERR_FAULT at the next call).  xbuf: the launch's exchange
 * region, 16-byte aligned, set_ensemble_beam_xbuf_bytes(de, dd) bytes (0: these dims have no such launch), zero-filled by the
 * call; the exchange regions inside ws_e / ws_d are not used and no workspace size changed.
 * SET_ERR_ARG: null pointers, max_picks < 1, start_idx outside the vocabulary — answered before any HIP call.
 * SET_ERR_UNSUPPORTED (take set_*_step + set_beam_pick_f32): de->B != dd->B, T, D, A or the VOCABULARY SIZE differ between the
 * models, an adaptive decoder, and whatever either sibling refuses (no token table, k > 4, dimensions outside its launch,
 * SET_DEC_PERSISTENT=0, k V >= 2^31, another process owns the device's persistent launches) — all answered BEFORE anything is
 * touched; only a device whose LDS limit or resident-workgroup capacity turns out too small is answered after the prologues have
 * been written into ws_e / ws_d (outputs untouched).
 * Parity: tests/test_hip_ensemble_beam.py against the reference's beam goldens and the batched per-step search. */
int set_ensemble_beam_persistent(const SetEditNetWeights* we, const SetEditNetDims* de, const SetDcnetWeights* wd,
                                 const SetDcnetDims* dd, const float* X, const int64_t* prev, const int64_t* prevlen,
                                 int64_t start_idx, int64_t end_idx, int max_picks, int32_t* hist_parent,
                                 int64_t* hist_word, float* best_score, int64_t* best_word, int32_t* result,
                                 void* ws_e, size_t ws_e_bytes, void* ws_d, size_t ws_d_bytes, void* xbuf,
                                 size_t xbuf_bytes, void* stream);
/* set_ensemble_beam_persistent plus the n-best list: hist_score (max_picks, 4), the convention and completion order of
 * set_editnet_beam_persistent_nbest; the scores are those of the joint pick.  Every other output holds the same bytes. */
int set_ensemble_beam_persistent_nbest(const SetEditNetWeights* we, const SetEditNetDims* de, const SetDcnetWeights* wd,
                                       const SetDcnetDims* dd, const float* X, const int64_t* prev,
                                       const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_picks,
                                       int32_t* hist_parent, int64_t* hist_word, float* best_score, int64_t* best_word,
                                       int32_t* result, void* ws_e, size_t ws_e_bytes, void* ws_d, size_t ws_d_bytes,
                                       void* xbuf, size_t xbuf_bytes, void* stream, float* hist_score);
size_t set_ensemble_beam_xbuf_bytes(const SetEditNetDims* de, const SetDcnetDims* dd);
/* multinomial twin of set_dcnet_greedy (dcnet_rl.py:320-327); see set_editnet_sample */
int set_dcnet_sample(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                     const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed,
                     uint64_t offset, int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream);
/* set_dcnet_sample with SetSampleOpts applied at every timestep (see set_editnet_sample_opts) */
int set_dcnet_sample_opts(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                          const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed,
                          uint64_t offset, int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                          const SetSampleOpts* opts);
/* the loop of set_dcnet_sample_opts with the Gumbel-max draw (the contract above set_editnet_sample_gumbel), on the per-step
 * kernels */
int set_dcnet_sample_gumbel(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                            const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed,
                            uint64_t offset, int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                            const SetSampleOpts* opts);
/* The same loop as prologue + ONE persistent launch (csrc/decode_persistent.hip, sampled mode) for 1 .. 8 rows and an active
 * token table: every workgroup forms the noise of its own vocabulary rows and publishes, per (row, slice), the slice's
 * log-sum-exp of y, the first arg-max of s, max s and y there (the four words of the greedy launch's fc exchange); every
 * workgroup combines the slices in slice order.  Tokens are those of set_dcnet_sample_gumbel for the same (seed, offset) wherever
 * the two routes' logits (equal to 1e-4) do not bring the two largest perturbed scores within that distance; seq_logp agrees to
 * 1e-4.  A timed-out exchange poisons seq_logp with NaN and seq with 0 (SET_ERR_FAULT at the next call), as in the greedy launch.
 * SET_ERR_UNSUPPORTED (take set_dcnet_sample_gumbel), answered BEFORE anything is touched: no token table, more than 8 rows,
 * dimensions the launch does not cover, SET_DEC_PERSISTENT=0, row limits in force (set_decode_row_limits), another process owns
 * the device's persistent launches.  Only a device whose LDS limit or resident-workgroup capacity turns out too small is answered
 * after the prologue has been written into `ws` and seq / seq_logp have been cleared.  SET_ERR_ARG: as above set_editnet_sample_gumbel,
 * and max_len > d->maxT.
 * Parity: tests/test_hip_dcnet_gumbel_persistent.py. */
int set_dcnet_gumbel_persistent(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                                const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed,
                                uint64_t offset, int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                                const SetSampleOpts* opts);
int set_dcnet_xe_forward(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* caps,
                         int64_t caps_stride, const int* host_decode_lengths, const int64_t* prev,
                         const int64_t* prevlen, float* predictions, void* ws, size_t ws_bytes,
                         void* stream);
/* set_dcnet_xe_forward that also writes last_hidden (B, D), sorted row order (dcnet_with_mse.py:321,341,
 * `decoder_last_hidden[:batch_size_t] = h2.clone()`): h2 of row b at its last step t = host_decode_lengths[b] - 1,
 * before the output dropout; zeros for a row of decode length 0.  last_hidden == NULL: set_dcnet_xe_forward. */
int set_dcnet_xe_forward_hidden(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* caps,
                                int64_t caps_stride, const int* host_decode_lengths, const int64_t* prev,
                                const int64_t* prevlen, float* predictions, float* last_hidden, void* ws,
                                size_t ws_bytes, void* stream);
/* names: "enc" (B,T,2C) "final_hidden" (B,2C) "mask" (B,T) "att1_c" (B,T,A) "h1" "c1" "h2" "c2"
 * "emb" "attend_cap" (B,2C) "alpha_c" (B,T) "logits" (B,V) "it" "unfinished"
 * "enc_bar" the barrier words of the persistent encoder and, behind them, its status word (as EditNet's)
 * "pd_pc" (B,T,4D) = enc language_lstm.W_ih[:,D:]^T of the persistent small-batch decode (NULL for batches beyond its row
 * limit, which carve no such buffer; written only where that decode takes the dims) */
void* set_dcnet_ws_tensor(const SetDcnetDims* d, void* ws, const char* name);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points (the sub-module `forward`s the reference's beam search calls
 * directly, editnet.py:645-653 / eval_full.py:133-149)
 * ------------------------------------------------------------------------------------------ */
/* y = act(x W^T + bias): nn.Linear (+ ReLU/tanh/sigmoid).  x (M,K) ldx, w (N,K) ldw, y (M,N) ldy */
size_t set_linear_workspace_bytes(int M, int N, int K);
int set_linear_f32(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias,
                   float* y, int64_t ldy, int M, int N, int K, int act, void* ws, size_t ws_bytes,
                   void* stream);
/* The grouped NT GEMM under every forward contraction (csrc/gemm_f32.hip), as its launcher takes it: up to 6 problems
 *     C_i[M_i, N_i] = act_i(sum over segments s of A_is[M_i, K_is] W_is[N_i, K_is]^T + bias_i)
 * in ONE launch, each contraction a concatenation of up to 3 (A, W) column segments that stay where they lie (every K a
 * multiple of 32; A, W 16-byte aligned, lda / ldw multiples of 4 floats and >= K).  For direct tests and measurements of the
 * kernel family: tile class, split, segment layout, row gate and k-loop are the caller's to choose.
 *   ksplit   0: the launcher's planner decides.  >= 1: that many K slices, clamped to the problem's k-tiles (K_total / 32).
 *            A problem that ends up split writes its partials into `ws` and is reduced into C with bias and activation by a
 *            second launch (as set_linear_f32 does); an unsplit one runs the fused epilogue straight into C.
 *   bm_hint  0: row-tile class from the largest M (<= 16 rows: 16, <= 32: 32, <= 512: 64, beyond: 128 or 64 by the tile
 *            model).  64 / 128: forced for the whole launch.
 *   row_list, row_count   both or neither; device memory.  Only rows row_list[0 .. *row_count) of every A are contracted and
 *            only those rows of every C written; indices are clamped to [0, M), the count to [0, M].  Unsplit problems only
 *            (SET_ERR_ARG with ksplit > 1; with ksplit = 0 the problems stay unsplit), not with `alive`, and not on the
 *            <= 16-row class (SET_ERR_UNSUPPORTED).
 *   alive    device int or NULL: *alive == 0 when the kernels start -> the launch writes nothing, neither C nor partials —
 *            the loop-left gate of the free-running decode loops.  The reduction launches carry no gate (the decode loops
 *            hand gated partials to gated consumers), so a split problem takes `alive` only with SET_GEMM_NT_KEEP_SLABS
 *            (SET_ERR_ARG otherwise; with ksplit = 0 the problems stay unsplit).
 *   flags    SET_GEMM_NT_NO_ASM: take the compiler-scheduled k-loop where the hand-written 64x64 one is eligible.  Flips a
 *            process-wide switch around the call: NOT thread-safe, diagnostic only.
 *            SET_GEMM_NT_KEEP_SLABS: no reduction launches; each problem goes to the launcher with its own bias and
 *            activation, so a split one with either is refused (SET_ERR_ARG) and otherwise leaves its partials in `ws`:
 *            problem i's slab s at ws + slab_offset_i + s * M_i * N_i floats, slab_offset_i = the 256-byte-rounded sizes
 *            (ksplit_j * M_j * N_j * 4 bytes) of the split problems j < i.
 *   set_gemm_nt_greedy_scope(1) before the call (0 after it; a switch of the calling thread): plan and launch as the no-grad
 *            greedy rollout of EditNet does.  With SET_GEMM_SPLIT unset, a launch whose problems all have >= 65 rows, without a row list and without bm_hint = 64, then runs on
 *            the 128x64 split-precision kernel (profile tag "gemm_nt_f32<128,64>:bf16x3"): every fp32 operand as three
 *            exact bf16 planes, six partial products accumulated in fp32.  Its error against the exact product is that of
 *            the fp32 kernels (measured: profiles/gemm_split_errors.json), its bits are not theirs; products of small
 *            integers are exact on both.  An element whose split accumulator is not finite (an operand of +-inf, NaN or
 *            |x| >= 2^128 - 2^119, or a true overflow) is recomputed as an fp32 FMA chain, so inf / NaN come out as from the
 *            fp32 kernels.  Without it (every caller but that rollout) and with SET_GEMM_SPLIT=0 the fp32 kernels run.
 *   ksplit_out  NULL or n ints: the split each problem ran with.   rows_out  NULL or one int: the row-tile class.
 * Every refusal is answered before any HIP call. */
#define SET_GEMM_NT_NO_ASM 1
#define SET_GEMM_NT_KEEP_SLABS 2
typedef struct SetGemmNtSeg {
    const float* A; int64_t lda;
    const float* W; int64_t ldw;
    int32_t K, pad_;
} SetGemmNtSeg;
typedef struct SetGemmNtProb {
    SetGemmNtSeg seg[3];
    float* C; int64_t ldc;
    const float* bias;               /* N floats or NULL */
    int32_t nseg, M, N, act, ksplit, pad_;
} SetGemmNtProb;
typedef struct SetGemmNtLaunch {
    const int32_t* row_list; const int32_t* row_count;
    const int32_t* alive;
    int32_t* ksplit_out; int32_t* rows_out;      /* HOST memory */
    int32_t bm_hint, flags;
} SetGemmNtLaunch;
/* upper bound for `ws` of the call below (0 when nothing can be split or an argument is out of range) */
size_t set_gemm_nt_group_workspace_bytes(const SetGemmNtProb* probs, int n);
int set_gemm_nt_greedy_scope(int on);
int set_gemm_nt_group_f32(const SetGemmNtProb* probs, int n, const SetGemmNtLaunch* launch /* NULL: all defaults */,
                          void* ws, size_t ws_bytes, void* stream);
/* EmbeddingC.forward (editnet.py:300-304), eval: out[i] = relu(table[ids[i]]) */
int set_embed_relu_f32(const float* table, const int64_t* ids, int64_t ids_stride, float* out,
                       int64_t ldo, int n, int D, int V, void* stream);
/* nn.LSTMCell / LSTMCellC (editnet.py:226-244): gates = x Wih^T + bih + h Whh^T + bhh, order i,f,g,o */
size_t set_lstm_cell_workspace_bytes(int M, int D, int Kx);
int set_lstm_cell_f32(const float* x, int64_t ldx, int Kx, const float* h, const float* c,
                      const float* w_ih, int64_t ld_wih, const float* w_hh, const float* b_ih,
                      const float* b_hh, float* h_out, float* c_out, int M, int D, void* ws,
                      size_t ws_bytes, void* stream);
/* CaptionAttentionC.forward (editnet.py:364-381); att1_c may be NULL (computed into ws).
 * H (M,T,Dh) caption features, h1 (M,D) decoder state.  Outputs gated (M,Dh), alpha_c (M,T).
 * Also serves DCNet's CaptionAttention (dcnet.py:254-270) when w->ca_gate_w is NULL: `gated`
 * then receives the plain context (M,Dh) (Dh = 2C there; EditNet requires Dh == D). */
size_t set_caption_attention_workspace_bytes(int M, int T, int Dh, int A);
int set_caption_attention_f32(const SetEditNetWeights* w, const float* H, const float* att1_c,
                              const float* h1, const float* word, const float* mask, float* gated,
                              float* alpha_c, int M, int T, int Dh, int D, int A, void* ws,
                              size_t ws_bytes, void* stream);
/* the un-gated form (DCNet, w->ca_gate_w == NULL) that also emits the decoder-side projection incl. bias it scored with,
 * att2_out (M,A) — the `att2` operand of set_attention_bwd_f32 — for the training node */
int set_caption_attention_att2_f32(const SetEditNetWeights* w, const float* H, const float* att1_c, const float* h1,
                                   const float* mask, float* ctx, float* alpha_c, float* att2_out, int M, int T,
                                   int Dh, int D, int A, void* ws, size_t ws_bytes, void* stream);
/* VisualAttentionC.forward (editnet.py:439-447); att1 may be NULL (att_embed + features_att are
 * then recomputed exactly as the reference does every call).  adaptive != 0 selects the masked
 * variant (editnet_adaptive.py:438-457).  ctx (M,F). */
size_t set_visual_attention_workspace_bytes(int M, int R, int F, int D, int A);
int set_visual_attention_f32(const SetEditNetWeights* w, const float* X, const float* att1,
                             const float* h1, float* ctx, float* alpha, int M, int R, int F, int D,
                             int A, int adaptive, void* ws, size_t ws_bytes, void* stream);
/* Same with att1 (M,R,A) required and the region mask rmask (M,R; 1 = valid, NULL = no masking) supplied
 * by the caller instead of re-derived (grad-enabled adaptive path); ws >= the size above. */
int set_visual_attention_masked_f32(const SetEditNetWeights* w, const float* X, const float* att1,
                                    const float* rmask, const float* h1, float* ctx, float* alpha, int M,
                                    int R, int F, int D, int A, void* ws, size_t ws_bytes, void* stream);
/* SelectC.forward hard mode (editnet.py:403-421): sel = M[b,j*] * (a + (1-a)), j* = argmax alpha_c */
int set_select_f32(const float* Mem, const float* alpha_c, float* sel, int M, int T, int D,
                   void* stream);
/* SelectC.forward with soft = True (editnet.py:419-420): sel (M,D) = sum_t alpha_c[b,t] * Mem[b,t,:] (terms added in
 * index order), and its backward: dM[b,t,:] = alpha[b,t] * dsel[b,:], dalpha[b,t] = <dsel[b,:], Mem[b,t,:]>. */
int set_select_soft_f32(const float* Mem, const float* alpha_c, float* sel, int M, int T, int D,
                        void* stream);
int set_select_soft_bwd_f32(const float* dsel, const float* Mem, const float* alpha, float* dM, float* dalpha,
                            int M, int T, int D, void* stream);
/* CopyLSTMCellC.forward (editnet.py:265-285); x (M,2D+F) */
size_t set_copy_lstm_workspace_bytes(int M, int D, int Kx);
int set_copy_lstm_f32(const SetEditNetWeights* w, const float* x, int64_t ldx, int Kx,
                      const float* h2, const float* c2, const float* c_memory, float* h_out,
                      float* c_out, int M, int D, void* ws, size_t ws_bytes, void* stream);
/* CaptionEncoderC.forward (editnet.py:319-348): outputs padded to T (caller slices to max len).
 * H, Mem (B,T,D) ; final_hidden (B,D) ; mask (B,T) */
size_t set_caption_encoder_workspace_bytes(int B, int T, int D);
int set_caption_encoder_f32(const SetEditNetWeights* w, const int64_t* seq, const int64_t* seq_len,
                            float* H, float* Mem, float* final_hidden, float* mask, int B, int T,
                            int D, int V, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training support (the reference's backward is PyTorch autograd over a1-a12,
 * editnet.py:579).  `*_train_f32` = the operator forward that additionally stores what its
 * backward needs (POST-activation gates i,f,g,o; copy gate; context-gate factors); `*_bwd_f32` =
 * the hand-written pointwise / attention part of the operator's backward.  The plain dX = dY W and
 * dW = dY^T X contractions between them are library GEMMs on the PyTorch side (autograd_ops.py).
 * ------------------------------------------------------------------------------------------ */
int set_lstm_cell_train_f32(const float* x, int64_t ldx, int Kx, const float* h, const float* c,
                            const float* w_ih, int64_t ld_wih, const float* w_hh, const float* b_ih,
                            const float* b_hh, float* h_out, float* c_out, float* gates_out, int M, int D,
                            void* ws, size_t ws_bytes, void* stream);
/* dgates (M,4D) = pre-activation gate gradients, dc_prev (M,D); dh / dc may be NULL (zero) */
/* Token cross-entropy of the training loops (editnet.py:571-577, dcnet.py:391-397: pack_padded_sequence of scores and
 * targets, CrossEntropyLoss) on the (B, T, V) scores in place: element (b, t, v) at scores[b*stride_b + t*stride_t + v],
 * target word of (b, t) at targets[b*tstride_b + t*tstride_t].  The batch is sorted by decreasing decode length and
 * live[t] (HOST array, T <= 64 entries, non-increasing) = number of sequences with decode length > t: row (b, t) is one
 * of the packed rows iff b < live[t].  Forward: rowloss (T*B floats, index t*B + b; zeros for dead rows), lse (2*T*B
 * floats: [t*B + b] the row's log-sum-exp rounded to fp32, [T*B + t*B + b] the remainder of that rounding, so that the
 * backward's exp(x - lse) does not inherit half an ulp of |lse| as a relative error of the whole row; zeros for dead rows)
 * and loss_sum (1 float) = the SUM of the token losses (divide by the token count for CrossEntropyLoss's mean).
 * Backward: lse as the forward of the same arguments wrote it; grad (T, B, ld_grad) with ld_grad = V rounded up to 4 —
 * (softmax - onehot) * dloss[0] for live rows, zeros for dead rows and for the padding columns (so the buffer can feed
 * set_gemm_f32 as a zero-padded k-major operand).
 * Both refuse, before any launch and without touching an output: T > 64 (SET_ERR_UNSUPPORTED); a live table with an
 * entry below 0 or above B, or one that increases (SET_ERR_ARG); the backward also ld_grad != V rounded up to 4
 * (SET_ERR_ARG). */
int set_xe_loss_f32(const float* scores, int64_t stride_b, int64_t stride_t, const int64_t* targets, int64_t tstride_b,
                    int64_t tstride_t, const int* live, int B, int T, int V, float* rowloss, float* lse,
                    float* loss_sum, void* stream);
int set_xe_loss_bwd_f32(const float* scores, int64_t stride_b, int64_t stride_t, const int64_t* targets,
                        int64_t tstride_b, int64_t tstride_t, const int* live, int B, int T, int V, const float* lse,
                        const float* dloss, float* grad, int64_t ld_grad, void* stream);
/* nn.MSELoss pieces of the DCNet MSE stage (dcnet_with_mse.py:392).  Forward: *out (device, 1 float) = sum over the n
 * floats of (a[i] - b[i])^2, in one fixed reduction order (the same bits on every call; divide by n for the mean).
 * Backward: da = s (a - b), db = -da with s = scale * dout[0] (dout NULL: s = scale); da or db may be NULL. */
int set_mse_sum_f32(const float* a, const float* b, int64_t n, float* out, void* stream);
int set_mse_bwd_f32(const float* a, const float* b, int64_t n, float scale, const float* dout, float* da, float* db,
                    void* stream);

/* The tail of the training step — torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.Adam.step()
 * (editnet.py:580-581, dcnet.py:399-400, editnet_rl.py:684-686) — over n fp32 tensors in two launches per 40 tensors:
 * per-chunk sums of squares, then the Adam update with the clipping coefficient min(1, max_norm / (norm + 1e-6)) folded
 * into the gradient read (deterministic norm, no host round trip).  All arrays are HOST arrays of length n; the pointers
 * in params / grads / exp_avg / exp_avg_sq are 16-byte aligned DEVICE pointers to numel[i] contiguous floats.  step[i] is
 * the 1-based step count of tensor i (bias corrections and 1 - beta are formed on the host in double, as torch forms
 * them, then rounded to fp32), lr / beta1 / beta2 / eps / weight_decay the hyper-parameters of its param group (weight_decay in torch.optim.Adam's L2 form).  max_norm <= 0: no
 * clipping.  scale_grads != 0: the clipped gradient is also written back (clip_grad_norm_'s in-place effect; costs one
 * more gradient-sized write).  total_norm_out (device, 1 float, may be NULL) receives the gradient norm.
 * ws: set_clip_adam_workspace_bytes(n, numel) bytes. */
size_t set_clip_adam_workspace_bytes(int n, const int64_t* numel);
int set_clip_adam_f32(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const int64_t* numel, const int64_t* step, const double* lr,
                      const double* beta1, const double* beta2, const double* eps, const double* weight_decay,
                      float max_norm, int scale_grads, float* total_norm_out, void* ws, size_t ws_bytes, void* stream);

/* nn.LSTMCell forward (training form, gates saved) for an input that is a concatenation with loop-invariant column
 * blocks: gates = x0 w0^T (+ x1 w1^T) + h w_hh^T + pre, where w0 / w1 are column blocks of weight_ih (row strides
 * ld_w0 / ld_w1) and pre (M,4D) holds the invariant blocks' products plus both biases, contracted once per sequence by
 * the caller (editnet.py:523: final_hidden and image_mean; dcnet.py:336: final_hidden).  x1 may be NULL. */
int set_lstm_cell_pre_train_f32(const float* x0, int64_t ld_x0, const float* w0, int64_t ld_w0, int K0,
                                const float* x1, int64_t ld_x1, const float* w1, int64_t ld_w1, int K1,
                                const float* h, const float* w_hh, const float* pre, int64_t ld_pre, const float* c,
                                float* h_out, float* c_out, float* gates_out, int M, int D, void* ws,
                                size_t ws_bytes, void* stream);
int set_lstm_cell_bwd_f32(const float* dh, const float* dc, const float* gates, const float* c_prev,
                          const float* c_new, float* dgates, float* dc_prev, int M, int D, void* stream);
int set_copy_lstm_train_f32(const SetEditNetWeights* w, const float* x, int64_t ldx, int Kx,
                            const float* h2, const float* c2, const float* c_memory, float* h_out,
                            float* c_out, float* gates, float* c_new, float* cg, int M, int D, void* ws,
                            size_t ws_bytes, void* stream);
/* stage 1 of CopyLSTMCellC backward: du (copy-gate pre-activation grad), direct grads of c_memory and
 * c_new, o-gate pre-activation grad; stage 2 (after dcn += du W_n) is set_lstm_gates_bwd_f32 */
int set_copy_gate_bwd_f32(const float* dh, const float* dadp, const float* ogate, const float* adp,
                          const float* cg, const float* cmem, const float* c_new, float* du,
                          float* dcm_direct, float* dcn_direct, float* do_pre, int M, int D, void* stream);
/* the same with the o-gate read in place from the saved (M,4D) gate block: ogate = gates + 3D, ld_ogate = 4D */
int set_copy_gate_bwd_ld_f32(const float* dh, const float* dadp, const float* ogate, int64_t ld_ogate,
                             const float* adp, const float* cg, const float* cmem, const float* c_new, float* du,
                             float* dcm_direct, float* dcn_direct, float* do_pre, int M, int D, void* stream);
int set_lstm_gates_bwd_f32(const float* dcn, const float* do_pre, const float* gates, const float* c_prev,
                           float* dgates, float* dc_prev, int M, int D, void* stream);
int set_caption_attention_train_f32(const SetEditNetWeights* w, const float* H, const float* att1_c,
                                    const float* h1, const float* word, const float* mask, float* gated,
                                    float* alpha_c, float* ctx, float* zt, float* s, float* t, int M, int T,
                                    int Dh, int D, int A, void* ws, size_t ws_bytes, void* stream);
int set_context_gate_bwd_f32(const float* dout, const float* zt, const float* s, const float* t, float* dz,
                             float* ds, float* dt, int M, int D, void* stream);
/* the same with a common row stride ld_out >= D for dz / ds / dt: the three can then be column blocks of one (M, 3D) buffer
 * whose products with stacked weight blocks are single contractions */
int set_context_gate_bwd_ld_f32(const float* dout, const float* zt, const float* s, const float* t, float* dz,
                                float* ds, float* dt, int64_t ld_out, int M, int D, void* stream);
/* additive-attention backward (use_tanh=1: caption attention, 0: visual attention with ReLU).
 * values (M,L,Dv) are the attended rows (H or X); att2 (M,A) includes the decoder-projection bias.
 * Outputs datt1 (M,L,A), datt2 (M,A), dwfull_part (M,A; sum over M = d full_att.weight),
 * dvalues (M,L,Dv) or NULL, de (M,L) or NULL (sum = d full_att.bias). */
int set_attention_bwd_f32(const float* dctx, const float* dalpha_ext, const float* alpha,
                          const float* values, const float* att1, const float* att2, const float* w_full,
                          float* datt1, float* datt2, float* dwfull_part, float* dvalues, float* de, int M,
                          int L, int Dv, int A, int use_tanh, void* stream);
/* Caption-encoder recurrence of the grad-enabled path (CaptionEncoderC editnet.py:333-338; the packed BiLSTM of
 * dcnet.py:233), one step for all rows with the length handling inside the kernels: rows with t < lens[b] advance, the
 * others carry (h, c) and emit zeros.  xg = hoisted input projection x W_x^T + b_x, element (b, t, :) at
 * xg + b ld_xg_row + t ld_xg_t.  train: h_out / c_out (B,D) new state, H / Mem (Mem may be NULL) row (b, t) at
 * b ld_out_b + t ld_out_t + out_col0, Hprev (same layout, may be NULL) receives h (the state the step started from, the
 * operand of dW_hh), gates (B,4D) post-activations.  bwd: dH / dM (same layout as H / Mem, may be NULL) + dh / dc
 * (B,D, may be NULL) -> dgates rows (b, :) at dgates + b ld_dg (pre-activation gradients = gradient of xg[b,t,:]),
 * dc_prev (B,D) and dh_pass (B,D): the caller adds dgates W_hh to dh_pass to obtain dh of the previous step. */
size_t set_encoder_cell_workspace_bytes(int B, int D);
int set_encoder_cell_train_f32(const float* xg, int64_t ld_xg_row, int64_t ld_xg_t, const float* h, const float* c,
                               const float* w_hh, const float* b_hh, const int64_t* lens, int t, float* h_out, float* c_out,
                               float* H, float* Mem, float* Hprev, int64_t ld_out_b, int64_t ld_out_t, int out_col0,
                               float* gates, int B, int D, void* ws, size_t ws_bytes, void* stream);
int set_encoder_cell_bwd_f32(const float* dh, const float* dc, const float* dH, const float* dM, int64_t ld_d_b,
                             int64_t ld_d_t, int d_col0, const int64_t* lens, int t, const float* gates,
                             const float* c_prev, const float* c_new, float* dgates, int64_t ld_dg, float* dc_prev,
                             float* dh_pass, int B, int D, void* stream);
int set_select_bwd_f32(const float* dsel, const float* Mem, const float* alpha, float* dM, float* dalpha,
                       int M, int T, int D, void* stream);
/* The attention block of one training timestep (editnet.py:534-540) in four launches: the decoder-side projections of
 * both attentions and the [word,h1] parts of tc_affine / context_gate as one grouped GEMM, both attention roles +
 * SelectC as one kernel, the context side of the gate, its pointwise.  att1_c (M,T,A) = cap_features_att(H),
 * att1 (M,R,A) = features_att(att_embed(X)) (this step's, with its dropout), rmask (M,R) or NULL.  Outputs: gated (M,D)
 * = attend_cap, alpha_c (M,T), ctx (M,D) = sum_t alpha_t H_t, zt / s / t (M,D) the gate's factors (for the backward),
 * sel (M,D), attend_img (M,F), alpha_v (M,R); att2_c_out / att2_v_out (M,A) or NULL: the decoder-side projections incl.
 * bias exactly as scored (what set_attention_bwd_f32 takes as `att2`: the backward need not recompute them). */
size_t set_editnet_attentions_workspace_bytes(int M, int D, int A);
int set_editnet_attentions_train_f32(const SetEditNetWeights* w, const float* H, const float* att1_c,
                                     const float* mask, const float* Mem, const float* X, const float* att1,
                                     const float* rmask, const float* h1, const float* word, float* gated,
                                     float* alpha_c, float* ctx, float* zt, float* s, float* t, float* sel,
                                     float* attend_img, float* alpha_v, float* att2_c_out, float* att2_v_out, int M,
                                     int T, int R, int F, int D, int A, void* ws, size_t ws_bytes, void* stream);
/* Accumulating forms used by the whole-sequence training node (xe_sequence.py): gradients of loop-invariant operands
 * (H, Mem, cap_features_att(H), and features_att(att_embed(X)) in eval mode) are summed over the timesteps in place
 * instead of by one tensor-sized add per timestep.  acc_* = 1: `out += contribution`, rows beyond M are not touched.
 * ld_datt2 (>= A, 0 = A): row stride of datt2, so that the two attentions of a step can write the halves of one
 * (M, 2A) buffer whose product with the stacked decoder projections is ONE contraction.
 * select: with acc_dM only the selected row of dM changes (dalpha is always overwritten). */
int set_attention_bwd_acc_f32(const float* dctx, const float* dalpha_ext, const float* alpha,
                              const float* values, const float* att1, const float* att2, const float* w_full,
                              float* datt1, float* datt2, float* dwfull_part, float* dvalues, float* de, int M,
                              int L, int Dv, int A, int use_tanh, int acc_datt1, int acc_dvalues, int64_t ld_datt2,
                              void* stream);
/* dvalues[b, l, :] (+)= sum_t alpha[t, b, l] dctx[t, b, :] over per-sequence logs alpha (T,B,L), dctx (T,B,Dv), T <= 64:
 * the attended rows' gradient of all timesteps in one pass. */
int set_attention_dvalues_f32(const float* alpha, const float* dctx, float* dvalues, int T, int B, int L, int Dv,
                              int accumulate, void* stream);
int set_select_bwd_acc_f32(const float* dsel, const float* Mem, const float* alpha, float* dM, float* dalpha,
                           int M, int T, int D, int acc_dM, void* stream);
/* nn.Dropout(p) in training mode (editnet.py:299-302, :441, :546) with the library's Philox4x32-10 generator:
 * y[r, c] = x[r, c] / (1 - p) with probability 1 - p, else 0; one uniform per element from counter
 * (r, c / 4, offset) and key seed, so a (seed, offset) pair reproduces the mask.  x == y (in place) is allowed.
 * backward: dx (+)= dy * (y != 0 ? scale : 0) with y the forward OUTPUT (scale = 1 / (1 - p)); on the two sites that
 * follow a ReLU this also applies the ReLU's derivative (scale = 1 in eval mode = plain ReLU backward).
 * cols, all leading dimensions: multiples of 4; pointers 16-byte aligned. */
int set_dropout_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int cols, float p, uint64_t seed,
                    uint64_t offset, void* stream);
/* set_dropout_f32 of ONE operand for `steps` timesteps in one launch: y + t * y_step = dropout(x) drawn at offset + t
 * (t = 0 .. steps - 1), bit for bit what `steps` calls write.  The per-timestep region dropout of the train-mode forward
 * (editnet.py:441: `att_embed`'s nn.Dropout sees the same relu(W X) with a fresh mask every timestep) is the caller. */
int set_dropout_steps_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t y_step, int rows, int cols, int steps,
                          float p, uint64_t seed, uint64_t offset, void* stream);
/* its backward over all timesteps: dx (+)= sum_t dy[t] * (y[t] != 0 ? scale : 0), t ascending — what `steps` accumulating
 * calls of set_dropout_bwd_f32 leave in dx, bit for bit */
int set_dropout_bwd_steps_f32(const float* dy, int64_t lddy, int64_t dy_step, const float* y, int64_t ldy, int64_t y_step,
                              float* dx, int64_t ldx, int rows, int cols, int steps, float scale, int accumulate,
                              void* stream);
/* EmbeddingC.forward in train mode (editnet.py:299-302) in one launch: set_embed_relu_f32 followed by set_dropout_f32
 * in place (the same counters, hence the same mask for a (seed, offset) pair) */
int set_embed_relu_dropout_f32(const float* table, const int64_t* ids, int64_t ids_stride, float* out, int64_t ldo,
                               int n, int D, int V, float p, uint64_t seed, uint64_t offset, void* stream);
int set_dropout_bwd_f32(const float* dy, int64_t lddy, const float* y, int64_t ldy, float* dx, int64_t ldx, int rows,
                        int cols, float scale, int accumulate, void* stream);
/* backward of set_dropout_f32 with the keep mask regenerated from (seed, offset): dx (+)= dy * keep / (1 - p).  For the
 * site that does not follow a ReLU (h2 before fc, editnet.py:545), where an exactly-zero kept input must still pass its
 * gradient — nn.Dropout's backward multiplies by the mask, not by the output's zero pattern. */
int set_dropout_bwd_philox_f32(const float* dy, int64_t lddy, float* dx, int64_t ldx, int rows, int cols, float p,
                               uint64_t seed, uint64_t offset, int accumulate, void* stream);
/* out[c] (+)= sum_r x[r, c] (bias gradients over all (t, b) rows): two deterministic passes through a workspace of
 * set_colsum_workspace_bytes(cols); cols, ld multiples of 4. */
size_t set_colsum_workspace_bytes(int cols);
int set_colsum_f32(const float* x, int64_t ld, int rows, int cols, float* out, int accumulate, void* ws,
                   size_t ws_bytes, void* stream);
/* Several column sums as ONE pair of launches (the ~16 bias gradients of a training step; reference: autograd's per-bias
 * sum over (t, b) of every nn.Linear / nn.LSTMCell bias, editnet.py:223-560): out (+)= colsum(x), and out2 (+)= the same sums
 * when non-NULL (two biases fed by the same gradient: LSTMCell's bias_ih / bias_hh).  Deterministic (no atomics);
 * n <= SET_COLSUM_MAX; cols, ld multiples of 4; ws of set_colsum_group_workspace_bytes(d, n). */
#define SET_COLSUM_MAX 24
typedef struct SetColsumDesc {
    const float* x; int64_t ld; int rows; int cols;
    float* out; int accumulate;
    float* out2; int accumulate2;
} SetColsumDesc;
size_t set_colsum_group_workspace_bytes(const SetColsumDesc* d, int n);
int set_colsum_group_f32(const SetColsumDesc* d, int n, void* ws, size_t ws_bytes, void* stream);
/* mask[r] = (sum_c x[r, c] != 0) as 0/1 floats: the data-derived region mask of the adaptive model
 * (adaptive_features/editnet_adaptive.py:449-453) on the per-step, dropped-out region embedding. */
int set_rowsum_mask_f32(const float* x, int64_t ld, int rows, int cols, float* mask, void* stream);
/* dst[:, :] (+)= [src0 | src1 | ...] column blocks (1..4 segments, cols[i] floats wide, row stride ld[i]): builds the
 * concatenated LSTM input rows of editnet.py:523 / :541 inside the per-sequence operand logs (no torch.cat). */
int set_pack_f32(float* dst, int64_t ldd, int rows, int nseg, const float* const* src, const int64_t* ld,
                 const int* cols, int accumulate, void* stream);

/* Multinomial sampling epilogue of one free-running step as an operator (the grad-enabled SCST rollout,
 * editnet_rl.py:521-543 / dcnet_rl.py:320-340): replaces exp -> torch.multinomial -> gather -> <end> rewrite ->
 * `unfinished` latch -> seq store -> `unfinished.sum() == 0` host check.  logits (B,V) include the bias.
 * State owned by the caller across the steps of one rollout: it (B) int64, unfinished (B) int32,
 * alive (max_len+2) int32 (all initialised here at t == 0); call with t = 0,1,2,... in order.
 * Outputs of the step: seq[:,t] (seq (B,max_len) pre-zeroed), it = next input token, raw_ids (B) = the sampled
 * word before the <end> rewrite or -1 once every row had finished at an earlier step (the reference's `break`),
 * lse (B) = logsumexp(logits), step_logp (B) = log_softmax(logits)[raw_id] (0 after the break).
 * RNG: Philox4x32-10, counter (row, t, offset), key seed. */
int set_sample_pick_f32(const float* logits, int64_t ld_logits, int B, int V, int t, int max_len, int64_t end_idx,
                        uint64_t seed, uint64_t offset, int64_t* seq, int64_t* it, int32_t* unfinished,
                        int32_t* alive, int64_t* raw_ids, float* lse, float* step_logp, void* stream);
/* set_sample_pick_f32 with options (SetSampleOpts, above set_editnet_sample_opts) */
int set_sample_pick_opts_f32(const float* logits, int64_t ld_logits, int B, int V, int t, int max_len, int64_t end_idx,
                             uint64_t seed, uint64_t offset, int64_t* seq, int64_t* it, int32_t* unfinished,
                             int32_t* alive, int64_t* raw_ids, float* lse, float* step_logp, void* stream,
                             const SetSampleOpts* opts);
/* set_sample_pick_opts_f32 that also records the kept set: kept_key (B) uint32, may be NULL.  Row b's kept set is
 * {v : order_key(y[v]) >= kept_key[b]}, y = fl32(logits * (1.0f / temperature)) and order_key the order-preserving key of a float
 * (u = bits of f; 0x80000000 for -0.0; ~u when the sign bit is set, u | 0x80000000 otherwise): the threshold the kernel found
 * after its "arg-max is always kept" clamp, 0 when nothing is cut (top_k off or >= V, top_p == 1) and with neutral or NULL opts.
 * Every other output is that of set_sample_pick_opts_f32 bit for bit; refusals are the same. */
int set_sample_pick_opts_key_f32(const float* logits, int64_t ld_logits, int B, int V, int t, int max_len, int64_t end_idx,
                                 uint64_t seed, uint64_t offset, int64_t* seq, int64_t* it, int32_t* unfinished,
                                 int32_t* alive, int64_t* raw_ids, float* lse, float* step_logp, void* stream,
                                 const SetSampleOpts* opts, uint32_t* kept_key);
/* backward of step_logp w.r.t. logits: dlogits[b,v] = g[b] (1[v == raw_id_b] - exp(logits[b,v] - lse[b])); rows
 * with raw_id < 0 get zeros */
int set_sample_logp_bwd_f32(const float* logits, int64_t ld_logits, const float* lse, const int64_t* raw_ids,
                            const float* g, float* dlogits, int64_t ld_dlogits, int B, int V, void* stream);
/* backward of the step_logp of set_sample_pick_opts_key_f32 (the log-prob under the distribution sampled from), for `rows` rows
 * in ONE launch (a rollout's (T, B) logs are T * B rows): with inv_t = 1.0f / temperature, y = fl32(logits[r,v] * inv_t),
 *     dlogits[r,v] = g[r] * inv_t * (1[v == raw_id_r] - (order_key(y) >= kept_key[r] ? exp(y - lse[r]) : 0)).
 * The kept set is piecewise constant in the logits and is held constant; y is the rounded product the forward compared, so words
 * outside the set get exactly 0.  Rows with raw_id < 0 get zeros.  kept_key NULL: every word is kept; opts NULL: neutral — with
 * both the values are those of set_sample_logp_bwd_f32 bit for bit.  Rows are read and written 16 bytes at a time when
 * ld_logits and ld_dlogits are multiples of 4 and both bases are 16-byte aligned, by scalar accesses otherwise; columns
 * V .. ld_dlogits-1 are not written.  SET_ERR_ARG (before any HIP call, nothing written) for a NULL pointer other than
 * kept_key / opts, rows <= 0, V <= 0, a leading dimension below V and for options set_sample_pick_opts_f32 refuses. */
int set_sample_logp_bwd_opts_f32(const float* logits, int64_t ld_logits, const float* lse, const int64_t* raw_ids,
                                 const uint32_t* kept_key, const float* g, float* dlogits, int64_t ld_dlogits, int rows, int V,
                                 const SetSampleOpts* opts, void* stream);
/* the device RNG itself (tests: known-answer vectors): out (n,4) uint32 = Philox4x32-10(counter (i,0,offset), key seed) */
int set_philox4x32(uint32_t* out, int n, uint64_t seed, uint64_t offset, void* stream);
/* The Gumbel-max pick of one timestep (the contract above set_editnet_sample_gumbel): the arguments, outputs and bookkeeping
 * of set_sample_pick_opts_f32 — one workgroup per row, t = 0 initialises it / unfinished / alive — with the word drawn as the
 * first maximum of y + g.  opts carries the temperature only (NULL: 1); top_k != 0 or top_p != 1 answers SET_ERR_ARG. */
int set_gumbel_pick_f32(const float* logits, int64_t ld_logits, int B, int V, int t, int max_len, int64_t end_idx,
                        uint64_t seed, uint64_t offset, int64_t* seq, int64_t* it, int32_t* unfinished, int32_t* alive,
                        int64_t* raw_ids, float* lse, float* step_logp, void* stream, const SetSampleOpts* opts);
/* out (rows, V) fp32 = the noise g[v] of (seed, offset, row, t, v) of that contract, row = 0 .. rows - 1: the test hook of the
 * noise, as set_philox4x32 is of the raw generator.  SET_ERR_ARG: NULL out, rows / V <= 0, t outside [0, 255], V > 2^26 - 4. */
int set_gumbel_fill_f32(float* out, int rows, int V, int t, uint64_t seed, uint64_t offset, void* stream);

/* The vocabulary-row epilogue of one free-running timestep (csrc/epilogue.hip greedy_pick_k / sample_pick_k) with every
 * argument the decode loops give it, for direct tests: one workgroup per row turns
 *     logit[b, v] = sum over slabs s < n of logits[s * stride + b * ld + v]  (+ bias[v]),  v < V
 * into the row's word (greedy: first index of the maximum; sample: inverse CDF of one Philox uniform per (seed, offset, b, t)),
 * does the bookkeeping of editnet_rl.py:529-547 (<end> -> 0, `unfinished` latch, seq / seq_logp[:, t] while t < max_len and
 * alive[t - 1] != 0, alive[t] += rows still unfinished, it = next input word), gathers emb_out[b] = relu(table[it[b]])
 * (table (>= V, D), emb_out (B, D); skipped when either is NULL) and, with `tail`, finishes the NEXT timestep's LSTM cell of
 * the row: gates = g0 slabs (in index order) + pre + tab[it, col0 .. col0 + 4D), order i, f, g, o; c_out = f c_in + i g,
 * h_out = o tanh(c_out); c_in may be c_out.
 * The caller owns the state: it, unfinished (B), alive (> t entries, alive[t] zero before the call) are NOT initialised here.
 * The row-limit override of set_decode_row_limits applies to the greedy mode as it does inside the decode loops; the sample
 * mode has no row limit (sample_pick takes none, in the rollout neither).  `stride` is taken as given: with n > 1 the caller
 * keeps the slabs apart (stride >= B * ld); it is not checked.
 *   SET_ERR_ARG          a NULL args / logits / seq / it / unfinished / alive (greedy: seq_logp too), mode not 0 / 1, B, V,
 *                        n, max_len <= 0, t < 0, ld < V, and a tail that is not laid out as the kernels read it (tail D <= 0
 *                        or not a multiple of 4, a NULL or not 16-byte-aligned g0 / tab / c_in / c_out / h_out, g0_n < 1,
 *                        g0_ld / g0_stride / ld_tab / col0 / ldpre not multiples of 4, nrows <= 0, misaligned pre)
 *   SET_ERR_UNSUPPORTED  D not a multiple of 4
 * Every refusal is answered before any HIP call and nothing is written.  Rows of up to 12288 words whose ld and stride are
 * multiples of 4 floats on a 16-byte-aligned base are read once as float4 into registers; any other row takes the
 * scalar kernels.  raw_ids / lse / step_logp (sample mode; each may be NULL) as set_sample_pick_f32. */
#define SET_PICK_GREEDY 0
#define SET_PICK_SAMPLE 1
typedef struct SetPickTail {
    const float* g0; int64_t g0_stride, g0_ld;   /* gate pre-activation partials (rows, 4 D), g0_n slabs */
    const float* pre; int64_t ldpre;             /* (rows, ldpre) or NULL */
    const float* tab; int64_t ld_tab;            /* token table (nrows, ld_tab) */
    const float* c_in; float* c_out; float* h_out;   /* (rows, D) */
    int32_t g0_n, col0, nrows, D;
} SetPickTail;
typedef struct SetPickArgs {
    const float* logits; int64_t ld, stride;
    const float* bias;                           /* V floats or NULL */
    int64_t end_idx;
    int64_t* seq; float* seq_logp;               /* (B, max_len) */
    int64_t* it; int32_t* unfinished; int32_t* alive;
    const float* table; float* emb_out;
    uint64_t seed, offset;                       /* sample mode */
    int64_t* raw_ids; float* lse; float* step_logp;
    const SetPickTail* tail;                     /* or NULL */
    int32_t n, B, V, t, max_len, D, mode, pad_;
} SetPickArgs;
int set_pick_slabs_f32(const SetPickArgs* args, void* stream);
/* the same with SetSampleOpts in sample mode (see set_sample_pick_opts_f32).  The greedy mode takes no options: non-NULL
 * opts that are not neutral give SET_ERR_ARG there. */
int set_pick_slabs_opts_f32(const SetPickArgs* args, const SetSampleOpts* opts, void* stream);

/* Beam-search step epilogue for NI images x k hypotheses (rows i*k+j), replacing the host bookkeeping of
 * editnet.py:654-699 / dcnet.py:450-500 / eval_full.py:150-200: log_softmax (or, with logits2, the ensemble
 * log((softmax(logits)+softmax(logits2))/2)), + running scores, flat top-k over k*V per image (ties: lowest
 * flat index), parent/word split, completed-hypothesis tracking (best completed score, first maximum),
 * k_left -= #<end>, live hypotheses compacted to the front, sequences re-indexed and extended
 * (seqs_in -> seqs_out, cur_len valid tokens -> cur_len+1), next input `words`, and `rows` = the parent
 * row of every hypothesis row for set_beam_gather_f32.  k <= 8.  Step 1 is expressed by the caller through
 * scores = {0, -inf, ...}.  Images with k_left == 0 are left untouched. */
int set_beam_pick_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                      int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in,
                      int64_t* seqs_out, float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words,
                      int32_t* rows, void* stream);
/* set_beam_pick_f32 plus the N-BEST list of every image: done_score (NI, k), done_seq (NI, k, Lmax), done_len (NI, k) and
 * n_done (NI), which the caller zero-fills before step 1 (n_done) and hands to every step.  Every COUNTED <end> pick (one among
 * the first k_left picks of its image) appends one entry at index n_done[i]: its value, its cur_len + 1 tokens and that length.
 * COMPLETION ORDER: by step and, within a step, by pick rank (value descending, flat index ascending among equals).  An image
 * completes at most k hypotheses, so the arrays have room for all of them; entries past n_done[i] are never written.  Images
 * with k_left == 0 are left untouched.  Every other output holds the same bytes as after set_beam_pick_f32.  SET_ERR_ARG also
 * for a NULL done_* array; the other refusals are those of set_beam_pick_f32. */
int set_beam_pick_nbest_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                            int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in,
                            int64_t* seqs_out, float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words,
                            int32_t* rows, float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done,
                            void* stream);
/* In-place re-index of up to four (NI*k, D) recurrent-state tensors by `rows` (editnet.py:687-696). */
int set_beam_gather_f32(float* s0, float* s1, float* s2, float* s3, const int32_t* rows, int NI, int k, int D,
                        void* stream);

/* Constrained beam-search pick (csrc/beam_constrained.hip): the step of set_beam_pick_nbest_f32 — same arguments up to n_done,
 * same state, done_* mandatory — with candidates REMOVED before the flat top-k and completed hypotheses ranked by a
 * length-normalised score.  Nothing is renormalised: a surviving candidate (j, v) keeps the value scores[j] + logp_j[v].
 * With s[0 .. L-1] the L = cur_len tokens of slot j (s[0] = <start>), candidate (j, v) is removed if
 *   a. v is one of the n_banned ids of `banned` (device memory; an id outside [0, V) matches nothing), or
 *   b. v == end_idx and L - 1 < min_len (L - 1 words have been generated so far), or
 *   c. no_repeat_ngram = n >= 1, L >= n and some i in 1 .. L - n has s[i .. i+n-2] == s[L-n+1 .. L-1] and s[i+n-1] == v
 *      (<start> at position 0 never takes part; n = 1: no word twice).
 * The k largest surviving values (ties: lowest flat index j V + v) are the picks; the first k_left count; parent / word split,
 * shrinking k, compaction, words, rows and the sequence re-index are those of set_beam_pick_f32.  A counted <end> pick of value x
 * completes a hypothesis of cur_len generated words whose RANK SCORE is r = x for length_alpha == 0 (no division: bit-equal) and
 * r = x / powf(cur_len, length_alpha) otherwise: best_score and done_score hold r, the best of a pick is the first maximum of r in
 * pick order and replaces best_* only when strictly greater.  The running `scores` stay raw sums.
 * An image with k_left > 0 and NO surviving finite candidate ends there: k_left = 0, scores = -inf, words = 0, rows = identity,
 * best_* / done_* as they stood, seqs_out not written (as for a finished image).
 * Neutral constraints {0, 0, 0, 0, NULL}: the integer outputs of set_beam_pick_nbest_f32; floats agree to rounding (another
 * summation order of the log-sum-exp).  The outputs do not depend on the row layout (float4 reads for ld % 4 == 0, 16-byte
 * aligned rows and V <= 12288; scalar reads otherwise).
 * ws: set_beam_pick_constrained_workspace_bytes(NI, k) bytes (0 for NI <= 0 or k outside 1 .. 8), 16-byte aligned.
 * All before any HIP call — SET_ERR_ARG: a NULL pointer (c, ws and the done_* arrays included), ws misaligned or too small,
 * no_repeat_ngram outside 0 .. 16, min_len < 0, length_alpha negative or not finite, n_banned outside 0 .. 64 or banned == NULL
 * with n_banned > 0 (or the reverse), and what set_beam_pick_f32 refuses; SET_ERR_UNSUPPORTED: k > 8, k V >= 2^31 - 1, Lmax > 256. */
typedef struct SetBeamConstraints {
    int32_t no_repeat_ngram;      /* 0 = off, 1..16 */
    int32_t min_len;              /* 0 = off */
    float   length_alpha;         /* 0 = off, finite, >= 0 */
    int32_t n_banned;             /* 0..64 */
    const int64_t* banned;        /* device, n_banned ids; NULL iff n_banned == 0 */
} SetBeamConstraints;
size_t set_beam_pick_constrained_workspace_bytes(int NI, int k);
int set_beam_pick_constrained_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                                  int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in,
                                  int64_t* seqs_out, float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words,
                                  int32_t* rows, float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done,
                                  const SetBeamConstraints* c, void* ws, size_t ws_bytes, void* stream);

/* Diverse (group) beam-search pick (Vijayakumar et al., "Diverse Beam Search"; csrc/beam_constrained.hip bd_merge_k): the step of
 * set_beam_pick_constrained_f32 — same arguments up to n_done, same constraints c (non-NULL, a neutral struct allowed), same
 * limits — with the k slots of an image in `groups` = G groups of g = k / G: group gi owns slots gi g .. gi g + g - 1 and is a
 * beam search of its own over them.  g_left (NI, G) is the group's k_left (g at the start of a search, when only the first slot
 * of every group is alive: score 0, the others -inf); k_left[img] is kept as the sum of the image's g_left.
 * The groups of an image pick in order gi = 0 .. G - 1.  A candidate (j, v) of group gi — slot j of the group with a finite score,
 * v not removed by c — has the value x = scores[j] + logp_j[v] and the KEY y = x - penalty n(v) (float32), n(v) = how many
 * counted picks of groups 0 .. gi - 1 of this image at this step have the word v.  <end> is exempt: never penalised, an <end>
 * pick is never counted.  The group's picks are its g best candidates by y descending, then flat index j V + v ascending (j the
 * slot index within the image); the first g_left[gi] count.  The value carried forward, and ranked by x / cur_len^alpha when the
 * pick completes a hypothesis, is x, NOT y: scores stay sums of the model's log-probabilities.  Within a group the bookkeeping
 * is that of set_beam_pick_constrained_f32 (live picks first, the other slots die, parent and child in one group); best_* is the
 * first maximum of r over all groups in group order, then pick rank; done_* is appended in that order and done_group (NI, k)
 * records each completion's group (at most k hypotheses complete per image).
 * A group with g_left > 0 and no surviving finite candidate ends: g_left = 0, its scores = -inf, words = 0, rows = identity, its
 * sequences not written.  A group that had ended before the step gets rows = identity and words = 0 and nothing else; a finished
 * image (k_left <= 0) is left untouched as by set_beam_pick_constrained_f32.
 * groups == 1 (g_left = k_left): the outputs of set_beam_pick_constrained_f32 byte for byte, done_group = 0.
 * ws: set_beam_pick_diverse_workspace_bytes(NI, k) bytes (0 for NI <= 0 or k outside 1 .. 8), 16-byte aligned.
 * All before any HIP call — SET_ERR_ARG: what set_beam_pick_constrained_f32 answers with it, a NULL done_group or g_left,
 * groups < 1, k % groups != 0, a penalty that is negative or not finite; SET_ERR_UNSUPPORTED: as set_beam_pick_constrained_f32. */
size_t set_beam_pick_diverse_workspace_bytes(int NI, int k);
int set_beam_pick_diverse_f32(const float* logits, const float* logits2, int64_t ld, int NI, int k, int V, int64_t end_idx,
                              int cur_len, int Lmax, float* scores, int32_t* k_left, const int64_t* seqs_in,
                              int64_t* seqs_out, float* best_score, int64_t* best_seq, int32_t* best_len, int64_t* words,
                              int32_t* rows, float* done_score, int64_t* done_seq, int32_t* done_len, int32_t* n_done,
                              int32_t* done_group, int32_t* g_left, int groups, float penalty,
                              const SetBeamConstraints* c, void* ws, size_t ws_bytes, void* stream);

/* Constrained greedy and sampled picks (csrc/epilogue.hip, the CONS instantiations of greedy_pick_k / sample_pick_k; the ban list:
 * csrc/row_pick.h): the rules a-c of set_beam_pick_constrained_f32 in the two free-running decode modes.  The pick of row b at
 * timestep t is THE PICK OF THAT MODE APPLIED TO THE ROW WITH THE REMOVED WORDS AT -inf: arg-max and its first-index tie rule,
 * temperature, the top-k / top-p kept set, the inverse-CDF draw, lse, step_logp and seq_logp all see the masked row, so the
 * log-probabilities are those of the constrained, renormalised distribution (the one a sample is drawn from; beam search does
 * not renormalise and stays as it is).  With s[0] = <start>, s[1 .. t] = seq[b, 0 .. t-1] and L = t + 1, word v is removed if
 *   a. v is one of the n_banned ids of `banned` (device memory; an id outside [0, V) matches nothing), or
 *   b. v == end_idx and t < min_len, or
 *   c. no_repeat_ngram = n >= 1, L >= n and some i in 1 .. L - n has s[i .. i+n-2] == s[L-n+1 .. L-1] and s[i+n-1] == v
 *      (<start> at position 0 never takes part, so it is never read; n = 1: no word twice).
 * A row that has already finished (t > 0 and unfinished[b] == 0) gets exactly what the unconstrained pick gives it.  The
 * <end> -> 0 rewrite, the `unfinished` latch, alive, raw_ids, the embedding gather, the LSTM tail, the greedy row-limit override
 * (set_decode_row_limits) and the loop gate are unchanged.  One workgroup per row builds the row's list in LDS (at most 64 + 1 +
 * 255 entries) and applies it as the row is read: no extra launch, nothing written into the logits, no scratch.  Both row
 * layouts of set_pick_slabs_f32 are covered and give the same outputs.  Neutral constraints {0, 0, 0, 0, NULL} give the bits of
 * the unconstrained pick.
 * SET_ERR_ARG, before any HIP call and with nothing written: c == NULL, no_repeat_ngram outside 0 .. 16, min_len < 0, n_banned
 * outside 0 .. 64, banned == NULL with n_banned > 0 (or the reverse), length_alpha != 0 (nothing is ranked here), max_len > 255
 * (the row's history lives in LDS), V <= n_banned + 1 + max_len (so that, by counting, every row keeps at least one word: there
 * is no "row ran out of candidates" case), and whatever the unconstrained entry refuses.
 *
 * set_pick_slabs_constrained_f32: set_pick_slabs_opts_f32 with constraints — one pick on the arguments of the decode loops; the
 * history is args->seq[:, :t], so also SET_ERR_ARG for t > max_len.  opts may be NULL; in greedy mode it must be neutral.
 * Float64 restatement: tests/pick_constrained_oracle.py. */
int set_pick_slabs_constrained_f32(const SetPickArgs* args, const SetSampleOpts* opts, const SetBeamConstraints* c, void* stream);
/* The free-running loops under constraints: the arguments of set_editnet_greedy / set_editnet_sample_opts / set_dcnet_greedy /
 * set_dcnet_sample_opts plus c, applied at every timestep.  These entries ALWAYS run on the per-step kernels, wherever the
 * unconstrained loop runs — small batches (never the persistent launch), adaptive features, and the split-precision GEMM route
 * of a greedy decode from 65 rows on (set_editnet_greedy; the split changes the GEMMs only) — with the LSTM tail inside the
 * pick as in the unconstrained per-step loop.  A neutral c gives the bits of that per-step loop.  Refusals: those above (max_len
 * is the loop's) and those of the unconstrained entry, all before anything is touched. */
int set_editnet_greedy_constrained(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                                   const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                                   int64_t start_idx, int64_t end_idx, int max_len, int64_t* seq,
                                   float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                                   const SetBeamConstraints* c);
int set_editnet_sample_constrained(const SetEditNetWeights* w, const SetEditNetDims* d, const float* X,
                                   const float* image_mean, const int64_t* prev, const int64_t* prevlen,
                                   int64_t start_idx, int64_t end_idx, int max_len, uint64_t seed, uint64_t offset,
                                   int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                                   const SetSampleOpts* opts, const SetBeamConstraints* c);
int set_dcnet_greedy_constrained(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                                 const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_len,
                                 int64_t* seq, float* seq_logp, void* ws, size_t ws_bytes, void* stream,
                                 const SetBeamConstraints* c);
int set_dcnet_sample_constrained(const SetDcnetWeights* w, const SetDcnetDims* d, const int64_t* prev,
                                 const int64_t* prevlen, int64_t start_idx, int64_t end_idx, int max_len,
                                 uint64_t seed, uint64_t offset, int64_t* seq, float* seq_logp, void* ws,
                                 size_t ws_bytes, void* stream, const SetSampleOpts* opts,
                                 const SetBeamConstraints* c);

/* Stochastic beam search pick (Kool, van Hoof, Welling, ICML 2019; csrc/sbs.hip): one timestep t (0-based, t <= 254) of a
 * search that leaves, per image, k <= 8 DISTINCT sequences which are an exact sample WITHOUT replacement from the model's
 * sequence distribution, in draw order.  NI images x k slots; slot j of image i is logits row r = i k + j.
 * Slot state (updated in place): phi (log-probability of the prefix), G (its perturbed log-probability; -inf = dead slot),
 * finished, len (tokens so far) and the tokens themselves, seqs (NI, k, Lmax), WITHOUT <start>, <end> stored as end_idx.
 * Before step 0 the caller sets, per image, slot 0 to phi = G = 0 and every other slot to G = -inf, finished = len = 0 and
 * n_open = 1.
 *   live, unfinished slot j:
 *     y[v]    = fl32(x[v] * (1.0f / temperature))                 (the product rounded, as in the Gumbel-max draw)
 *     phi'[v] = phi_j + (y[v] - logsumexp(y))
 *     g[v]    = phi'[v] + noise(seed, offset, r, t, v)            (the noise of the Gumbel-max draw above, csrc/philox.h)
 *     Z       = max_v g[v]
 *     u       = (G_j - g[v]) + log(1 - exp(g[v] - Z))             (log(1 - exp(d)) as log(-expm1(d)) for d > -log 2, log1p(-exp(d))
 *     g~[v]   = G_j - max(u, 0) - log1p(exp(-|u|))                 otherwise)
 *     the first arg-max of g gets g~ = G_j exactly (u = -inf there); words with y = -inf are never candidates.
 *   finished slot j: ONE candidate, itself: g~ = G_j, phi and tokens unchanged, flat index j V + end_idx; its row is not read.
 *   pick: the k largest g~ over all candidates of the image, ties to the lowest flat index j V + v.  g~ is increasing in g for
 *     a fixed parent, so the candidates of a parent are its k best words by (g descending, v ascending).
 * Output slots are in pick order (slot 0 has the largest G).  Per output slot: phi, G, finished (parent finished, or word ==
 * end_idx), len, the tokens re-indexed by parent and extended (seqs_in -> seqs_out; entries past len are not written),
 * words = the next input word (0 for a finished or dead slot) and rows = the parent row for set_beam_gather_f32 (the slot's
 * own row for a finished parent and for a dead slot).  Fewer than k finite candidates leave dead slots (G = phi = -inf, len 0).
 * n_open (NI) = the live unfinished slots after the pick.  An image with n_open == 0 on entry is a no-op: state untouched,
 * words = 0, rows = identity, and its k Lmax tokens are copied from seqs_in to seqs_out so that the caller's buffer swap holds.
 * Two launches (one workgroup per row, then one wave per image); rows of up to 12288 words with ld % 4 == 0 on a 16-byte-
 * aligned base are read once as float4 into registers, any other row by scalar reads (three sweeps over the row: callers pad
 * the leading dimension, as evaluate.sample_captions_distinct does); the outputs do not depend on the path.
 * ws: set_sbs_workspace_bytes(NI, k) bytes (0 for NI <= 0 or k outside 1 .. 8), 16-byte aligned.
 * SET_ERR_ARG (before any HIP call, nothing written): a NULL args or pointer field, NI <= 0, k outside 1 .. 8, V <= 0, t outside
 * 0 .. 254, V > 2^26 - 4, ld < V, end_idx outside 0 .. V - 1 (<end> is a word of the vocabulary), Lmax < t + 1, seqs_in ==
 * seqs_out, a workspace that is too small or misaligned, options
 * set_sample_pick_opts_f32 refuses, top_k != 0, top_p != 1 (opts carries the temperature only; NULL: 1).
 * Float64 restatement: tests/sbs_oracle.py. */
typedef struct SetSbsArgs {
    const float* logits; int64_t ld;             /* (NI k, ld) */
    int64_t end_idx;
    uint64_t seed, offset;
    float* phi; float* G; int32_t* finished; int32_t* len;      /* (NI, k) */
    const int64_t* seqs_in; int64_t* seqs_out;   /* (NI, k, Lmax) */
    int64_t* words; int32_t* rows;               /* (NI k) */
    int32_t* n_open;                             /* (NI) */
    void* ws; size_t ws_bytes;
    int32_t NI, k, V, t, Lmax, pad_;
} SetSbsArgs;
size_t set_sbs_workspace_bytes(int NI, int k);
int set_sbs_pick_f32(const SetSbsArgs* args, const SetSampleOpts* opts, void* stream);
/* The same pick for the ENSEMBLE of two models that step on the same words (evaluate.sample_captions_distinct_ensemble; the
 * beam searches' log((softmax_e + softmax_d) / 2), eval_full.py:151-153).  logits2 (NI k, ld): the second model's rows, with
 * args->ld and args->V.  Each model is tempered on its own, BEFORE the average:
 *     y_e[v] = fl32(x_e[v] * (1.0f / temperature)),  y_d[v] likewise from logits2
 *     p = y_e[v] - logsumexp(y_e),  q = y_d[v] - logsumexp(y_d)          (each log-sum-exp formed as the one-model pick forms its own)
 *     l[v]    = log(0.5 (exp(p) + exp(q))) = hi + log1p(exp(lo - hi)) - ln 2,  hi = max(p, q), lo = min(p, q)
 *     phi'[v] = phi_j + l[v],   g[v] = phi'[v] + noise(seed, offset, r, t, v)
 * and everything from Z on as above.  A word that is -inf in ONE model is a candidate with l = hi - ln 2; a word that is -inf in
 * both never is.  The averaged probabilities are a distribution over the words, so the result is the exact sample without
 * replacement from the ensemble's sequence distribution.  A word's noise is that of the one-model pick: it does not depend on
 * the number of models.  Semantics, refusals, state, outputs and workspace (set_sbs_workspace_bytes) are those of
 * set_sbs_pick_f32; the register path also needs logits2 16-byte aligned and holds both rows; SET_ERR_ARG for a NULL logits2.
 * Profile scopes sbs_rows_ens / sbs_rows_ens_scalar, then sbs_merge.  Float64 restatement: tests/sbs_oracle.py on
 * L = log(0.5 (softmax(y_e) + softmax(y_d))) (tests/sbs_ensemble_fixtures.py). */
int set_sbs_pick_ensemble_f32(const SetSbsArgs* args, const float* logits2, const SetSampleOpts* opts, void* stream);
/* Both picks under TRUNCATION: opts carries temperature, top_k and top_p (SetSampleOpts; validated as set_sample_pick_opts_f32
 * validates them; top_k >= V is off).  Every step's WORD distribution is cut to a kept set S and renormalised over it, which is
 * still a distribution over the words: the top-down construction applies unchanged and the k sequences are the exact sample
 * without replacement from the truncated model q.  phi is log q(prefix): the log-probability under the truncated, tempered model.
 * The kept set of a live unfinished row, on z[v] (below), by the rules of the truncated sampled pick (SetSampleOpts above):
 *   top-k (off at 0 or >= V): every word with z >= the top_k-th largest z, that value's ties all included;
 *   top-p (off at 1), over what top-k kept: value groups in descending order until their mass sum exp(z - max z) reaches
 *     top_p M (M: the mass of what top-k kept), the crossing group included whole;
 *   the arg-max is always kept; comparisons are on values (-0.0 and +0.0 are one group).
 * The mass of a candidate threshold is summed in one fixed order (per thread in enumeration order, a tree over the wave, waves in
 * index order); a target closer to a group boundary than float32 summation resolves may fall on either side.
 *   set_sbs_pick_opts_f32 (one model): z = y = fl32(x * (1.0f / temperature)).  Words outside S are -inf: never candidates.
 *     phi'[v] = phi_j + (y[v] - logsumexp over S of y), the log-sum-exp formed as the untruncated pick forms its own.
 *   set_sbs_pick_ensemble_opts_f32: the truncation applies to the ENSEMBLE's word distribution, not to each model.  Each model is
 *     tempered and normalised on its own over the whole vocabulary and l[v] is formed as above; z = l;
 *     phi'[v] = phi_j + (l[v] - L_S),   L_S = max l + log(sum over S of exp(l - max l)).
 * g, Z, g~, the pick and every output are as above with phi' so defined; a word's noise does not depend on the options.  Fewer than
 * k words in S leave dead slots, as fewer than k finite candidates do (top_k = 1: one live slot per image, phi = G = 0).
 * NULL opts, or top_k off and top_p == 1: the untruncated kernel, state and outputs byte for byte those of set_sbs_pick_f32 /
 * set_sbs_pick_ensemble_f32.  Refusals (SET_ERR_ARG before any HIP call, nothing written): those of the entries above except
 * that top_k > 0 and top_p in (0, 1) are taken; top_k < 0, top_p outside (0, 1] or not finite, a temperature outside 1e-3 .. 1e3.
 * Workspace: set_sbs_workspace_bytes, unchanged.  Both row-read paths give the same bytes; on the scalar path every pass of the
 * bitwise descent (32 for top-k, 33 for top-p) re-reads the row, so callers pad the leading dimension.  Profile scopes
 * sbs_rows_trunc / sbs_rows_trunc_scalar and sbs_rows_ens_trunc / sbs_rows_ens_trunc_scalar (the untruncated scopes when nothing
 * is cut), then sbs_merge.  Float64 restatement: tests/sbs_trunc_oracle.py. */
int set_sbs_pick_opts_f32(const SetSbsArgs* args, const SetSampleOpts* opts, void* stream);
int set_sbs_pick_ensemble_opts_f32(const SetSbsArgs* args, const float* logits2, const SetSampleOpts* opts, void* stream);

/* General-layout fp32 GEMM on the MFMA pipe, used for the Linear backward (replaces the cuBLAS calls
 * autograd makes for nn.Linear / nn.LSTMCell: dX = dY.W and dW += dY^T.X):
 *     C[m,n] (+)= sum_k a(m,k) * b(n,k)
 *     a(m,k) = a_kminor ? A[k*lda + m] : A[m*lda + k];   b(n,k) = b_kminor ? B[k*ldb + n] : B[n*ldb + k]
 * accumulate != 0 adds into C (in-place .grad accumulation).  `ws` is scratch for split-K slabs (may be
 * NULL: the contraction is then never split).  Leading dimensions are multiples of 4 floats; a k-minor
 * operand needs its own dimension (M or N) to be a multiple of 4 — for A, alternatively rows that are readable up
 * to the next multiple of 4 (lda >= round_up(M,4); output rows >= M are never stored) —; a k-major one needs
 * K % 4 == 0, or rows that are zero-padded by the caller up to the next multiple of 4 (leading dimension >=
 * round_up(K,4)). */
int set_gemm_f32(const float* A, long long lda, int a_kminor, const float* B, long long ldb, int b_kminor,
                 float* C, long long ldc, int M, int N, int K, int accumulate, void* ws, size_t ws_bytes,
                 void* stream);
/* Up to 6 independent problems of the same operand layout in one launch (the dX products of one module's
 * backward share dY and are individually too small to fill the chip).  Outputs must not alias each other. */
typedef struct SetGemmDesc {
    const float* A; long long lda;
    const float* B; long long ldb;
    float* C; long long ldc;
    int M, N, K, accumulate;
} SetGemmDesc;
int set_gemm_group_f32(const SetGemmDesc* descs, int n, int a_kminor, int b_kminor, void* ws, size_t ws_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Split-K partials handed to their consumer instead of being reduced by a launch of their own (round 5; the XE / SCST
 * backward of xe_sequence.py: 130 reduction launches of ~5 us per training step disappear).  A SetSlabSrc describes one
 * addend of a (rows, N) gradient: value(m, j) = sum_{s < nslab} p[s * slab_stride + m * ld + j] for m < rows, 0 for the rows
 * beyond (a sequence that had left the batch when the product ran).  Sums run in slab order, then in list order:
 * deterministic.
 * set_gemm_group_slabs_f32 = set_gemm_group_f32 without its reduction: problem i's partials stay in `ws` and out[i]
 * describes them (nslab >= 2); a problem the plan does not split is written to descs[i].C as usual (accumulate honoured)
 * and out[i].nslab = 0.  The caller keeps `ws` untouched until every consumer has run.
 * The *_src entry points are the backward kernels of the decode step with such lists as (part of) their gradient input:
 * gradient = base (may be NULL) + the listed addends.
 * ------------------------------------------------------------------------------------------ */
typedef struct SetSlabSrc {
    const float* p;
    int64_t slab_stride;     /* floats between two partials */
    int64_t ld;              /* floats between two rows */
    int32_t nslab;           /* 0: this entry contributes nothing */
    int32_t rows;            /* rows the partials hold */
} SetSlabSrc;
#define SET_MAX_SRC 4
int set_gemm_group_slabs_f32(const SetGemmDesc* descs, int n, int a_kminor, int b_kminor, void* ws, size_t ws_bytes,
                             SetSlabSrc* out, void* stream);
/* set_lstm_cell_bwd_f32 with dh = the listed addends (n_dh <= SET_MAX_SRC; 0: dh = 0) */
int set_lstm_cell_bwd_src_f32(const SetSlabSrc* dh_src, int n_dh, const float* dc, const float* gates, const float* c_prev,
                              const float* c_new, float* dgates, float* dc_prev, int M, int D, void* stream);
/* set_copy_gate_bwd_ld_f32 with dh = the listed addends + the backward of the output dropout (editnet.py:545) of dh_drop
 * (M, D; may be NULL): dh_drop * keep / (1 - p) with the keep mask regenerated from (seed, offset) as
 * set_dropout_bwd_philox_f32 does; p = 0: dh_drop is added as it is (eval mode). */
int set_copy_gate_bwd_src_f32(const SetSlabSrc* dh_src, int n_dh, const float* dh_drop, int64_t ld_drop, float p, uint64_t seed,
                              uint64_t offset, const float* dadp, const float* ogate, int64_t ld_ogate, const float* adp,
                              const float* cg, const float* cmem, const float* c_new, float* du, float* dcm_direct,
                              float* dcn_direct, float* do_pre, int M, int D, void* stream);
/* set_lstm_gates_bwd_f32 / set_select_bwd_acc_f32 / set_context_gate_bwd_ld_f32 / set_attention_bwd_acc_f32 with their
 * gradient input = base (NULL allowed where noted) + the listed addends.  set_attention_bwd_src_f32 also stores the gradient
 * it summed to dctx_out (M, Dv) when that is not NULL (the caption context's gradient is needed again after the loop). */
int set_lstm_gates_bwd_src_f32(const float* dcn_base, const SetSlabSrc* src, int n_src, const float* do_pre, const float* gates,
                               const float* c_prev, float* dgates, float* dc_prev, int M, int D, void* stream);
int set_select_bwd_src_f32(const float* dsel_base, const SetSlabSrc* src, int n_src, const float* Mem, const float* alpha,
                           float* dM, float* dalpha, int M, int T, int D, int acc_dM, void* stream);
int set_context_gate_bwd_src_f32(const float* dout_base /* may be NULL */, const SetSlabSrc* src, int n_src, const float* zt,
                                 const float* s, const float* t, float* dz, float* ds, float* dt, int64_t ld_out, int M, int D,
                                 void* stream);
int set_attention_bwd_src_f32(const float* dctx_base /* may be NULL */, const SetSlabSrc* src, int n_src, float* dctx_out,
                              const float* dalpha_ext, const float* alpha, const float* values, const float* att1,
                              const float* att2, const float* w_full, float* datt1, float* datt2, float* dwfull_part,
                              float* de, int M, int L, int Dv, int A, int use_tanh, int acc_datt1, int64_t ld_datt2,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * The timestep loops of the XE / SCST training node as ONE call each (csrc/train_loop.hip): the loop bodies of
 * editnet.py:505-546 (train mode, teacher-forced, fixed-36 features) and of autograd's BPTT over them, i.e. exactly the
 * sequence of entry points above that show-edit-tell_amd/xe_sequence.py issues per timestep, with the per-sequence logs
 * addressed as base + t * (rows of one timestep).  Issued from Python the ~45 launches per timestep cost more host time than
 * their kernels take (16.3 ms of enqueue for a 16.0-ms step at B = 128).  All pointers are device pointers except `bts`
 * (host: rows still in the batch at every timestep, editnet.py:506) and `w`.  Logs are (T, B, .) row-major, the state logs
 * H1 / C1 / H2 / C2 (T + 1, B, D) with slot t = the state BEFORE timestep t.
 * ------------------------------------------------------------------------------------------ */
typedef struct SetXELoopArgs {
    int T, B, R, F, Tc, D, A, V, train;
    float p_embed, p_out;
    uint64_t seed, off_embed, off_out;           /* Philox: timestep t of a site draws at off_* + t */
    const int* bts;
    const SetEditNetWeights* w;
    const float *E, *al_wih, *al_whh;
    const int64_t* tok; int64_t tok_step, tok_stride;      /* word of (t, b) = tok[t * tok_step + b * tok_stride] */
    const float *X, *H, *Mem, *mask, *att1_c, *pre1, *att1; int64_t att1_step;
    float *EMB, *H1, *C1, *H2, *C2, *G1, *G2, *WHC, *ZT, *S, *TT, *ALPHAC, *ALPHAV, *ATT2C, *ATT2V, *SEL, *CNEW, *CG, *X2, *H2D;
    float *gated, *cx, *aimg;                    /* (B, D), (B, D), (B, F) scratch — or (T, B, .) logs, see step_logs */
    void* ws_l; size_t ws_l_bytes;               /* set_lstm_cell_workspace_bytes */
    void* ws_c; size_t ws_c_bytes;               /* set_editnet_attentions_workspace_bytes */
    void* ws_k; size_t ws_k_bytes;               /* set_copy_lstm_workspace_bytes */
    int step_logs;                               /* 1: gated / cx / aimg hold every timestep; the copy cell contracts its input
                                                    as the segments [h1 | gated | attend_img] where they lie and X2 / WHC are
                                                    packed ONCE after the loop (0: one packing launch per timestep) */
    const float* rmask; int64_t rmask_step;      /* adaptive features (editnet_adaptive.py:449-453): 0/1 region mask (B, R) of
                                                    timestep t at rmask + t * rmask_step, or NULL (fixed-36 features) */
} SetXELoopArgs;
int set_editnet_xe_train_loop_f32(const SetXELoopArgs* a, void* stream);

typedef struct SetXEBwdLoopArgs {
    int T, B, R, F, Tc, D, A, acc_datt1;
    float p_out;                                 /* 0: eval mode (no output dropout) */
    uint64_t seed, off_out;
    const int* bts;
    const float *cl_cnew_w, *cl_cmem_w, *cl_x2h_w, *cl_h2h_w, *w_ctx, *w_h1, *dec_cat, *al_wih, *al_whh, *va_full, *ca_full;
    const float *G1, *G2, *C1, *C2, *CG, *SEL, *CNEW, *ZT, *S, *TT, *ALPHAC, *ALPHAV, *ATT2C, *ATT2V, *X, *H, *Mem, *att1_c, *att1;
    int64_t att1_step;
    const float* dH2D;                           /* (T, B, D) gradient of fc's input */
    float *DU, *DGW, *DSZT, *DATT2, *DWFC, *DWFV, *DEC, *DEV, *DCTX, *DG1, *datt1; int64_t datt1_step;
    float *datt1c, *dMem;
    float *DC1[2], *DC2[2], *dcm, *dcn, *dop, *dalc;
    void* slab_ws[5]; size_t slab_ws_bytes;      /* one scratch region per product position of a timestep */
    float* tmp[11];                              /* (B, N) landing buffers of products the plan does not split */
    const float* DLAST;                          /* (T, B, D) or NULL: gradient entering h2 of timestep t directly (adaptive
                                                    features: d decoder_last_hidden at every row's last timestep, zero elsewhere) */
} SetXEBwdLoopArgs;
int set_editnet_xe_train_bwd_loop_f32(const SetXEBwdLoopArgs* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Host-side CIDEr-D for the self-critical reward (HOST pointers, no stream: per-sample n-gram work that shards with
 * the batch; the reference calls an external Python scorer at editnet_rl.py:636).  Sentences are int64 token ids.
 * create: the document-frequency table of preprocess_rl.py:7-55 as n_entries n-grams (entry i = lens[i] <= 4 ids at
 * tokens[4 i ..]) with their document counts df[i]; ref_len = number of documents; n = 4, sigma = 6 for CIDEr-D.
 * score: hypothesis i = hyp_tokens[hyp_off[i] .. hyp_off[i+1]) against reference set set_of_hyp[i]; set s = references
 * [ref_set_off[s], ref_set_off[s+1]); reference r = ref_tokens[ref_off[r] .. ref_off[r+1]).  scores: n_hyp doubles.
 * ------------------------------------------------------------------------------------------ */
void* set_ciderd_create(const int64_t* tokens, const int32_t* lens, const double* df, int64_t n_entries, double ref_len,
                        int n, double sigma);
void set_ciderd_destroy(void* scorer);
int set_ciderd_score(void* scorer, const int64_t* hyp_tokens, const int64_t* hyp_off, int n_hyp,
                     const int32_t* set_of_hyp, const int64_t* ref_tokens, const int64_t* ref_off,
                     const int64_t* ref_set_off, int n_sets, double* scores);

/* ------------------------------------------------------------------------------------------
 * CIDEr-D on the DEVICE (csrc/ciderd_device.hip): the integer reward path of ciderd.py:211-250 / ciderd_host.hip:77-156 with
 * sentences, reference vectors and scores in device memory on `stream` and no host read, and the same kernel with candidates
 * as each other's references (evaluate.consensus_rerank).  Sentences are rows of int64 VOCABULARY ids (not interned ids), at
 * most 64 per sentence; an n-gram is packed like make_key(.., uint64_t*) of ciderd_host.hip:57-61 (id + 1 in 16-bit fields, 0 =
 * no gram), so every id must lie in [0, 65534).  All arithmetic is double; sums over the lanes of a wave are one fixed
 * butterfly, so a row's result does not depend on the launch it is part of.  No atomics; only the declared outputs are written.
 *
 * key: the packing, on the host (ciderd_host.hip:57-61): *key_out = sum (tokens[j] + 1) << 16 j, j < k.  SET_ERR_ARG: NULL, k
 *   outside 1 .. 4; SET_ERR_UNSUPPORTED: an id outside [0, 65534).
 * create (ciderd_host.hip:171-189, ciderd.py:70-97): HOST arrays in the format of set_ciderd_create, the tokens being
 *   vocabulary ids; builds a device table packed key -> document count (16-byte {key, count} slots, open addressing with linear
 *   probing, capacity = the power of two >= max(2, 2 n_entries)), copies it on `stream` and waits for the copy.  The handle
 *   comes back in *handle_out (NULL on failure).  SET_ERR_ARG: NULL handle_out / arrays, n outside 1 .. 4, ref_len or sigma not
 *   positive, n_entries < 0; SET_ERR_UNSUPPORTED: an id outside [0, 65534) — both before any HIP call.  Entries with a length
 *   outside 1 .. 4 are skipped; of a repeated gram the last count stands.  destroy frees the table (NULL: nothing).
 * create_corpus: the table of cocoEval's `CIDEr` — the same formula, with df and N taken from the reference sets of the corpus
 *   that is scored: df(g) = the number of SETS one of whose references holds g (once per set however often it occurs there),
 *   ref_len = n_sets, so log ref_len = log(n_sets).  The references are DEVICE arrays in the form vectorise and score take them:
 *   reference r = ref_tokens[r ld .. r ld + L) with length ref_lens[r] (or the 0 rule with ref_lens == NULL), set s = references
 *   [ref_set_off[s], ref_set_off[s + 1]) (device int64, n_sets + 1), max_set the caller's bound on a set's size.  The table has
 *   the layout create builds, capacity = the power of two >= max(2, 2 gram_bound); gram_bound is the caller's bound on the
 *   number of distinct grams, e.g. sum_r sum_{k < n} max(0, len_r - k) from the lengths it holds on the host.  Everything is
 *   enqueued on `stream` and nothing is read back: the table is cleared by a memset, then one wave per set enters its
 *   references' grams with a 64-bit compare-and-swap on a slot's key and a double atomic add of 1 on its count (exact: an
 *   integer below 2^53).  The slot of a key depends on the order of arrival, the map key -> count does not.  A set the host
 *   cannot check (offsets outside [0, n_refs] or decreasing, a set larger than max_set) and a reference with an id outside
 *   [0, 65534) contribute nothing (score answers such a set with NaN).  A gram that finds no slot because gram_bound was too
 *   small is dropped and counted.  The handle serves lookup, vectorise, score and destroy as one from create does.
 *   SET_ERR_ARG: NULL handle_out / ref_set_off (ref_tokens with n_refs > 0), n outside 1 .. 4, sigma not positive, n_sets < 1,
 *   n_refs, max_set or gram_bound < 0, L < 1, ld < L; SET_ERR_UNSUPPORTED: L > 64, gram_bound > 2^40 — before any HIP call.
 * dropped (for tests: it waits for `stream`): *dropped_out = the grams create_corpus dropped, 0 for a handle from create.
 *   SET_ERR_ARG: NULL handle / dropped_out.
 * lookup: df_out[i] = document count of the packed key keys[i] (device arrays of n), 0.0 for an absent key or key 0.
 * vec_bytes / vectorise (ciderd_host.hip:77-99): sentence i = tokens[i ld .. i ld + L) (device int64, ld >= L), its length
 *   lens[i] clamped to [0, L] (device int32), or with lens == NULL the decoder's rule of ciderd.py:222-224: cut after the first 0,
 *   the 0 itself stays, a row without 0 is taken whole.  One wave per sentence writes its record into vecs (vec_bytes(n_sent, L)
 *   bytes, 8 + 8 L words of 8 bytes per sentence): the norms of the orders 1 .. 4, the number of bigrams, the length, a flag "an
 *   id was outside [0, 65534)", then per order the L keys of the DISTINCT grams by first position (0 elsewhere) and their weights
 *   tf (log ref_len - log max(1, df)).  vec_bytes is 0 for n_sent < 0 or L outside 1 .. 64.  SET_ERR_ARG: NULL handle / tokens /
 *   vecs, n_sent < 0, L < 1, ld < L; SET_ERR_UNSUPPORTED: L > 64 — before any HIP call.
 * score (ciderd_host.hip:101-156): hypothesis i (rows of hyp_tokens as in vectorise, L and hyp_lens likewise) against the
 *   references of set set_of_hyp[i] (device int32) = records [ref_set_off[s], ref_set_off[s + 1]) (device int64, n_sets + 1) of
 *   ref_vecs, which vectorise wrote with L = ref_L for n_refs sentences.  One wave per hypothesis:
 *     scores[i] = 10 / (n max(1, |set|)) sum_r sum_k  [sum_g min(g_h, g_r) g_r / (|g_h| |g_r|)]_k exp(-(l_h - l_r)^2 / 2 sigma^2)
 *   (the division only where both norms are non-zero, as on the host), and with pair_scores != NULL also
 *   pair_scores[i pair_ld + r] = the score against reference r of the set alone, r < |set|; nothing else is written.  max_set is
 *   the caller's bound on |set|.  What the host cannot check is answered by the kernel with NaN in scores[i] and nothing else
 *   touched: set_of_hyp[i] outside [0, n_sets), offsets outside [0, n_refs] or decreasing, a set larger than max_set.  An id
 *   outside [0, 65534) in the hypothesis or one of its references gives NaN in scores[i] (and in its pair_scores).
 *   SET_ERR_ARG: NULL handle / hyp_tokens / set_of_hyp / ref_set_off / scores (ref_vecs with n_refs > 0), a negative count, L or
 *   ref_L < 1, hyp_ld < L, pair_scores with pair_ld < max_set; SET_ERR_UNSUPPORTED: L or ref_L > 64 — before any HIP call and
 *   before the handle is read.
 * ------------------------------------------------------------------------------------------ */
int set_ciderd_device_key(const int64_t* tokens, int k, uint64_t* key_out);
int set_ciderd_device_create(const int64_t* tokens, const int32_t* lens, const double* df, int64_t n_entries, double ref_len,
                             int n, double sigma, void* stream, void** handle_out);
int set_ciderd_device_create_corpus(const int64_t* ref_tokens, int64_t ld, const int32_t* ref_lens, int64_t n_refs, int L,
                                    const int64_t* ref_set_off, int n_sets, int max_set, int64_t gram_bound,
                                    int n, double sigma, void* stream, void** handle_out);
int set_ciderd_device_dropped(void* handle, int64_t* dropped_out, void* stream);   /* tests only: synchronises */
void set_ciderd_device_destroy(void* handle);
int set_ciderd_device_lookup(void* handle, const uint64_t* keys, int64_t n, double* df_out, void* stream);
size_t set_ciderd_device_vec_bytes(int n_sent, int L);
int set_ciderd_device_vectorise(void* handle, const int64_t* tokens, int64_t ld, const int32_t* lens, int n_sent, int L,
                                void* vecs, void* stream);
int set_ciderd_device_score(void* handle, const int64_t* hyp_tokens, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L,
                            const int32_t* set_of_hyp, const void* ref_vecs, int ref_L, int64_t n_refs,
                            const int64_t* ref_set_off, int n_sets, int max_set, double* scores, double* pair_scores,
                            int64_t pair_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * BLEU on the DEVICE (csrc/bleu_device.hip): the statistics and scores of coco-caption's BleuScorer (n = 4, option "closest") as
 * bleu.py states them, from id rows in device memory on `stream` with no host read.  Sentences are rows of int64 vocabulary ids,
 * at most 64 per sentence, ids in [0, 65534) (the packing of set_ciderd_device_key).  Stateless: there is no handle.
 *   guess[k] = max(0, len - k + 1), correct[k] = sum over the distinct k-grams g of the hypothesis of min(count_h(g), max_r
 *   count_r(g)), testlen = len, reflen = the reference length that minimises (|len_r - len|, len_r);  with b the running product
 *   of (correct[k] + 1e-15) / (guess[k] + 1e-9): bleu[k] = b^(1/k), times exp(1 - 1/ratio) where ratio = (testlen + 1e-15) /
 *   (reflen + 1e-9) < 1.  The statistics are integers; the scores are double and a function of the row's integers alone, so a
 *   row's result does not depend on the launch it is part of.  No atomics; only the declared outputs are written.
 * ref_bytes / prepare: reference i = tokens[i ld .. i ld + L) (device int64, ld >= L), its length lens[i] clamped to [0, L]
 *   (device int32), or with lens == NULL the decoder's rule: cut after the first 0, the 0 itself stays, a row without 0 is taken
 *   whole.  One wave per reference writes its record into recs (ref_bytes(n_refs, L) bytes, 16-byte aligned; 8 + 4 L words of 8
 *   bytes per reference: the length, a flag "an id was outside [0, 65534)", six zero words, then per position the keys of the four
 *   grams that start there, 0 = none).  ref_bytes is 0 for n_refs < 0 or L outside 1 .. 64.  SET_ERR_ARG: NULL tokens / recs,
 *   n_refs < 0, L < 1, ld < L; SET_ERR_UNSUPPORTED: L > 64 — before any HIP call.  n_refs == 0: nothing is done.
 * score: hypothesis i (rows of hyp as in prepare, L and hyp_lens likewise) against the references of set set_of_hyp[i] (device
 *   int32) = records [ref_set_off[s], ref_set_off[s + 1]) (device int64, n_sets + 1) of ref_recs, which prepare wrote with
 *   L = ref_L for n_refs references.  One wave per hypothesis writes stats[i, 0..10) = correct[1..4], guess[1..4], testlen, reflen
 *   (int32), with scores != NULL scores[i, 0..4) = bleu[1..4] of the sentence, and with pair_scores != NULL
 *   pair_scores[i pair_ld + r] = the sentence's bleu[4] against reference r of its set alone, r < |set|; nothing else is written.
 *   An empty set gives correct = 0 and reflen = 0.  max_set is the caller's bound on |set|.  What the host cannot check is
 *   answered by the kernel with -1 in stats[i, :] and NaN in scores[i, :], nothing else touched: set_of_hyp[i] outside [0, n_sets),
 *   offsets outside [0, n_refs] or decreasing, a set larger than max_set.  An id outside [0, 65534) in the hypothesis or one of its
 *   references gives correct = -1 and NaN scores (and pair scores) in that row.
 *   SET_ERR_ARG: NULL hyp / set_of_hyp / ref_set_off / stats (ref_recs with n_refs > 0), a negative count, L or ref_L < 1,
 *   hyp_ld < L, pair_scores with pair_ld < max_set; SET_ERR_UNSUPPORTED: L or ref_L > 64 — before any HIP call.  n_hyp == 0: nothing
 *   is done.
 * ------------------------------------------------------------------------------------------ */
size_t set_bleu_device_ref_bytes(int n_refs, int L);
int set_bleu_device_prepare(const int64_t* tokens, int64_t ld, const int32_t* lens, int n_refs, int L, void* recs, void* stream);
int set_bleu_device_score(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L, const int32_t* set_of_hyp,
                          const void* ref_recs, int ref_L, int64_t n_refs, const int64_t* ref_set_off, int n_sets, int max_set,
                          int32_t* stats, double* scores, double* pair_scores, int64_t pair_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * ROUGE-L on the DEVICE (csrc/rouge_device.hip): the statistics and score of coco-caption's Rouge as rouge.py states them, from id
 * rows in device memory on `stream` with no host read.  Sentences and their limits are those of the BLEU block above, and the
 * references are ITS records: size them with set_bleu_device_ref_bytes, write them with set_bleu_device_prepare; one preparation
 * serves set_bleu_device_score and this entry.  Stateless: there is no handle.
 *   lcs(h, r) = the length of the longest common subsequence;  lcs_p = max_r lcs(h, r);  (lcs_r, len_r) = lcs and length of the
 *   reference with the largest recall lcs / len_r (compared exactly, as fractions; of equal recalls the first of the set; a
 *   reference of no ids is skipped, (0, 0) if all are empty);  P = lcs_p / len_h, Rc = lcs_r / len_r, and with both non-zero
 *   score = (1 + beta^2) P Rc / (Rc + beta^2 P), else 0 (coco: beta = 1.2).  The statistics are integers; the score is double, in
 *   this order of operations without contraction, and a function of the row's integers alone, so a row's result does not depend
 *   on the launch it is part of.  No atomics; only the declared outputs are written.
 * score: hypothesis i, reference sets, L, hyp_lens, ref_L, n_refs, ref_set_off, n_sets, max_set as in set_bleu_device_score.  One
 *   wave per hypothesis writes stats[i, 0..4) = lcs_p, len_h, lcs_r, len_r (int32), with scores != NULL scores[i], and with
 *   pair_scores != NULL pair_scores[i pair_ld + r] = the sentence's score against reference r of its set alone, r < |set|; nothing
 *   else is written.  An empty set gives 0, len_h, 0, 0 and the score 0.  What the host cannot check is answered by the kernel with
 *   -1 in stats[i, :] and NaN in scores[i], nothing else touched: set_of_hyp[i] outside [0, n_sets), offsets outside [0, n_refs]
 *   or decreasing, a set larger than max_set.  An id outside [0, 65534) in the hypothesis or one of its references gives -1 in
 *   stats[i, :] and a NaN score in that row (and NaN pair scores from the first such sentence on).
 *   SET_ERR_ARG: NULL stats, beta not finite or not positive, and what set_bleu_device_score refuses with it;
 *   SET_ERR_UNSUPPORTED: L or ref_L > 64 — before any HIP call.  n_hyp == 0: nothing is done.
 * ------------------------------------------------------------------------------------------ */
int set_rouge_device_score(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L, const int32_t* set_of_hyp,
                           const void* ref_recs, int ref_L, int64_t n_refs, const int64_t* ref_set_off, int n_sets, int max_set,
                           double beta, int32_t* stats, double* scores, double* pair_scores, int64_t pair_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * Word edit distance on the DEVICE (csrc/editdist_device.hip): the statistics, similarity and canonical word alignment that
 * editdist.py states, from id rows in device memory on `stream` with no host read.  Sentences and their limits are those of the
 * BLEU block above.  Stateless: there is no handle.
 *   d(h, r) = the unit-cost Levenshtein distance of the id sequences (substitution, insertion, deletion: 1 each);
 *   m = max(len_h, len_r);  sim(h, r) = (m - d) / m, one double division, and 1 when both are empty.  Of a set the reference of
 *   the largest sim is chosen (compared exactly, as fractions, empty against empty as 1/1; of equal ones the first of the set).
 *   The statistics are integers; the score is a function of the row's integers alone, so a row's result does not depend on the
 *   launch it is part of.  No atomics, no LDS; only the declared outputs are written.
 * score: hypothesis i, reference records (set_bleu_device_prepare's: one preparation serves BLEU, ROUGE-L and this entry), L,
 *   hyp_lens, ref_L, n_refs, ref_set_off, n_sets, max_set as in set_bleu_device_score.  One wave per hypothesis writes
 *   stats[i, 0..4) = dist, len_h, len_r, ref (int32; ref = the chosen reference's position in its set), with scores != NULL
 *   scores[i] = sim of those integers, and with pair_scores != NULL pair_scores[i pair_ld + r] = sim against reference r of its set
 *   alone, r < |set|; nothing else is written.  An empty set gives len_h, len_h, 0, -1 and the score of an empty reference.  What
 *   the host cannot check is answered by the kernel with -1 in stats[i, :] and NaN in scores[i], nothing else touched:
 *   set_of_hyp[i] outside [0, n_sets), offsets outside [0, n_refs] or decreasing, a set larger than max_set.  An id outside
 *   [0, 65534) in the hypothesis or one of its references gives -1 in stats[i, :] and a NaN score in that row (and NaN pair scores
 *   from the first such sentence on).
 *   SET_ERR_ARG: NULL stats, and what set_bleu_device_score refuses with it; SET_ERR_UNSUPPORTED: L or ref_L > 64 — before any HIP
 *   call.  n_hyp == 0: nothing is done.
 * align: the edit script that turns source row i (src[i src_ld .. i src_ld + src_L), src_lens as hyp_lens) into hypothesis row i
 *   (hyp, hyp_ld, hyp_lens, L), read off the full table D (rows: source, columns: hypothesis) from (len_s, len_h) backwards, at every
 *   cell the first rule that applies: keep (equal words, D equal on the diagonal), substitute (diagonal + 1), insert (left + 1),
 *   else delete.  One wave per row writes
 *     stats[i, 0..8)  = dist, len_h, len_s, keep, sub, ins, del, unchanged (1 when dist == 0)                  (int32)
 *     hyp_ops[i ops_ld + j], j < L       = 1 keep, 2 substitute, 3 insert, 0 at and beyond len_h                (int8)
 *     hyp_src[i ops_ld + j], j < L       = the aligned source position of a kept / substituted word, else -1    (int32)
 *     src_ops[i src_ops_ld + k], k < src_L = 1 kept, 2 substituted, 3 deleted, 0 at and beyond len_s            (int8)
 *   and nothing else.  An id outside [0, 65534) inside either sentence: stats[i, :] = -1, ops 0, hyp_src -1.
 *   SET_ERR_ARG: a NULL pointer other than the lengths (with n > 0), n < 0, L or src_L < 1, hyp_ld or ops_ld < L, src_ld or
 *   src_ops_ld < src_L; SET_ERR_UNSUPPORTED: L or src_L > 64 — before any HIP call.  n == 0: nothing is done.
 * ------------------------------------------------------------------------------------------ */
int set_edit_device_score(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n_hyp, int L, const int32_t* set_of_hyp,
                          const void* ref_recs, int ref_L, int64_t n_refs, const int64_t* ref_set_off, int n_sets, int max_set,
                          int32_t* stats, double* scores, double* pair_scores, int64_t pair_ld, void* stream);
int set_edit_device_align(const int64_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, int n, int L, const int64_t* src,
                          int64_t src_ld, const int32_t* src_lens, int src_L, int32_t* stats, int8_t* hyp_ops, int64_t ops_ld,
                          int32_t* hyp_src, int8_t* src_ops, int64_t src_ops_ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SET_HIP_H */
