/* speechsplit_amd.h -- C ABI of the MI355X (gfx950) SpeechSplit engine.
 *
 * The reference (biggytruck/SpeechSplit) is pure PyTorch and has no FFI of its own; the
 * boundary a maintainer binds is therefore derived from what its Python surface needs.  Each entry point names
 * the reference statement(s) it replaces.  Conventions:
 *   - plain C types only; every pointer marked "dev" is caller-owned device memory (e.g. tensor.data_ptr());
 *     the engine never frees caller memory and allocates nothing after ss_bind;
 *   - every call is asynchronous on the hipStream_t passed as `stream` (void*; NULL = default stream);
 *   - return value 0 = ok, negative = error, text via ss_last_error() (no C++ exceptions cross the ABI);
 *   - one engine per device per process; an engine is not thread-safe;
 *   - tensors are contiguous fp32, batch-first [B, T, C] exactly as the reference passes them (model.py:297,337);
 *   - T must be a multiple of the code down-sampling factor 8 (model.py:87,223-227) and <= max_frames, except in the
 *     eval-mode forwards (ss_g3_forward / ss_g6_forward with training == 0, ss_g3_rhythm), which take any T up to
 *     SS_MAX_EVAL_FRAMES whose plan (ss_plan_bytes) fits the bound workspace -- long utterances, as the reference runs them
 *     (InterpLnr is the identity in eval mode, model.py:382-383).  Everything that trains or differentiates (train-mode
 *     forwards, ss_*_backward*, ss_*_train_step, the data-parallel steps, SS_STEP_BUCKET, ss_interp_*) keeps T <= max_frames
 *     (<= 256) and refuses more up front, nothing enqueued, the engine usable afterwards.  That range, 8 <= T <= 256 in steps
 *     of 8, is tested end to end on the GPU: train steps, gradients and ss_interp_* at 8, 200 and 256 frames as well as at the
 *     64..192 frames of the benchmark configurations (tests/test_gpu_frame_range.py);
 *   - the random-resampling draws of InterpLnr (model.py:392-393 rand(B*7)+0.5; :399-402 randint) are INPUTS:
 *     `scales` f32 and `len_seg` i32, one [B*7] row per InterpLnr call in call order.  Given equal draws the
 *     index path is bit-exact against the reference;
 *   - what EVERY call that takes an engine refuses, in this order, each in a message that starts with the call's name, with nothing
 *     enqueued and no event recorded on any stream: (1) a NULL engine; (2) the wrong kind of engine -- ss_g3_* need a Generator_3,
 *     ss_g6_* a Generator_6, everything about parameters, gradients or the optimiser either of the two, ss_interp_* and the host
 *     getters any kind; the message names the kind the call needs and the kind the engine is; (3) an engine that is not bound as far
 *     as the call needs: the workspace, the gradient arena, and the Adam arenas wherever an optimiser step is part of the call
 *     (pass SS_STEP_NO_ADAM to go without); (4) a member of a data-parallel group where the call has no data-parallel form.  Then the
 *     call's own arguments -- NULL required pointers, B, T, flags outside the accepted set (every shape the planner would refuse is
 *     refused here, before the call touches a stream) -- and last the status word (ss_status) for the calls that consult it.  Three
 *     refusals come before (3): a bad argument of ss_set_grad_clip / ss_grad_norm / ss_grad_clip_stats, training != 0 with a length
 *     array, and "backward without a preceding forward" (ss_*_backward*).  With a NULL engine: ss_destroy is a no-op; ss_status and
 *     ss_grad_accum_count return 0 and ss_scratch_fallbacks -1 without a message; every other size or offset query returns -1 and
 *     every pointer-returning call NULL, with the message; ss_check and ss_clear_abort refuse before they synchronise.
 */
#ifndef SPEECHSPLIT_AMD_H
#define SPEECHSPLIT_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ss_engine ss_engine;

/* reference hparams.py:9-32 (only the values the hot path reads) */
typedef struct ss_hparams {
    int freq, dim_neck, freq_2, dim_neck_2, freq_3, dim_neck_3;
    int dim_enc, dim_enc_2, dim_enc_3, dim_freq, dim_spk_emb, dim_f0, chs_grp;
    int min_len_seg, max_len_seg, max_len_seq, max_len_pad;
} ss_hparams;

#define SS_GENERATOR_3 3 /* model.py:283 Generator_3 = Encoder_7 | Encoder_t | Decoder_3 */
#define SS_GENERATOR_6 6 /* model.py:324 Generator_6 = Encoder_t | Encoder_6 | Decoder_4 */
#define SS_INTERP_ONLY 0 /* model.py:355 a bare InterpLnr module: no parameters, ss_interp_* only (arenas may be NULL) */

#define SS_STEP_NO_ADAM 1 /* ss_*_train_step: stop after backward (data-parallel: all-reduce grads, then ss_adam_step) */
#define SS_STEP_SPLIT_BACKWARD 2 /* ss_g3_train_step: return once the head + decoder gradients (arena offsets >=
                                    ss_grad_split(), 80 % of the bytes, produced first) are complete, so their all-reduce
                                    overlaps the encoder backward that ss_train_finish() then enqueues */
#define SS_STEP_SPLIT_NO_JOIN 4 /* with SS_STEP_SPLIT_BACKWARD: do not make `stream` wait for the decoder's weight-gradient
                                    GEMMs (they run on an engine stream beside the encoder backward, as in the one-call
                                    step); the consumer of the decoder range orders itself with ss_wait_decoder_grads() */

#define SS_STEP_ACCUMULATE 8 /* ss_*_train_step and the data-parallel steps: this step's backward ADDS its parameter gradients to what the
                                gradient arena holds instead of starting from zeros; nothing else about the step changes (see "gradient
                                accumulation" below ss_zero_grads).  Composes with every other flag. */

#define SS_STEP_BUCKET 16 /* ss_*_train_step: T is the length bucket of THIS batch and the step runs with max_len_pad = T (what the
                             reference does when its hparams.max_len_pad is set to the bucket length: InterpLnr pads to it, the
                             encoders' len_org equals it, model.py:105,157,370).  T % 8 == 0, T <= max_frames.  A
                             bucket change re-plans the workspace (one memset, 0.1 - 0.2 ms at batch 64). */

#define SS_MAX_EVAL_FRAMES 8192 /* longest T an eval-mode forward accepts (131 s at a 16 ms hop) */

const char* ss_last_error(void);
int ss_abi_version(void);

/* model.py:285-295 / 327-334 (constructor).  No device memory is touched until ss_bind.  What each field of ss_hparams may be; anything
 * else returns NULL with an ss_last_error() that names the field and the accepted set, before anything is built (DESIGN.md section 1
 * has the audit behind every bound, tests/test_capi_hparams.py and tests/test_gpu_hparams.py a test at a non-default value of every free
 * field and a refusal test of every bound):
 *   dim_neck, dim_neck_2, dim_neck_3   free: each any of 1..32 (the reference takes any positive value; wider bottlenecks are refused).
 *   freq, freq_2, freq_3               free: may differ; every T must be a multiple of all three (checked per call).
 *   dim_enc, dim_enc_2, dim_enc_3      free: each a multiple of 64 in 64..1024 (the GroupNorm kernels work on 64-channel tiles).
 *   dim_freq                           free: a multiple of 4 in 32..512.  The mel slabs' rows are dim_freq floats apart and each tap of a
 *                                      layer-0 convolution reads dim_freq rounded up to 4 columns of them: another width would read past
 *                                      the rows, and behind the slab's last row past the slab.
 *   dim_spk_emb                        free: 1..1024, odd values included (one thread per column in the speaker-gradient kernel).
 *   dim_f0                             Generator_3: FIXED at 257 -- the training step quantises the resampled F0 itself into 256 bins plus
 *                                      unvoiced (utils.py:62-74).  Generator_6, which takes the one-hot and the target index as inputs:
 *                                      free in 32..512; target indices must lie in [0, dim_f0).
 *   chs_grp                            FIXED at 16.
 *   min_len_seg, max_len_seg           free: 1 <= min_len_seg < max_len_seg <= 32 (segment lengths are drawn from [min_len_seg,
 *                                      max_len_seg), model.py:399-402; a segment's 2 * max_len_seg candidate positions are the lanes of
 *                                      one wavefront).
 *   max_len_seq                        free: 1..512.  An utterance is resampled in S = max_len_seq / min_len_seg + 1 segments
 *                                      (model.py:365): every `[B*7]` below is [B*S], 7 at the defaults.
 *   max_len_pad                        free: 1..512; a training step runs with T == max_len_pad (or SS_STEP_BUCKET).
 * Wherever this header writes 80, 82, 257 or 337 for a tensor's last dimension it means dim_freq, dim_spk_emb, dim_f0 and
 * dim_freq + dim_f0.  max_batch >= 1, 8 <= max_frames <= 256.  The decoders' widths (512 / 256) are not in the struct. */
ss_engine* ss_create(int kind, const ss_hparams* hp, int max_batch, int max_frames);
void ss_destroy(ss_engine* e);

/* state_dict() table, reference key names and shapes, in parameters() order.
 * `offset` is in floats into each of the four arenas (params / grads / Adam m / Adam v). */
int ss_num_params(const ss_engine* e);
int ss_param_info(const ss_engine* e, int index, char* name, int name_cap, long* offset, int* ndim, long shape[3]);
long ss_arena_numel(const ss_engine* e);     /* floats per arena, alignment gaps included */
long ss_workspace_bytes(const ss_engine* e); /* activation workspace for (max_batch, max_frames) */
/* Workspace bytes an eval-mode forward of shape (B, T) needs (its activation plan plus the split-K scratch; host only, nothing
 * touched): 1 <= B <= max_batch, 8 <= T <= SS_MAX_EVAL_FRAMES, T a multiple of the code factors.  -1 (ss_last_error) otherwise.
 * ss_plan_bytes(e, max_batch, max_frames) == ss_workspace_bytes(e).  A bound workspace serves every (B, T) whose plan fits it:
 * a 16 x 192 Generator_3 workspace holds a 1 x 2000 forward. */
long ss_plan_bytes(const ss_engine* e, int B, int T);

/* .to(device) (solver.py:65): adopt caller-allocated device memory.  All four arenas hold ss_arena_numel floats.
 * The workspace is zero-filled here. */
int ss_bind(ss_engine* e, float* params_dev, float* grads_dev, float* adam_m_dev, float* adam_v_dev, void* workspace_dev,
            long workspace_bytes, void* stream);
/* Move a bound engine to another (larger) workspace, e.g. of ss_plan_bytes(e, B, T) bytes for a long eval-mode forward.  At least
 * ss_workspace_bytes(e) bytes, 256-byte aligned.  The Adam state (step count, hyper-parameters) carries across; the parameter,
 * gradient and Adam arenas stay where they are; the rest of the new workspace is zero-filled and the next call re-plans its shape.
 * Synchronises `stream` and the engine's own streams first: the old workspace is unused once the call returns. */
int ss_set_workspace(ss_engine* e, void* workspace_dev, long workspace_bytes, void* stream);

/* ---- Generator_3 (model.py:297-320) ---- */
/* G(x_f0, x_org, c_trg): x_f0 [B,T,337] = [mel 80 | f0 one-hot 257], x_org [B,T,80], c_trg [B,82] -> out [B,T,80].
 * training != 0 applies InterpLnr after each of the three encoder conv layers (model.py:203): scales/len_seg [3][B*7]. */
int ss_g3_forward(ss_engine* e, const float* x_f0_dev, const float* x_org_dev, const float* c_trg_dev,
                  const float* scales_dev, const int* len_seg_dev, int B, int T, int training, float* out_dev,
                  void* stream);
/* loss.backward() for the last ss_g3_forward: d_out [B,T,80] -> grads arena (overwritten, not accumulated). */
int ss_g3_backward(ss_engine* e, const float* d_out_dev, void* stream);
/* ss_g3_backward and, in the same call, the gradients w.r.t. the forward's INPUTS (what x_f0.grad / x_org.grad / c_trg.grad hold after
 * loss.backward() in the reference): dx_f0 [B,T,337] (80 mel columns, then the 257 one-hot columns), dx_org [B,T,80], dc_trg [B,82] --
 * caller-owned, dense, overwritten; B and T those of the last ss_g3_forward, training or eval mode alike (training: through each encoder
 * layer's resampling).  Every output pointer may be NULL; with all three NULL the call is ss_g3_backward, launch for launch.  The parameter
 * gradients are those of ss_g3_backward.  The input gradients come from the layer-0 convolutions' input-gradient GEMMs (on the streams of
 * their blocks, joined before the call returns) and one kernel that sums decoder layer 0's gate gradients over time and contracts them with
 * the speaker columns of W_ih (fixed-order fp32 sums).  Errors (nothing enqueued): a Generator_6 engine, no preceding forward. */
int ss_g3_backward_inputs(ss_engine* e, const float* d_out_dev, float* dx_f0_dev, float* dx_org_dev, float* dc_trg_dev, void* stream);
/* G.rhythm(x_org) (model.py:316-320): codes [B, T/8, 2] */
int ss_g3_rhythm(ss_engine* e, const float* x_org_dev, int B, int T, float* codes_dev, void* stream);

/* ---- Generator_6 (model.py:337-351) ---- */
/* P(x_org, f0_trg): x_org [B,T,80], f0_trg [B,T,257] -> logits [B,T,257]; training: scales/len_seg [3][B*7] (model.py:128) */
int ss_g6_forward(ss_engine* e, const float* x_org_dev, const float* f0_trg_dev, const float* scales_dev,
                  const int* len_seg_dev, int B, int T, int training, float* out_dev, void* stream);
int ss_g6_backward(ss_engine* e, const float* d_out_dev, void* stream);
/* ss_g6_backward and the input gradients dx_org [B,T,80], df0_trg [B,T,257] (dense, caller-owned, each may be NULL; all NULL: exactly
 * ss_g6_backward), as ss_g3_backward_inputs.  Errors (nothing enqueued): a Generator_3 engine, no preceding forward. */
int ss_g6_backward_inputs(ss_engine* e, const float* d_out_dev, float* dx_org_dev, float* df0_trg_dev, void* stream);

/* ---- ragged batches in eval mode (nothing to mirror: the reference converts one utterance per call, and padding a batch changes every
 *      row's result -- GroupNorm statistics, the reverse LSTM direction and the k=5 convolutions all look across time) ----
 * A ragged forward takes len i32[B] (caller-owned device memory, read by the kernels in stream order like every other input; it is not
 * copied into the workspace) next to the usual [B, T, C] inputs:
 *   - row b of the output, frames [0, len[b]), equals the eval-mode forward of that utterance alone at T = len[b], to the accuracy of any
 *     eval-mode forward; output frames t >= len[b] are exact zeros (ss_g3_rhythm_ragged: code rows >= len[b] / freq_2);
 *   - input frames t >= len[b] are never used: they may hold anything, NaN included;
 *   - len[b] is a multiple of every code factor (freq, freq_2, freq_3) and lies in [factor, T]; T obeys the rules of the eval-mode
 *     forwards (up to SS_MAX_EVAL_FRAMES, plan within the bound workspace).  Every kernel uses min(max(len[b], 0), T): a length outside
 *     the contract gives unspecified values in that row only, and nothing is read or written outside the tensors;
 *   - eval-mode only: training != 0 together with a length array is refused with nothing enqueued, and ss_*_backward* after a ragged
 *     forward is refused with the eval-only error a forward above max_frames gives; the engine stays usable;
 *   - len == NULL is exactly ss_g3_forward / ss_g6_forward (with NULL draws) / ss_g3_rhythm, launch for launch; with every len[b] == T the
 *     result is bit-identical to theirs (the predicates select nothing and the arithmetic is the same).
 * Where the lengths act: the staging of the inputs writes zeros behind each row's end; every GroupNorm takes its statistics over the row's
 * own frames (1 / (16 len[b])) and writes zeros behind them, which with the zero halo rows is the padding the next convolution sees in a
 * run of the utterance alone; every recurrence zeroes the state of a row at frames behind its end, so the reverse direction reaches the
 * row's last frame with the zero state; the copy of the head's output to the caller writes zeros there instead of the bias.  A batch
 * costs what its longest row costs: sort by length (speechsplit_amd.convert.plan_batches). */
int ss_g3_forward_ragged(ss_engine* e, const float* x_f0_dev, const float* x_org_dev, const float* c_trg_dev, const int* len_dev, int B,
                         int T, int training, float* out_dev, void* stream);
int ss_g3_rhythm_ragged(ss_engine* e, const float* x_org_dev, const int* len_dev, int B, int T, float* codes_dev, void* stream);
int ss_g6_forward_ragged(ss_engine* e, const float* x_org_dev, const float* f0_trg_dev, const int* len_dev, int B, int T, int training,
                         float* out_dev, void* stream);

/* ---- codes: the encoders alone, and the decoder on codes the caller supplies (eval mode only; nothing to mirror beyond model.py:84-87,
 *      194-229, 301-309: the reference only ever decodes what it has just encoded) ----
 * The model's product is its bottleneck codes -- content (codes_x), rhythm (codes_r), pitch (codes_f0) -- plus the speaker row.  These four
 * calls split an eval-mode forward at them, so that codes of different utterances can be recombined, edited, cached, or decoded for many
 * speakers from one encode.  Asynchronous on `stream` like their neighbours.
 *   - a code is dense, caller-owned fp32 [B, T / factor, 2 * dim_neck*]: cat(forward half of the encoder BLSTM's output sampled at the LAST
 *     frame of each block of `factor` frames, backward half at the FIRST), exactly what model.py:223-227 and :84-87 return.  Factors and
 *     widths: codes_x freq / dim_neck, codes_r freq_2 / dim_neck_2, codes_f0 freq_3 / dim_neck_3;
 *   - encode runs the encoders of an eval-mode forward and nothing behind them: no decoder recurrence, decoder projection or head launch
 *     (ss_profile counts none in SS_PROF_REC_FWD, SS_PROF_DEC_PROJ, SS_PROF_DEC_PROJ0, SS_PROF_HEAD).  One launch then writes every
 *     requested code; any output pointer may be NULL (that code is not written), all NULL is an error.  The codes are the bytes the
 *     forward's decoder-input assembly reads (ss_g3_encode's codes_r is ss_g3_rhythm's result bit for bit);
 *   - decode assembles the decoder input from the caller's codes and speaker rows c_trg [B, dim_spk_emb] (up-sampling every code by its
 *     factor, model.py:301-309 / 341-347), then runs the decoder BLSTM and the head exactly as the forward does, after the decoder's own
 *     weight preparation and the parameter guard.  No conv block, GroupNorm or encoder recurrence launch (none in SS_PROF_CONV_FWD,
 *     SS_PROF_GN, SS_PROF_ENC_REC).  decode(encode(x)) is bit-identical to the eval-mode forward of x at the same (B, T, len);
 *   - B and T obey the rules of the eval-mode forwards: 1 <= B <= max_batch, T a multiple of every code factor, up to SS_MAX_EVAL_FRAMES,
 *     plan within the bound workspace; ss_plan_bytes(e, B, T) is sufficient for both calls;
 *   - len_dev != NULL is a ragged batch under the length rules of ss_g3_forward_ragged.  encode never uses input frames t >= len[b] and
 *     writes exact zeros in code rows at or beyond len[b] / factor.  decode never reads code rows at or beyond len[b] / factor (they may
 *     hold anything, NaN included) and its output frames t >= len[b] are exact zeros.  With every len[b] == T the result is bit-identical
 *     to the dense call (len_dev == NULL);
 *   - afterwards no forward is left to differentiate: ss_*_backward* is refused with the "backward without a preceding forward" error,
 *     and the engine stays usable;
 *   - refused with nothing enqueued, in a message that names the call: the wrong kind of engine, an engine that is not bound, a NULL
 *     required pointer (every input, decode's out, all of encode's outputs), B or T outside the rules above. */
int ss_g3_encode(ss_engine* e, const float* x_f0_dev, const float* x_org_dev, const int* len_dev /* NULL: dense */, int B, int T,
                 float* codes_x_dev /* [B, T/freq, 2*dim_neck] or NULL */, float* codes_r_dev /* [B, T/freq_2, 2*dim_neck_2] or NULL */,
                 float* codes_f0_dev /* [B, T/freq_3, 2*dim_neck_3] or NULL */, void* stream);
int ss_g3_decode(ss_engine* e, const float* codes_x_dev, const float* codes_r_dev, const float* codes_f0_dev,
                 const float* c_trg_dev /* [B, dim_spk_emb] */, const int* len_dev /* NULL: dense */, int B, int T,
                 float* out_dev /* [B, T, dim_freq] */, void* stream);
/* Generator_6: codes_r (Encoder_t, freq_2 / dim_neck_2) and codes_f0 (Encoder_6, freq_3 / dim_neck_3); out [B, T, dim_f0] logits */
int ss_g6_encode(ss_engine* e, const float* x_org_dev, const float* f0_trg_dev, const int* len_dev, int B, int T, float* codes_r_dev,
                 float* codes_f0_dev, void* stream);
int ss_g6_decode(ss_engine* e, const float* codes_r_dev, const float* codes_f0_dev, const int* len_dev, int B, int T, float* out_dev,
                 void* stream);

/* ---- differentiable decode: train the decoder, the head and speaker rows on GIVEN codes, and gradients with respect to the codes ----
 * ss_*_decode above is forward only.  These calls run the same computation on a dense batch, keep its state, and differentiate it down to
 * the codes and the speaker rows -- with the encoders out of the picture: adapting to a new speaker from cached codes, code-space
 * optimisation, saliency per code.  Asynchronous on `stream` like their neighbours.
 *   - ss_g3_decode_train / ss_g6_decode_train: ss_*_decode's computation (same launches, same bits in out) under the rules of everything
 *     that differentiates: 1 <= B <= max_batch, T <= max_frames, T a multiple of every code factor, plan within the bound workspace.  No
 *     len_dev: ragged forwards have no backward.  Both precision modes.  out is required;
 *   - ss_g3_decode_backward / ss_g6_decode_backward: d_out [B, T, head width] is the gradient of the caller's loss with respect to out.
 *     Writes the gradient arena's decoder + head range [ss_grad_split(e), arena) and the status slot.  flags: 0 or SS_STEP_ACCUMULATE.
 *     Without SS_STEP_ACCUMULATE the WHOLE arena is cleared first, as every backward does, so the encoder range holds exact zeros; with
 *     it the gradients are added to what the arena holds and ss_grad_accum_count counts the call.  Any of d_codes_* and dc_trg may be NULL
 *     (not computed); all NULL gives parameter gradients only.  A code gradient is dense fp32 with the shape of its code: element
 *     [b][blk][c] is the sum of the decoder-input gradient over the block's `factor` frames, frames ascending, in one launch for all
 *     requested codes, without atomics (the same bits on every run).  dc_trg is [B, dim_spk_emb], per row and NOT summed over the batch,
 *     as ss_g3_backward_inputs returns it.  When the call returns (in stream order) the side stream's weight gradients are joined;
 *   - neither call launches a conv block, a GroupNorm, an encoder recurrence, an encoder BLSTM GEMM or an InterpLnr kernel (ss_profile
 *     counts none in SS_PROF_CONV_*, SS_PROF_GN, SS_PROF_ENC_REC, SS_PROF_ENC_LSTM, SS_PROF_WGRAD);
 *   - ss_adam_step_decoder: ss_adam_step restricted to [ss_grad_split(e), arena).  The encoder range of the parameters and of both
 *     moments keeps its bits; the step counter advances by one (a following ss_adam_step uses step + 1).  Clipping (ss_set_grad_clip),
 *     the non-finite skip and the status word act as for ss_adam_step; the norm is taken over the WHOLE arena as it stands (exact zeros in
 *     the encoder range after a non-accumulating decode backward);
 *   - ss_g3_decode_train_step: decode, MSE against target_mel [B, T, dim_freq] (mean, as ss_g3_train_step; loss: one device float), the
 *     backward, and ss_adam_step_decoder's update, in one call.  flags: SS_STEP_NO_ADAM (stop behind the backward) and / or
 *     SS_STEP_ACCUMULATE; every other flag is refused.  dc_trg (nullable) as above: what an optimiser over speaker rows needs;
 *   - state: after ss_*_decode_train only ss_*_decode_backward is valid -- ss_*_backward*, ss_train_finish are refused with a message that
 *     says the last forward was a decode.  ss_*_decode_backward is refused after a full forward, after a plain ss_*_decode / ss_*_encode
 *     and with no forward at all.  The engine stays usable after each refusal;
 *   - refused with nothing enqueued, in a message that names the call: the wrong kind of engine, an engine that is not bound, a NULL
 *     required pointer, B or T outside the rules above (T > max_frames included), flags outside the accepted set, a member of a
 *     data-parallel group (the data-parallel steps have no decode form). */
int ss_g3_decode_train(ss_engine* e, const float* codes_x_dev, const float* codes_r_dev, const float* codes_f0_dev,
                       const float* c_trg_dev /* [B, dim_spk_emb] */, int B, int T, float* out_dev /* [B, T, dim_freq] */, void* stream);
int ss_g3_decode_backward(ss_engine* e, const float* d_out_dev, float* d_codes_x_dev /* nullable */, float* d_codes_r_dev /* nullable */,
                          float* d_codes_f0_dev /* nullable */, float* dc_trg_dev /* [B, dim_spk_emb], nullable */, int flags, void* stream);
int ss_g6_decode_train(ss_engine* e, const float* codes_r_dev, const float* codes_f0_dev, int B, int T, float* out_dev /* [B, T, dim_f0] */,
                       void* stream);
int ss_g6_decode_backward(ss_engine* e, const float* d_out_dev, float* d_codes_r_dev /* nullable */, float* d_codes_f0_dev /* nullable */,
                          int flags, void* stream);
int ss_adam_step_decoder(ss_engine* e, float grad_scale, void* stream);
int ss_g3_decode_train_step(ss_engine* e, const float* codes_x_dev, const float* codes_r_dev, const float* codes_f0_dev, const float* c_trg_dev,
                            const float* target_mel_dev, int B, int T, float grad_scale, int flags, float* loss_dev,
                            float* dc_trg_dev /* nullable */, void* stream);

/* ---- Solver.train step body (solver.py:157-172), fused: cat(mel,f0) -> InterpLnr -> quantize_f0 -> G -> mse(mean)
 *      -> backward -> Adam.  mel [B,T,80], f0 [B,T,1] (-1e10 = unvoiced), emb [B,82], len_org i32[B];
 *      scales/len_seg [4][B*7] (outer call first).  T must equal hp.max_len_pad (model.py:105,157).
 *      grad_scale multiplies the gradients (1/world_size under data parallelism).  loss: one device float. */
int ss_g3_train_step(ss_engine* e, const float* mel_dev, const float* f0_dev, const float* emb_dev,
                     const int* len_org_dev, const float* scales_dev, const int* len_seg_dev, int B, int T,
                     float grad_scale, int flags, float* loss_dev, void* stream);
/* Generator_6 has no training loop in the reference; cross-entropy against target_idx i32[B,T] is this
 * engine's choice.  f0_onehot [B,T,257]; scales/len_seg [3][B*7]. */
int ss_g6_train_step(ss_engine* e, const float* mel_dev, const float* f0_onehot_dev, const int* target_idx_dev,
                     const float* scales_dev, const int* len_seg_dev, int B, int T, float grad_scale, int flags,
                     float* loss_dev, void* stream);

/* second half of a SS_STEP_SPLIT_BACKWARD step: encoder backward (+ Adam unless SS_STEP_NO_ADAM) */
int ss_train_finish(ss_engine* e, float grad_scale, int flags, void* stream);
/* After a SS_STEP_SPLIT_BACKWARD | SS_STEP_SPLIT_NO_JOIN step and BEFORE ss_train_finish is enqueued: make `consumer_stream`
 * (e.g. the stream the all-reduce of the decoder range is launched on) wait until the head + decoder gradients are final. */
int ss_wait_decoder_grads(ss_engine* e, void* consumer_stream);
/* the engine stream that carries the decoder's weight-gradient GEMMs (a hipStream_t; NULL if the engine runs without
 * branch streams).  A collective launched from it is ordered behind those GEMMs by construction. */
void* ss_side_stream(ss_engine* e);
/* How ss_bind chose the engine's branch streams.  The step forks three branches off the stream it is issued on; HIP maps a process's
 * streams onto 4 in-order hardware queues without saying which, and two streams on one queue cannot overlap (measured +14 % on the
 * step).  ss_bind therefore creates a pool of streams, MEASURES which of them share a queue with the caller's stream and with each
 * other (a 400 us spin kernel on one stream delays a trivial kernel on another only if they share a queue; ~10 ms once), keeps three
 * on queues of their own and destroys the rest.  Issue the steps on the stream that was passed to ss_bind. */
const char* ss_stream_report(const ss_engine* e);
/* first arena offset (floats) of the decoder + head parameters; [0, split) is the encoder */
long ss_grad_split(const ss_engine* e);

/* ---- data parallel over RCCL (nothing to mirror: the reference is single-device, solver.py:38) ----
 * One process per GPU.  Rank 0 obtains a 128-byte id (ss_comm_unique_id) and hands it to the other ranks by any means
 * (a file, MPI, torch.distributed's store); every rank then calls ss_comm_init.  RCCL is dlopen'd -- inside a process that
 * already loaded it (PyTorch) that copy is used. */
int ss_comm_unique_id(char* id128);
int ss_comm_init(ss_engine* e, const char* id128, int rank, int world);
int ss_comm_destroy(ss_engine* e);
/* in-place sum over the ranks of grads[offset, offset + count) (floats), enqueued on `stream` */
int ss_allreduce_grads(ss_engine* e, long offset, long count, void* stream);
/* The whole data-parallel step on this rank's shard (utterances [rank*B, (rank+1)*B) of the global batch and the matching
 * slices of the draws): the one-GPU step with the gradient arena all-reduced in BUCKETS on a communication stream of the engine's
 * own while the backward is still running -- each decoder layer (25 / 25 / 11 MB for Generator_3) as soon as its weight-gradient
 * GEMMs have retired (layer 2 first; they run beside the encoder backward), the head, the two wide layers of the conv trunk as the
 * trunk's backward passes them, and last the few MB that are final only at the end (layer-0 convolutions, encoder BLSTMs, Encoder_t,
 * the status slot); then Adam with the 1/world mean folded in.  flags: 0, SS_STEP_BUCKET (every rank passes the same T) and / or SS_STEP_ACCUMULATE.  loss: this
 * rank's local mean loss.  ss_g6_dp_train_step: the same for Generator_6 (cross-entropy step of ss_g6_train_step).
 * ss_tune("dp_model", R) MODELS an R-rank run on one GPU without a communicator: every collective is replaced by a stand-in kernel of
 * the modelled duration (ring all-reduce over one 153 GB/s xGMI link + 25 us), so a kernel trace shows where each bucket would sit
 * (tools/dp_timeline.sh); ss_tune("dp_buckets", 0) restores round 2's two buckets behind the whole backward. */
int ss_g3_dp_train_step(ss_engine* e, const float* mel_dev, const float* f0_dev, const float* emb_dev, const int* len_org_dev,
                        const float* scales_dev, const int* len_seg_dev, int B, int T, int flags, float* loss_dev, void* stream);
int ss_g6_dp_train_step(ss_engine* e, const float* mel_dev, const float* f0_onehot_dev, const int* target_idx_dev, const float* scales_dev,
                        const int* len_seg_dev, int B, int T, int flags, float* loss_dev, void* stream);
/* Where the collectives of a data-parallel step sit (for the multi-GPU scaling record): with ss_dp_profile(e, 1) every collective of
 * ss_g3_dp_train_step / ss_g6_dp_train_step is bracketed by hipEvents on the communication stream and one event marks the end of the
 * backward on the main stream.  ss_dp_profile_read (synchronises) returns the number of collectives of the LAST step and, for up to
 * `cap` of them in enqueue order, four doubles each: arena offset (-1: the grouped rest at the backward's end), element count, start
 * and end in microseconds RELATIVE TO THE BACKWARD'S END (negative = the collective ran beside the backward).  out == NULL: count only. */
/* Number of launches since ss_create that found the step's scratch (split-K partial slabs, column-sum partials, fused encoder weight gradients)
 * exhausted and took their slower fallback (atomics / unsplit / one workgroup per column block).  0 in a healthy run: an undersized scratch shows
 * up here instead of only in a profile. */
long ss_scratch_fallbacks(const ss_engine* e);
int ss_dp_profile(ss_engine* e, int on);
int ss_dp_profile_read(ss_engine* e, double* out, int cap);

/* torch.optim.Adam(G.parameters(), lr, [beta1, beta2]) (solver.py:62,172).  `step` = updates already applied. */
int ss_set_adam(ss_engine* e, double lr, double beta1, double beta2, double eps, long step, void* stream);
int ss_adam_step(ss_engine* e, float grad_scale, void* stream);
int ss_zero_grads(ss_engine* e, void* stream);

/* ---- gradient accumulation over micro-batches (nothing to mirror: the reference steps once per batch, solver.py:170-172; the semantics are
 *      those of calling loss.backward() k times between optimizer.zero_grad() and optimizer.step()) ----
 * SS_STEP_ACCUMULATE on ss_g3_train_step / ss_g6_train_step / ss_g3_dp_train_step / ss_g6_dp_train_step: the step's backward adds its
 *   parameter gradients to the arena.  A step WITHOUT the flag clears the arena as ever and so starts a new cycle.  In a
 *   SS_STEP_SPLIT_BACKWARD step the choice is made for the whole backward: the engine remembers it for the ss_train_finish that follows,
 *   which takes no accumulate flag of its own.  Without the flag every entry point enqueues exactly what it did before the flag existed.
 *   The arena then holds the plain SUM of the micro-batches' gradients, each the gradient of that micro-batch's own MEAN loss (no 1 / k
 *   inside).  As everywhere, grad_scale acts only inside the optimiser step and the norm: the caller of ss_*_train_step, ss_adam_step or
 *   ss_train_finish passes 1 / k (times 1 / world where it all-reduces itself).  The native data-parallel steps fold their mean in
 *   themselves: 1 / (world * ss_grad_accum_count).
 *   A cycle of k micro-batches on one GPU:   step(NO_ADAM);   step(NO_ADAM | ACCUMULATE) k - 2 times;   step(ACCUMULATE, grad_scale = 1 / k)
 *   -- or ss_zero_grads and then k accumulating steps.  Native data parallel: the first k - 1 micro-batches through the plain
 *   ss_g*_train_step(NO_ADAM [| ACCUMULATE]) (no collective is enqueued by them, communicator or not), the last through
 *   ss_g*_dp_train_step(ACCUMULATE), whose buckets all-reduce the local sums, each behind that micro-batch's last producer for its range.
 *   The micro-batches of one cycle may differ in B, in T (SS_STEP_BUCKET) and in route (fused, split, data-parallel): nothing is carried
 *   in the workspace between them, which a change of shape re-plans.  Each counts 1 / k through grad_scale whatever its size -- the mean of
 *   the micro-batches' means, which is the mean over the utterances only when they are equally large.  A cycle runs in ONE precision mode
 *   (ss_set_precision between cycles, not inside one).  Accumulating onto an arena the caller filled adds to it: the rule ss_op_gemm states
 *   for its C.  The status slot (the arena's last four floats) is overwritten by every backward, never added to.
 *   loss_dev stays the loss of the micro-batch of that call.  The clipping norm, its coefficient, the non-finite skip and the counters of
 *   ss_grad_clip_stats belong to the cycle's ONE optimiser step and act on the accumulated (and all-reduced) arena: one non-finite
 *   micro-batch skips the cycle's update once and counts once.
 * ss_grad_accum_count: backward passes summed into the arena since it was last cleared (host-side; no synchronisation): 0 after ss_bind and
 *   ss_zero_grads, 1 after a step or an ss_*_backward* without the flag, k after k - 1 further accumulating steps; 0 for a null engine. */
long ss_grad_accum_count(const ss_engine* e);

/* ---- clipping by global norm, and refusing non-finite gradients (nothing to mirror: the reference's solver never clips; the semantics are
 *      those of torch.nn.utils.clip_grad_norm_(G.parameters(), max_norm), norm_type 2, placed between backward and optimizer.step()) ----
 * ss_set_grad_clip: max_norm 0 = off (the default; every step is then enqueued exactly as without this call), > 0 = every optimiser step
 *   scales the gradients by coef = min(1, max_norm / (norm + 1e-6)), +inf = measure and guard only (coef is exactly 1).  Negative or NaN is
 *   refused with nothing enqueued, as is an engine that is not bound.  Resets the two counters of ss_grad_clip_stats.  ss_bind switches it off.
 *   The norm is grad_scale * the 2-norm of the PARAMETER elements of the gradient arena: the alignment gaps between tensors (behind the 257-float
 *   head bias) and the status slot in the arena's last four floats are never read, so a caller need not zero them.  Under data parallelism it is
 *   the norm of the ALL-REDUCED arena with the 1/world mean folded in through grad_scale: every rank computes the same coefficient.  float64 sums,
 *   one partial per workgroup added in a fixed order, no atomics: the same bits on every run and on every route to the optimiser (fused step,
 *   SS_STEP_NO_ADAM + ss_adam_step, ss_train_finish, SS_STEP_BUCKET, both data-parallel steps, both generators, both precisions).  Everything
 *   stays on the device; the fused one-GPU step sums the decoder + head range beside the encoder backward where it otherwise updates that range
 *   early, and updates the whole arena in one launch once the norm is known.
 *   SKIP: a norm that is not finite (one inf or NaN anywhere among the parameter elements) skips THAT optimiser step on the device -- parameters,
 *   both moments and the step counter untouched, exactly as for the status word -- but unlike the status word it is per step: no status bit is
 *   set, nothing is refused afterwards, and the next step runs normally.  The skipped counter is how a caller learns of it.
 * ss_grad_norm: stand-alone, *norm_dev = grad_scale * that norm of the arena as it is now (one device float); works whether or not clipping is on
 *   and changes neither the clip state nor the counters.
 * ss_grad_clip_stats: asynchronous device-to-device copy of four floats {norm of the last optimiser step before clipping, coefficient applied
 *   (0: the step was skipped), optimiser steps clipped (coef < 1), optimiser steps skipped as non-finite} since ss_set_grad_clip.  No
 *   synchronisation: read it the way the loss is read.  (The counters are floats: exact up to 2^24 steps.) */
int ss_set_grad_clip(ss_engine* e, float max_norm, void* stream);
int ss_grad_norm(ss_engine* e, float grad_scale, float* norm_dev, void* stream);
int ss_grad_clip_stats(ss_engine* e, float* out4_dev, void* stream);

/* ---- decoupled weight decay (AdamW) and an exponential moving average of the parameters, inside the optimiser step (nothing to mirror: the
 *      reference's solver uses plain Adam and keeps no average; the semantics are torch.optim.AdamW's single-tensor update and
 *      torch.optim.swa_utils.AveragedModel(G, multi_avg_fn=get_ema_multi_avg_fn(decay)).update_parameters(G) after optimizer.step()) ----
 * In the formulas t is the optimiser step being APPLIED (not skipped on the device: status word, remote status, non-finite norm under clipping).
 * WEIGHT DECAY: for a decayed element p1 = p * (float)(1 - lr * weight_decay) comes first, lr the current one of ss_set_adam (not lr / bc1), the
 *   factor formed in double on the device; today's Adam update then acts on p1.  Both moments are unchanged by decay.  which = 0: every parameter
 *   (AdamW(G.parameters(), weight_decay=wd) exactly); which = 1: tensors with ndim >= 2 only (conv, LSTM weight_ih / weight_hh, linear weights;
 *   biases and the GroupNorm affine are left alone), from ss_param_info's ndim.  Not built: coupled L2 decay (Adam(weight_decay=...)), amsgrad.
 * EMA: after an applied optimiser step, for every element of the arena, ema' = ema + w * (p' - ema), p' the fp32 parameter the step has just
 *   written, w = (float)(1 - d_t), d_t = decay, or with warm-up min(decay, (1 + n) / (10 + n)) with n the number of EMA updates applied so far.
 *   n lives in device memory beside the Adam state: it survives what that survives (geometry changes, ss_set_workspace, ss_set_adam).
 * SKIPS: a step skipped on the device changes nothing: neither p, m, v and the step counter (as ever) nor the decay, the average or n.
 * ACCUMULATION: only the cycle's one optimiser step decays and averages.
 * DECODER-ONLY STEP (ss_adam_step_decoder, ss_g3_decode_train_step without SS_STEP_NO_ADAM): decay acts on the decayed tensors inside
 *   [ss_grad_split, arena) only and the encoder range of p, m, v keeps its bits, but the average is still updated over the WHOLE arena, exactly
 *   once: the encoder range's parameters did not move, its average still approaches them (what AveragedModel.update_parameters does).
 * Both terms hold, with the same bits, on every route to the optimiser that covers the whole arena (fused step, SS_STEP_BUCKET, SS_STEP_NO_ADAM +
 * ss_adam_step, ss_train_finish, both data-parallel steps, both generators, clipping on or off): the factors and n are set once per step by the
 * step's one prepare kernel and every element sees the same values.  With both off -- the default, and what ss_bind restores -- every entry
 * point enqueues exactly what it did before these calls existed, to the same kernels.
 * ss_set_weight_decay: 0 = off.  Refused: negative, NaN or infinite weight_decay, which outside {0, 1}.
 * ss_set_ema: ema_dev is the caller's arena of ss_arena_numel floats, 16-byte aligned; NULL switches the average off.  updates < 0: the average
 *   starts as a copy of the parameters as they are now, n = 0.  updates >= 0: the buffer is adopted as it stands with n = updates (resuming).
 *   decay must lie in [0, 1).  The statistics of ss_ema_stats start again.
 * ss_ema_swap: exchanges the contents of the parameter arena and the EMA arena, gaps included; a second call restores the original bits.  Every
 *   forward re-lays the weights out from the parameter arena, so no cached image goes stale.  NOTE: a training step or optimiser step taken while
 *   swapped trains the AVERAGED weights; the engine does not prevent it (speechsplit_amd.Engine.ema_weights() does).
 * ss_ema_stats: asynchronous device-to-device copy of four floats {EMA updates applied (n), d_t of the last update, weight-decay factor of the
 *   last applied step, 0}; no synchronisation, as ss_grad_clip_stats.  (Floats: n is exact up to 2^24.)
 * All four need the optimiser's binding (both Adam arenas) and name a bad argument AFTER a missing binding. */
int ss_set_weight_decay(ss_engine* e, float weight_decay, int which, void* stream);
int ss_set_ema(ss_engine* e, float* ema_dev, double decay, int warmup, long updates, void* stream);
int ss_ema_swap(ss_engine* e, void* stream);
int ss_ema_stats(ss_engine* e, float* out4_dev, void* stream);

/* ---- learning-rate warm-up and decay inside the optimiser step, keyed on the device's own step counter (nothing to mirror: the reference's
 *      solver trains at a constant rate; the closed forms are those of torch.optim.lr_scheduler) ----
 * DEFINITION (float64 on the device, one thread, once per APPLIED step, every product and sum rounded on its own).  base is the lr of
 *   ss_set_adam.  t is the optimiser step being applied: 1-based, already incremented, exactly the t of the bias corrections.  s = t - 1.
 *   WARM-UP of W = warmup_steps >= 0 steps from the factor sf = warmup_start, 0 < sf <= 1:
 *     if W > 0 and s < W:  lr_t = base * (sf + (1 - sf) * ((double)s / (double)W))
 *   MAIN PART otherwise, with k = s - W, N = total_steps, P = period:
 *     kind 1 constant                         lr_t = base
 *     kind 2 cosine      (N >= 1, min_lr)     kk = min(k, N); lr_t = min_lr + (base - min_lr) * (0.5 * (1 + cospi((double)kk / (double)N)))
 *     kind 3 linear      (N >= 1, min_lr)     kk = min(k, N); lr_t = base + (min_lr - base) * ((double)kk / (double)N)
 *     kind 4 exponential (0 < gamma <= 1)     lr_t = max(base * pow(gamma, (double)k), min_lr)
 *     kind 5 step        (gamma, P >= 1)      lr_t = max(base * pow(gamma, (double)(k / P)), min_lr), integer division
 *   kind 0 is off: lr_t = base, the default and what ss_bind restores.
 * CONSUMERS: step_size = (float)(lr_t / bc1) and, under ss_set_weight_decay, the decay factor (float)(1 - lr_t * weight_decay).  Nothing else
 *   changes: the moments, the EMA, the clip coefficient and the bias corrections are what they were.
 * IN TORCH: SequentialLR(opt, [LinearLR(opt, sf, 1.0, W), main], [W]), or main alone when W = 0, with main = CosineAnnealingLR(T_max=N,
 *   eta_min=min_lr), LinearLR(1.0, min_lr / base, N), ExponentialLR(gamma) or StepLR(P, gamma), the rate read before each optimizer.step().
 *   Two deliberate differences: past N, cosine and linear STAY at min_lr (torch's cosine turns back up); and min_lr also floors the two
 *   geometric kinds (with min_lr = 0 they are torch's).
 * SKIPS: a step skipped on the device (status word, remote status, non-finite norm under clipping) leaves t alone, so the next applied step
 *   carries the rate of the SAME t; the words of ss_lr_stats do not move either.
 * POSITION: the schedule reads t, so ss_set_adam(..., step) positions it, and a run resumed from a checkpoint's step count lands on the right
 *   point without any further state.  In an accumulation cycle t counts optimiser steps, not micro-batches.
 * The options live in device memory beside the Adam state and survive what it survives (geometry changes, ss_set_workspace, ss_set_adam).
 * Every route to the optimiser picks the rate up from its one prepare kernel: the fused step, SS_STEP_BUCKET, SS_STEP_NO_ADAM + ss_adam_step,
 * ss_train_finish, both data-parallel steps, ss_adam_step_decoder, ss_g3_decode_train_step, both generators, both precisions.  With kind 0
 * every entry point enqueues exactly the kernels and arguments it did before these calls existed.
 * ss_set_lr_schedule: refused, with nothing enqueued: an engine without the optimiser's binding (both Adam arenas); then a kind outside
 *   0 .. 5; and for a kind other than 0: warmup_steps < 0; warmup_start outside (0, 1] or NaN; total_steps < 1 for cosine and linear; gamma
 *   outside (0, 1] or NaN for exponential and step; period < 1 for step; a negative or non-finite min_lr.  Options the kind does not read
 *   are ignored.  The words of ss_lr_stats start again (zero, and the kind).  Both calls name a bad argument AFTER a missing binding.
 * ss_lr_stats: asynchronous device-to-device copy of four floats {(float)lr_t of the last applied step, (float)(lr_t / base), t, kind}; no
 *   synchronisation, as ss_grad_clip_stats.  (Floats: t is exact up to 2^24.) */
int ss_set_lr_schedule(ss_engine* e, int kind, int warmup_steps, double warmup_start, int total_steps, double gamma, int period, double min_lr,
                       void* stream);
int ss_lr_stats(ss_engine* e, float* out4_dev, void* stream);

/* ---- InterpLnr as a standalone module (model.py:355-436; solver.py:59,161) ---- */
/* x [B,T,C], len_seq i32[B], draws [B*7] -> y [B,max_len_pad,C].  Optional outputs (may be NULL): i0 i32[B,P],
 * lam f32[B,P], counts i32[B] (un-truncated, model.py:418). */
int ss_interp_forward(ss_engine* e, const float* x_dev, const int* len_seq_dev, const float* scales_dev,
                      const int* len_seg_dev, int B, int T, int C, float* y_dev, int* i0_dev, float* lam_dev,
                      int* counts_dev, void* stream);
/* adjoint of the last ss_interp_forward: dy [B,P,C] -> dx [B,T,C] */
int ss_interp_backward(ss_engine* e, const float* dy_dev, int B, int T, int C, float* dx_dev, void* stream);

/* ---- offline feature extraction, the part that can be pinned without librosa / pysptk (make_spect_f0.py:57-71, utils.py:18-42) ----
 * wav: float64 [n] AFTER the host-side high-pass filtfilt and dither (make_spect_f0.py:53-54); mel_basis: float64 [513][n_mels]
 * (make_spect_f0.py:15 takes librosa's, transposed; here an input); out: float32 [ss_melspec_frames(n)][n_mels] =
 * (20 log10(max(1e-5, |STFT| . mel)) - 16 + 100) / 100 with the reference's reflect padding, periodic Hann window, 1024-point
 * transform and hop 256, computed in float64 as numpy does.  No engine needed. */
int ss_melspec_frames(int n);
int ss_melspec(const double* wav_dev, int n, const double* mel_basis_dev, int n_mels, float* out_dev, void* stream);
/* f0 float64 [n], -1e10 = unvoiced (RAPT's otype=2 convention, make_spect_f0.py:63-64) -> float32: (f0 - mean) / std / 4 clipped to
 * [-1, 1] and mapped to [0, 1] for voiced frames, mean / std over the voiced frames (utils.py:35-42). */
int ss_f0_normalize(const double* f0_dev, int n, float* out_dev, void* stream);

/* ---- pitch tracker: waveforms to F0 tracks (the stand-in for make_spect_f0.py:64's `pysptk.sptk.rapt`, which is not pinned here) ----
 * The published core of RAPT (Talkin 1995, "A robust algorithm for pitch tracking"): normalised cross-correlation candidates per frame plus
 * dynamic programming over the frames, with Talkin's published constants.  NOT a port of SPTK's rapt and no parity with it is claimed: RAPT's
 * two-rate search is left out, and its spectral-stationarity term (an LPC analysis per frame) is optional and off by default -- see
 * "spectral stationarity" below (ss_pitch_track_stat).  The output follows RAPT's otype=2 convention -- ln(F0 in
 * Hz), -1e10 for unvoiced frames, one value per 256-sample hop, ss_melspec_frames(n) values -- so ss_f0_normalize takes it unchanged.
 *
 * Constants: fs = 16000, hop = 256, correlation window w = 120, CAND_TR = 0.3, N_CANDS = 20 (19 voiced states plus the unvoiced one),
 * LAG_WT = 0.3, FREQ_WT = 0.02, DOUBL_C = 0.35, VTRAN_C = 0.005, VTR_A_C = 0.5, VO_BIAS = 0, A_FACT = 10000.
 * Inputs: x float64 [n], scale (the Python layer passes 32768, as the reference does), lo, hi in Hz.  Lmin = floor(16000 / hi),
 * Lmax = ceil(16000 / lo), K = Lmax - Lmin + 1, S = w + Lmax, F = n / 256 + 1 = ss_melspec_frames(n).
 * Per frame i, independent of every other frame:
 *   1. z_j = scale x[s + j], 0 <= j < S, s = 256 i - S / 2 (integer division), zero wherever s + j is outside [0, n).
 *      mu = sum_j z_j / S; y = z - mu for all S entries.
 *   2. e_k = sum_{j=k}^{k+w-1} y_j^2; phi_k = sum_{j<w} y_j y_{j+k} / sqrt(e_0 e_k + A_FACT) for Lmin <= k <= Lmax; phimax = max_k phi_k;
 *      rms_i = sqrt(sum_{j<S} y_j^2 / S + 1).
 *   3. Lag k is a voiced candidate when Lmin < k < Lmax, phi_k > phi_{k-1}, phi_k >= phi_{k+1}, phi_k > 0 and phi_k >= CAND_TR phimax.
 *      den = phi_{k-1} - 2 phi_k + phi_{k+1}; delta = 0.5 (phi_{k-1} - phi_{k+1}) / den if den < 0, else 0; L = k + delta;
 *      v = phi_k - 0.25 (phi_{k-1} - phi_{k+1}) delta.  The 19 largest v are kept, the smaller lag first on equal v.  State 0 is
 *      "unvoiced", states 1.. are the kept candidates in that order.
 *   4. Local cost d(0) = VO_BIAS + max(phimax, 0); d = 1 - v (1 - LAG_WT L / Lmax) for a voiced state.
 * Over the frames of one utterance: D_0 = d_0; D_i(a) = d_i(a) + min_b [D_{i-1}(b) + t_i(b -> a)], the lowest b on a tie, with
 * rr_i = rms_i / rms_{i-1} and
 *      t(unvoiced -> unvoiced) = 0;  t(unvoiced -> voiced) = VTRAN_C + VTR_A_C / rr_i;  t(voiced -> unvoiced) = VTRAN_C + VTR_A_C rr_i;
 *      t(voiced b -> voiced a) = FREQ_WT min(|xi|, DOUBL_C + |xi - ln 2|, DOUBL_C + |xi + ln 2|), xi = ln(L_a / L_b).
 * The end state is the argmin of D_{F-1} (the lowest index on a tie); backtrack from there.  f0_i = ln(16000 / L) for a voiced state,
 * -1e10 for state 0.
 * Arithmetic: float64, no atomics, the same bits on every run.  Order of the sums: mu and sum y^2 -- thread t of 256 adds its entries
 * j = t, t + 256, t + 512 in that order, then a pairwise tree over the 256 partials (t += t + s, s = 128, 64 .. 1); the three w-long sums of a
 * lag (sum y_j y_{j+k}, e_k and e_0; e_k is summed directly, not carried from e_{k-1}) run j = 0 .. w - 1 in order; xi is taken as
 * ln L_a - ln L_b; the minimum over b runs b = 0, 1, .. with a strict <.  Multiply-adds may be fused.
 *
 * Shapes: wav [B][max_n], f0 [B][F], phi [B][F][K], rms [B][F] with F = ss_melspec_frames(max_n).  No engine needed, no allocation inside,
 * asynchronous on `stream`.  n_dev i32[B] (NULL: every row has max_n samples): row b is, bit for bit, the result of running that utterance
 * alone at min(max(n[b], 513), max_n) samples -- a length outside 513 .. max_n spoils that row only; samples at or beyond it are never read
 * (they may hold NaN); f0 beyond the row's own F is -1e10 (ss_collate's padding), phi and rms beyond it are exact zeros; the hook
 * ss_op_pitch_dp never reads phi or rms there.
 * Refused before anything is enqueued, with a message that names the argument: null required pointers, B outside 1 .. 65535, max_n outside
 * 513 .. 256 (SS_MAX_EVAL_FRAMES - 1), lo_hz / hi_hz NaN or not positive, not lo_hz < hi_hz, Lmin < 16 (hi_hz above 1000), Lmax > 400
 * (lo_hz below 40) or K < 3, scale not finite or <= 0, scratch_bytes below ss_pitch_scratch_bytes(B, max_n, lo_hz, hi_hz) or scratch_dev
 * not 256-byte aligned. */
long ss_pitch_scratch_bytes(int B, int max_n, double lo_hz, double hi_hz);            /* host only; -1 + ss_last_error on bad arguments */
int  ss_pitch_track(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double lo_hz, double hi_hz,
                    double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);   /* f0 [B][ss_melspec_frames(max_n)] */
/* test hooks, each half alone; ss_op_pitch_dp takes the same scratch as ss_pitch_track */
int  ss_op_nccf(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double lo_hz, double hi_hz,
                double* phi_dev /* [B][F][K] */, double* rms_dev /* [B][F] */, void* stream);
int  ss_op_pitch_dp(const double* phi_dev, const double* rms_dev, const int* n_dev, int B, int max_n, double lo_hz, double hi_hz,
                    double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);

/* ---- pitch tracker, spectral stationarity: RAPT's third voicing-transition term (off unless these entry points are called) ----
 * In RAPT the cost of switching between voiced and unvoiced has a constant, a level-ratio part and a spectral part that makes a switch
 * cheap where the short-time spectrum changes and expensive where it stands still.  This is the published term -- Talkin 1995, and
 * get_f0's get_stationarity / get_similarity as published -- with the published constants; as for the rest of the tracker, no parity with
 * SPTK is claimed.  What it does NOT take from get_f0: rr stays the ratio of the NCCF segments' rms (get_f0 takes it from these windows).
 *
 * Constants: STAT_W = 480 (a 30 ms window), STAT_GAP = 320 (20 ms between the two windows' centres), LPC_ORD = 18 (2 + fs / 1000),
 * PREEMP = 0.4, ff = 1 / (1 + 10^-3) (the 30 dB stabilising floor), VTR_S_C = 0.5, and the offsets 0.8 and 0.2 of S below.
 * Frame i >= 1 has two windows: A centred on sample 256 i - 160 and B centred on sample 256 i + 160.  Per window centred on c, on the
 * tracker's scaled samples z = scale x (zero wherever the index is outside [0, n)):
 *      s = c - 240;  u_j = z[s + j], 0 <= j <= 480;  y_j = w_j (u_{j+1} - PREEMP u_j), j < 480, w_j = 0.5 - 0.5 cos(2 pi (j + 0.5) / 480);
 *      r_k = sum_{j < 480 - k} y_j y_{j+k}, k = 0 .. 18.
 *      If r_0 == 0: rho = a = (1, 0, .., 0) and E = 1.  Otherwise rho_0 = 1, rho_k = ff r_k / r_0, and Levinson-Durbin from a = (1), E = 1:
 *      for m = 1 .. 18: kappa = -(rho_m + sum_{q=1}^{m-1} a_q rho_{m-q}) / E;  a'_q = a_q + kappa a_{m-q} for q < m;  a'_m = kappa;
 *      E <- E (1 - kappa^2).
 * Itakura distortion of B's predictor on A's signal: c_0 = sum_q (a^B_q)^2, c_k = 2 sum_{q=0}^{18-k} a^B_q a^B_{q+k},
 *      d = (c_0 + sum_{k=1}^{18} c_k rho^A_k) / E^A;   S_i = min(0.2 / (max(d, 1) - 0.8), 1).
 * In exact arithmetic d >= 1, so 0 < S <= 1 and the outer min does nothing; in float64 0.2 / (1 - 0.8) is 1 + 2^-52, which it cuts off.
 * S_0 is unused and stored as an exact 0; beyond a row's own F the entries are exact zeros, as for phi and rms.
 * Transitions: VTR_S_C S_i is added to t(unvoiced -> voiced) and to t(voiced -> unvoiced) into frame i and to nothing else, as
 * (VTRAN_C + VTR_A_C / rr_i) + VTR_S_C S_i and (VTRAN_C + VTR_A_C rr_i) + VTR_S_C S_i: a track of zeros gives ss_pitch_track's bits.
 * Order of the sums: each r_k is cut into 24 chunks j = 20 c .. 20 c + 19, c = 0 .. 23, with y_j taken as 0 for j >= 480 (those terms add
 * exact zeros); thread 10 c + 5 w + g of 256 (w = 0 for A, 1 for B; g = 0 .. 4) adds the terms of chunk c for the lags k = 4 g .. 4 g + 3
 * (k <= 18), each lag in index order from zero, then thread 19 w + k adds that sum's 24 partials in chunk order, from p_0:
 * (((p_0 + p_1) + p_2) + ..) + p_23.  The Levinson sum starts from rho_m and adds a_q rho_{m-q} for q = 1, 2, ..; c_k adds
 * q = 0, 1, .. from zero (then doubles); d's numerator starts from c_0 and adds c_k rho^A_k for k = 1, 2, ..  Multiply-adds may be fused.
 *
 * ss_pitch_track_stat: ss_pitch_track's arguments, rules and refusals, with a scratch of ss_pitch_stat_scratch_bytes (that of
 * ss_pitch_scratch_bytes plus the S track [B][F], 256-byte aligned); it runs the NCCF, the stationarity, the candidates and the
 * recurrence.  Hooks: ss_op_pitch_stationarity writes S [B][F] alone (refused: null wav_dev / stat_dev, B, max_n, scale as above);
 * ss_op_pitch_dp_stat is ss_op_pitch_dp (same scratch) with stat_dev [B][F], also refused when null; it never reads stat beyond a row's F. */
long ss_pitch_stat_scratch_bytes(int B, int max_n, double lo_hz, double hi_hz);       /* host only; -1 + ss_last_error on bad arguments */
int  ss_pitch_track_stat(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double lo_hz, double hi_hz,
                         double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);
int  ss_op_pitch_stationarity(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double* stat_dev /* [B][F] */,
                              void* stream);
int  ss_op_pitch_dp_stat(const double* phi_dev, const double* rms_dev, const double* stat_dev, const int* n_dev, int B, int max_n,
                         double lo_hz, double hi_hz, double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);

/* ---- batched feature extraction: make_spect_f0.py:49-71 on ragged batches of recordings (filter, dither, mel spectrogram, F0 normalisation;
 * the pitch track between them is ss_pitch_track above, which takes the same wav / n_dev / B / max_n) ----
 * One length vector serves every call: n_dev i32[B] (NULL: every row has max_n samples).  Every kernel clamps n[b] into [513, max_n]:
 * row b has n_b = min(max(n[b], 513), max_n) samples and F_b = n_b / 256 + 1 frames of F = ss_melspec_frames(max_n) -- a length outside
 * 513 .. max_n spoils that row only.  Row b is, bit for bit, the result of running that utterance alone; nothing at or beyond n_b (F_b for
 * ss_f0_normalize_batch) is read -- it may hold NaN; defined filler is written behind it.  No atomics, every sum in a fixed order: the same
 * bits on every run.  No engine needed, no allocation inside, asynchronous on `stream`.
 *
 * ss_filtfilt: scipy.signal.filtfilt(b, a, x) for 6 coefficients (a 5th-order filter; scipy's default odd extension by
 * padlen = 3 * 6 = 18), then the scaling and dither of make_spect_f0.py:54-55.  No other order is provided.  x, dither, y: float64
 * [B][max_n], distinct buffers.  b[6], a[6], zi[5] are HOST arrays, read at call time (the Python layer computes them with signal.butter /
 * signal.lfilter_zi, as mel_basis is an input); a[0] must be exactly 1.  The reference's filter (30 Hz high-pass, poles at
 * |z| = 0.988 .. 0.996) is ill-conditioned in scipy's direct form: any other arrangement of the arithmetic lands ~3e-7 of max |y| away from
 * scipy's result, which moves the mel spectrogram by more than 1e-6.  So the result is DEFINED as this sequence of IEEE double operations --
 * every product and every sum rounded to double on its own, no fused multiply-add -- and equals scipy's to the bit:
 *   Extension.  With i = j - 18 for j in [0, n + 36): ext[j] = 2 x[0] - x[-i] for i < 0; ext[j] = x[i] for 0 <= i < n;
 *               ext[j] = 2 x[n-1] - x[2(n-1) - i] for i >= n.
 *   Step.       step(u): y = b0*u + z0; z_i = (b_{i+1}*u + z_{i+1}) - a_{i+1}*y for i = 0..3; z4 = b5*u - a5*y; returns y.
 *   Pass 1.     z = zi * ext[0]; v[j] = step(ext[j]), j ascending.
 *   Pass 2.     z = zi * v[n+35]; w[j] = step(v[j]), j descending.
 *   Output.     y[i] = w[i + 18], 0 <= i < n.
 *   Epilogue.   out[i] = y[i]*gain + (r[i] - 0.5)*dither_scale, rounded step by step, r = dither_dev (prng.rand values of the speaker's numpy stream:
 *               drawn on the host, or on the device by ss_mt19937_rand and ss_dither_rows below); dither_dev == NULL: out[i] = y[i]*gain.  gain = 0.96 and
 *               dither_scale = 1e-06 are make_spect_f0.py:54-55 exactly.  The odd-length fix of :52-53 changes n and stays in Python.
 * Zeros are written behind n_b.  scratch: the first pass's output, [B][max_n + 36] doubles, rounded up to 256 bytes.
 *
 * ss_melspec_batch: ss_melspec's chain on every row -- reflect padding by 512 about the row's OWN ends, periodic Hann window, 1024 points,
 * hop 256, mel projection (the 513-term sum in bin order), dB floor and offsets, [0, 1] scaling -- with the vocoder's 1024-point FFT in
 * place of ss_melspec's direct DFT (the two agree to ~1e-13 before the float32 cast).  mel_basis: float64 [513][n_mels];
 * out: float32 [B][F][n_mels], zeros in frames at or beyond F_b.
 *
 * ss_f0_normalize_batch: f0 float64 [B][F] (ss_pitch_track's output) -> float32 [B][F]: voiced frames (f0 != -1e10) of row b come out with
 * the bits of ss_f0_normalize on that row's F_b frames alone; unvoiced frames and frames at or beyond F_b get (float)unvoiced.
 *
 * Refused before anything is enqueued, with a message that names the argument: null required pointers, B outside 1 .. 65535, max_n outside
 * 513 .. 256 (SS_MAX_EVAL_FRAMES - 1) (ss_pitch_track's range), a[0] != 1, a b / a / zi entry, gain or dither_scale that is not finite,
 * scratch_bytes below ss_filtfilt_scratch_bytes(B, max_n) or scratch_dev not 256-byte aligned, n_mels < 1, unvoiced NaN. */
long ss_filtfilt_scratch_bytes(int B, int max_n);                                     /* host only; -1 + ss_last_error on bad arguments */
int  ss_filtfilt(const double* x_dev, const int* n_dev, int B, int max_n, const double* b, const double* a, const double* zi,
                 double gain, const double* dither_dev, double dither_scale, double* y_dev, void* scratch_dev, long scratch_bytes,
                 void* stream);
int  ss_melspec_batch(const double* wav_dev, const int* n_dev, int B, int max_n, const double* mel_basis_dev, int n_mels,
                      float* out_dev, void* stream);
int  ss_f0_normalize_batch(const double* f0_dev, const int* n_dev, int B, int max_n, double unvoiced, float* out_dev, void* stream);

/* ss_resample: recordings of any sample rate to the chain's 16 kHz (or back) -- scipy.signal.resample_poly(x, up, down) with a CALLER-SUPPLIED
 * filter, on ragged batches.  The ragged-batch rules are the ones above, with 1 in place of 513: row b has n_b = min(max(n[b], 1), max_n)
 * input samples and m_b = ceil(n_b up / down) output samples; M = ceil(max_n up / down) = ss_resample_len(max_n, up, down) columns are
 * written; a length outside 1 .. max_n spoils that row only; row b is, bit for bit, the result of running that recording alone.
 * x: float64 [B][max_n]; y: float64 [B][M]; h: float64 [n_taps] ON THE DEVICE, n_taps odd, half = (n_taps - 1) / 2.  h is an input, as
 * mel_basis and b, a, zi are: the Python layer passes scipy's own design for the reduced up / down,
 *     h = scipy.signal.firwin(20 max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up.
 * The result is DEFINED as this sequence of IEEE double operations -- every product and every sum rounded to double on its own, no fused
 * multiply-add -- and equals resample_poly's to the bit (summing the same taps in descending order already differs in the last place):
 *     y[b][m] = 0.0 + sum over k of x[b][k] * h[m*down + half - k*up],   0 <= m < m_b,
 * the sum over exactly those k with 0 <= k < n_b and 0 <= m*down + half - k*up < n_taps, k ascending: acc = 0.0; then acc = acc + x[b][k] * h[..]
 * for each such k in turn.  An output no tap reaches is 0.0.  Exact zeros are written in columns m_b .. M - 1.  x[b][k] for k >= n_b is never
 * read and may hold NaN: the range of k is a bound of the loop, not a zero tap multiplied in (NaN * 0 is NaN).  All index arithmetic is
 * in long.  No atomics, nothing crosses rows or outputs: the same bits on every run.  No engine needed, no allocation inside, asynchronous on
 * `stream`.  scratch: ss_resample_scratch_bytes(up, n_taps) bytes, 256-byte aligned; that is 0 today (the kernel reads h as it is given), and
 * scratch_dev may then be NULL.
 * Refused before anything is enqueued, with a message that names the argument: null x_dev / h_dev / y_dev, B outside 1 .. 65535, max_n < 1,
 * up or down outside 1 .. 1024, n_taps < 1 or even, max_n whose M does not fit an int (the 16 kHz chain behind it takes an int max_n),
 * scratch_bytes below ss_resample_scratch_bytes(up, n_taps), scratch_dev NULL while bytes are needed or not 256-byte aligned. */
long ss_resample_len(long n, int up, int down);              /* host only: ceil(n * up / down); -1 + ss_last_error on bad arguments (n outside 0 .. 2^40) */
long ss_resample_scratch_bytes(int up, int n_taps);          /* host only; may be 0; -1 + ss_last_error on bad arguments */
int  ss_resample(const double* x_dev, const int* n_dev, int B, int max_n, int up, int down, const double* h_dev, int n_taps,
                 double* y_dev, void* scratch_dev, long scratch_bytes, void* stream);

/* ss_remove_silence: trim the room tone at both ends of a recording and cap the pauses inside it, on ragged batches at the chain's 16 kHz
 * (nothing to mirror: users of the reference trim with librosa before make_spect_f0.py; parity with librosa.effects.trim / split is NOT
 * claimed -- this is the definition below, a RELATIVE threshold only, with no absolute gate).
 * Float64 throughout.  Every product and every sum is rounded to double on its own, no fused multiply-add; a sum "in order" adds one term at
 * a time, index ascending, starting from its first term.  x: float64 [B][max_n]; n_dev: i32 [B] (NULL: every row is full); row b has
 * n_b = min(max(n[b], 1), max_n) samples; a length outside 1 .. max_n spoils that row only; nothing at or beyond n_b is read (it may hold
 * NaN); row b is, bit for bit, the result of running that recording alone.  No atomics, no allocation inside, no engine needed, asynchronous
 * on `stream`.
 *   Blocks.    Block j covers samples [256 j, min(256 j + 256, n_b)), j = 0 .. J - 1, J = ceil(n_b / 256); only the last block may be short.
 *              256 is the chain's mel hop, so a removed block is a removed mel frame.  Jmax = ceil(max_n / 256).
 *   Levels.    Quarter sums Q_q = sum of x[i]^2 over i in [128 q, min(128 q + 128, n_b)), in order, q = 0 .. ceil(n_b / 128) - 1.  The level of
 *              block j is the energy of the 512-sample window centred on it, E_j = ((Q_{2j-1} + Q_{2j}) + Q_{2j+1}) + Q_{2j+2}; quarters that
 *              do not exist (q < 0, or q beyond the last) are left out and the rest are added in that order.  It is a plain SUM, not a mean: a
 *              window cut by the recording's end counts as quieter.  E_max = max_j E_j (NaN if a level is NaN).
 *   Activity.  a_j = E_j > ratio * E_max, STRICTLY; `ratio` in (0, 1) is the caller's (the Python layer passes 10 ** (-top_db / 10)); there is
 *              no logarithm on the device.  If no block is active (only when E_max is 0, or not finite) every block is kept and the row comes
 *              out as it went in.  Hangover: d_j = any a_i with |i - j| <= hang.
 *   Kept.      Take the maximal runs of d_j == 0, of length R.  A leading run (it contains block 0) keeps its last min(R, edge) blocks; a
 *              trailing run (it contains block J - 1) keeps its first min(R, edge) blocks; an interior run is kept whole when pause < 0 or
 *              R <= pause, otherwise it keeps its first ceil(pause / 2) and its last floor(pause / 2) blocks.  Every block with d_j == 1 is
 *              kept.  hang, edge >= 0 and pause >= -1 are ints: pause = -1 only trims, edge at or above J only caps pauses.  K blocks are
 *              kept; inv[c] is the c-th of them, ascending.
 *   Output.    y is the kept blocks in order: output block c starts at 256 c, and the new length is m_b = 256 (K - 1) + (length of block
 *              inv[K-1]).  Block c is a copy of block inv[c], to the bit, when c == 0 or inv[c-1] + 1 == inv[c].  At a join
 *              (inv[c-1] + 1 != inv[c]; write a = inv[c-1]) the first min(128, length of block inv[c]) samples are a cross-fade whose
 *              fade-out side is the signal that FOLLOWED the last kept block -- below the threshold by construction:
 *                  y[256 c + r] = x[256 (a + 1) + r] * (1.0 - g[r]) + x[256 inv[c] + r] * g[r]
 *              the difference 1.0 - g[r] and the two products first, then their sum.  Block a + 1 is always a full block inside the row
 *              (a + 1 < inv[c] <= J - 1).  g: HOST array [128], an input as STOI's window is; the Python layer passes
 *              g[r] = 0.5 - 0.5 cos(pi (r + 0.5) / 128) evaluated with the C library's cosine.  Exact zeros are written behind m_b.
 * y_dev: float64 [B][max_n]; m_dev: i32 [B]; inv_dev: i32 [B][Jmax] with -1 behind the K kept blocks, and k_dev: i32 [B], are outputs and may
 * each be NULL.  scratch: ss_silence_scratch_bytes(B, max_n) bytes, 256-byte aligned.  Every index a kernel reads back from scratch or from
 * inv / K is clamped into the row's own blocks and samples: a corrupt map changes numbers, never addresses (K into 1 .. J, a block into
 * 0 .. J - 1, a sample index to at most n_b - 1, m_b to at most n_b).
 * Test hooks, each a stage alone.  ss_op_silence_levels: x -> e [B][Jmax], zeros behind J_b.  ss_op_silence_mask: e [B][max_j] and a per-row
 * block count j_dev (i32 [B]; NULL: max_j; clamped into 1 .. max_j) -> inv [B][max_j], k [B].  ss_op_silence_gather: x, inv, k (INPUTS, read
 * with the clamps above) -> y, m.
 * Refused before anything is enqueued, with a message that names the argument: null x_dev / y_dev / m_dev / g / scratch_dev (the hooks: their
 * own pointers), B outside 1 .. 65535, max_n outside 1 .. 256 (SS_MAX_EVAL_FRAMES - 1) (max_j outside 1 .. SS_MAX_EVAL_FRAMES - 1), ratio not
 * in (0, 1), hang or edge negative, pause < -1, a g entry that is not finite, scratch_bytes below ss_silence_scratch_bytes(B, max_n),
 * scratch_dev not 256-byte aligned. */
long ss_silence_scratch_bytes(int B, int max_n);             /* host only; -1 + ss_last_error on bad arguments */
int  ss_remove_silence(const double* x_dev, const int* n_dev, int B, int max_n, double ratio, int hang, int edge, int pause,
                       const double* g /* host [128] */, double* y_dev /* [B][max_n] */, int* m_dev /* [B] */,
                       int* inv_dev /* [B][Jmax], -1 behind K; nullable */, int* k_dev /* [B]; nullable */, void* scratch_dev,
                       long scratch_bytes, void* stream);
int  ss_op_silence_levels(const double* x_dev, const int* n_dev, int B, int max_n, double* e_dev /* [B][Jmax] */, void* stream);
int  ss_op_silence_mask(const double* e_dev, const int* j_dev, int B, int max_j, double ratio, int hang, int edge, int pause,
                        int* inv_dev /* [B][max_j] */, int* k_dev /* [B] */, void* stream);
int  ss_op_silence_gather(const double* x_dev, const int* n_dev, int B, int max_n, const int* inv_dev, const int* k_dev,
                          const double* g /* host [128] */, double* y_dev, int* m_dev, void* stream);

/* ss_mt19937_rand: the dither draw of make_spect_f0.py:55 on the device -- numpy.random.RandomState.rand(count) continued from a
 * caller-supplied generator state, bit for bit in every draw and in the state left behind.
 * state_dev: unsigned [625] ON THE DEVICE, read and written in place: state[0 .. 623] is numpy's `key`, state[624] numpy's `pos` in 0 .. 624
 * (RandomState.get_state()[1] and [2]).  A pos above 624 cannot be refused on the host; the kernel treats it as 624.
 *   Recurrence.  N = 624, M = 397, A = 0x9908b0df.  x[0 .. 623] = key; for n >= 0, with y = (x[n] & 0x80000000) | (x[n+1] & 0x7fffffff):
 *                x[n+624] = x[n+397] ^ (y >> 1) ^ ((y & 1) ? A : 0).
 *   Tempering.   temper(y): y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680; y ^= (y << 15) & 0xefc60000; y ^= y >> 18.
 *   Stream.      word j is w[j] = temper(x[pos + j]).
 *   Draw.        out[i] = ((w[2i] >> 5) * 67108864.0 + (w[2i+1] >> 6)) / 9007199254740992.0, 0 <= i < count.  Every operation of the
 *                conversion is exact in double: there is no rounding and no contraction question.
 *   State after. count == 0: the state is unchanged, nothing is written and nothing is enqueued.  Otherwise, with tot = pos + 2 count and
 *                k = (tot - 1) / 624 (integer division): key' = x[624k .. 624k + 623] and pos' = tot - 624k.  That is what numpy holds after
 *                the same draws: the whole regenerated block, even when it is partly consumed (k == 0: the key as it was).
 * Two calls of c1 and c2 draws are one call of c1 + c2.  Word n + 624 needs nothing newer than n + 397, so 227 consecutive words are independent
 * and no more: a call is a chain of about 2 count / 227 dependent steps walked by ONE workgroup (there is no cheap jump-ahead, and none is
 * built).  No atomics, no allocation inside, no engine needed, asynchronous on `stream`.
 *
 * ss_dither_rows: the contiguous stream gathered into the [B][max_n] layout ss_filtfilt takes as dither_dev.  draws_dev: float64 [count];
 * first_dev: long [B] and n_dev: int [B], both ON THE DEVICE and read in stream order; out_dev: float64 [B][max_n].  Row b has
 * n_b = min(max(n[b], 0), max_n) draws: out[b][i] = draws[first[b] + i] for i < n_b, and exact zeros behind n_b.  A first[b] outside
 * [0, count - n_b] spoils that row only: it is clamped into [0, max(count - n_b, 0)], and a column whose draw would still lie at or beyond
 * count (n_b above count) is zero, so nothing outside draws[0 .. count) is read.  All index arithmetic is in long.
 *
 * Refused before anything is enqueued, with a message that names the argument: null state_dev, draws_dev, first_dev, n_dev or out_dev
 * (ss_mt19937_rand's out_dev may be NULL only when count == 0), count outside 0 .. 2^40, B outside 1 .. 65535, max_n < 1. */
int  ss_mt19937_rand(unsigned* state_dev /* [625] in/out */, long count, double* out_dev /* [count] */, void* stream);
int  ss_dither_rows(const double* draws_dev, long count, const long* first_dev, const int* n_dev, int B, int max_n,
                    double* out_dev /* [B][max_n] */, void* stream);

/* ---- Griffin-Lim vocoder: mel spectrograms back to waveforms (the checkpoint-free stand-in for demo.ipynb's WaveNet cell) ----
 * The inverse of ss_melspec's chain: mel [0, 1] -> amplitude 10^((100 mel - 100 + 16) / 20) -> linear magnitude through a CALLER-SUPPLIED
 * float64 inv_basis [n_mels][513] (the Python layer passes numpy.linalg.pinv of the [513][n_mels] basis), floored at `floor` >= 0 ->
 * Griffin-Lim with momentum as published (Perraudin et al. 2013, librosa's form) over ss_melspec's STFT (reflect padding by 512, periodic
 * Hann window, 1024-point transform, hop 256) and its inverse (window, overlap-add in frame order, division by the sum of the squared windows
 * of the frames that cover a sample -- 1.5 inside, down to 1.25 at the kept edges -- trimmed by 512 at both ends):
 *     ang = exp(i phase0); tprev = 0; n_iter times { r = STFT(ISTFT(mag ang)); a = r - momentum / (1 + momentum) tprev; tprev = r;
 *     ang = a / (|a| + 1e-16) }; wav = ISTFT(mag ang).
 * float64 throughout, a real FFT in LDS, no atomics: the same bits on every run.  phase0 [B][max_frames][513] is an input like every draw of
 * this ABI (NULL: zeros).  No engine needed, no allocation inside, asynchronous on `stream`.
 * Shapes: mel [B][max_frames][n_mels], mag [B][max_frames][513], spec [B][max_frames][513][2] (re, im),
 * wav [B][ss_griffinlim_samples(max_frames)]; F frames are 256 (F - 1) samples, and ss_melspec_frames of that is F again.
 * frames_dev i32[B] (NULL: every row has max_frames): row b is the result of running that utterance alone at
 * min(max(frames[b], 4), max_frames) frames -- a count outside 4 .. max_frames spoils that row only; mel / mag / spec / phase0 frames at or
 * beyond it are never read (they may hold NaN), output samples (and mag / spec frames) beyond it are exact zeros.
 * Refused before anything is enqueued, with a message that names the argument: null required pointers, B < 1, max_frames outside
 * 4 .. SS_MAX_EVAL_FRAMES, n_mels outside 1 .. 4096, n_iter outside 0 .. 1024, momentum outside [0, 1) or NaN, negative or NaN floor,
 * scratch_bytes below ss_griffinlim_scratch_bytes(B, max_frames) or scratch_dev not 256-byte aligned. */
int  ss_griffinlim_samples(int frames);                      /* 256 * (frames - 1); 0 for frames < 4 */
long ss_griffinlim_scratch_bytes(int B, int max_frames);     /* host only; -1 + ss_last_error on bad arguments */
int  ss_mel_to_linear(const float* mel_dev, const double* inv_basis_dev, const int* frames_dev, int B, int max_frames,
                      int n_mels, double floor, double* mag_dev, void* stream);
int  ss_griffinlim(const double* mag_dev, const double* phase0_dev, const int* frames_dev, int B, int max_frames, int n_iter,
                   double momentum, double* wav_dev, void* scratch_dev, long scratch_bytes, void* stream);
/* Non-negative mel inversion: ss_mel_to_linear's floored pseudo-inverse is not consistent with the mel it was given (a mel is the basis
 * applied to a non-negative spectrum, so an exact non-negative solution exists); projected FISTA started from it is.  Per frame, with
 * Bm the [513][n_mels] mel basis, P = inv_basis [n_mels][513] and amp_m = 10^((100 mel_m - 100 + 16) / 20):
 *     x = max(amp . P, 0);  y = x;  t = 1
 *     n_iter times:
 *         r  = y . Bm - amp                      (n_mels values)
 *         g  = r . Bm^T                          (513 values)
 *         xn = max(y - step g, 0)
 *         tn = (1 + sqrt(1 + 4 t^2)) / 2
 *         y  = xn + ((t - 1) / tn) (xn - x);  t = tn;  x = xn
 *     mag = max(x, floor)
 * `step` is an argument (the Python layer passes 1 / lambda_max(Bm^T Bm) from numpy.linalg.eigvalsh; 1 / 1.7994e-3 for the project's bank).
 * float64 throughout.  A bin that no band covers has g = 0 and keeps its starting value.  With n_iter == 0 the result is ss_mel_to_linear's
 * to the bit: the starting product is accumulated in its order, m ascending.  A band's sum y . Bm runs over the band's run of bins in bin
 * order (from 0, amp subtracted last), a bin's sum r . Bm^T over the bands that cover it in band order; one workgroup per frame runs the whole
 * iteration in one launch, no atomics: the same bits on every run.  Shapes, frames_dev and the ragged rules are ss_mel_to_linear's.
 *
 * The basis reaches the kernel PACKED, because every band of a mel filter bank is non-zero on one contiguous run of bins (the project's
 * bank: 941 non-zero weights, longest run 34) and the packed form sits in LDS for the whole iteration, where the dense one (328 KB) could not.
 * ss_mel_nnls_pack (host only) makes it from basis_host [513][n_mels]; the layout, 2 n_mels + W doubles for W non-zero weights:
 *     packed[2 m]     first bin of band m's run      (as a double; 0 for a band with no weight)
 *     packed[2 m + 1] length of the run, 0 .. 513    (as a double)
 *     packed[2 n_mels ...]  the weights: band 0's run in bin order, then band 1's, ... (band m's start at the sum of the lengths before it)
 * It returns the number of doubles the packed form takes and writes them when packed_host is non-NULL and cap_doubles is at least that
 * (NULL or a smaller cap: the size query alone).  It returns -1 and sets ss_last_error for a NULL basis_host, n_mels outside 1 .. 4096, a
 * weight that is negative or not finite, a band whose non-zero weights are not one contiguous run, and a packed size above 3072 doubles: what
 * the kernel's LDS image (packed form, amp, r and y: at most 40980 bytes) is sized for.
 * ss_mel_to_linear_nnls copies packed_dev [packed_doubles] to LDS and clamps every first bin and run length it reads there into the 513 bins
 * and the packed_doubles - 2 n_mels weights, so a corrupt buffer changes numbers, never addresses.  Refused before anything is enqueued, as
 * ss_mel_to_linear and: NULL packed_dev, packed_doubles outside 2 n_mels .. 515 n_mels (it disagrees with n_mels) or above 3072, n_iter
 * outside 0 .. 100000, step not finite and positive. */
long ss_mel_nnls_pack(const double* basis_host /* [513][n_mels] */, int n_mels, double* packed_host, long cap_doubles);
int  ss_mel_to_linear_nnls(const float* mel_dev, const double* inv_basis_dev, const double* packed_dev, long packed_doubles,
                           const int* frames_dev, int B, int max_frames, int n_mels, int n_iter, double step, double floor,
                           double* mag_dev, void* stream);
/* F0-guided harmonic mel inversion and harmonic start phases.  Above about 1 kHz the mel bands are wider than the harmonic spacing, so
 * both routes above hand Griffin-Lim a smooth spectrum with no harmonics in it.  With an F0 track a voiced frame is not 513 unknowns
 * against n_mels equations but one amplitude per harmonic at a known frequency.  The F0 has to BELONG to the mel: 5 % off, the harmonic
 * phases are worse than random ones.  All of it is float64.
 *
 * Constants.  fs = 16000, N = 1024, hop = 256, 513 bins, D = fs / N = 15.625 Hz.  f_top (1000 .. 8000 Hz; the Python layer passes 7600,
 * the bank's fmax) is the highest harmonic frequency.
 *
 * Voiced frames.  f0_hz [B][max_frames] is in Hz (the Python layer converts from ss_pitch_track's ln Hz / -1e10, so the device takes no
 * exponential).  A frame is VOICED when f = f0_hz is finite and 40 <= f <= 1000; anything else -- 0, NaN, negative, out of range -- is
 * unvoiced and never an error.
 *
 * Per voiced frame, with amp_m = 10^((100 mel_m - 100 + 16) / 20), Bm the [513][n_mels] basis and P = inv_basis:
 *   1. H = min(floor(f_top / f), 190) harmonics; harmonic h = 1 .. H sits at the fractional bin p_h = (h f) / D.
 *   2. Atoms.  Dm[k][h] = 512 W(k - p_h), where W(d) = 0.5 s(d) + 0.25 s(d - 1) + 0.25 s(d + 1) for |d| < 2 and 0 otherwise, and
 *      s(x) = sin(pi x) / (pi x), s(0) = 1: the main lobe of the periodic Hann window's transform for a unit cosine (in this form because
 *      the closed form sin(pi d) / (2 pi d (1 - d^2)) cancels near d = +-1).  An atom touches at most the four bins
 *      floor(p_h) - 1 .. floor(p_h) + 2; bins above 512 are dropped.
 *   3. Fit.  a = argmin over a >= 0 of || (Dm a) Bm - amp ||^2 by projected FISTA from a = 0: ss_mel_to_linear_nnls's loop with
 *      A = Bm^T Dm in place of Bm,
 *          a = 0;  y = a;  t = 1
 *          n_iter times:  r = (Dm y) Bm - amp;  g = Dm^T (Bm r);  an = max(y - step g, 0);  tn = (1 + sqrt(1 + 4 t^2)) / 2
 *                         y = an + ((t - 1) / tn) (an - a);  t = tn;  a = an
 *      step = 1 / L with L = (max over h of sum_m A[m][h]) (max over m of sum_h A[m][h]) = ||A||_1 ||A||_inf >= lambda_max(A^T A)
 *      (every entry of A is non-negative), computed per frame on the device; step = 0 when L is 0.  A is never formed:
 *      sum_h A[m][h] = ((Dm 1) Bm)_m and sum_m A[m][h] = (Dm^T (Bm 1))_h, through the loop's own three products.
 *      Orders: a bin's (Dm y)_k runs over the harmonics that cover it in ascending h; a band's sum over its run of bins in bin order (from
 *      0, amp subtracted last); a bin's (Bm r)_k over the bands that cover it in band order; a harmonic's g_h over its four bins in bin order.
 *   4. mag_h = Dm a;  res_m = max(amp_m - (mag_h Bm)_m, 0);  mag_n = max(res P, 0) (m ascending, as ss_mel_to_linear).
 *   5. mag = max(sqrt(mag_h^2 + mag_n^2), floor) and the harmonic share w = mag_h / sqrt(mag_h^2 + mag_n^2), 0 where both are 0.
 *
 * Unvoiced frames.  mag_dev is IN and OUT: the caller first fills it by either route above; unvoiced frames keep what is there and get
 * w = 0, so with an all-unvoiced f0_hz the result is that route's to the bit.
 *
 * Start phases.  The fundamental's phase at the frame centres, in cycles, reduced at every step (hop / fs / 2 = 0.008):
 *     u_0 = 0;   u_i = frac(u_{i-1} + 0.008 (f_{i-1} + f_i))  when frames i - 1 and i are both voiced;
 *     u_i = 0 when frame i is voiced and frame i - 1 is not (and on unvoiced frames);   frac(t) = t - floor(t);   no operation is fused,
 *     so u is what numpy computes, to the bit.
 * Bin k of a voiced frame belongs to harmonic h_k = min(max(rint(k / p_1), 1), H), ties to even; its harmonic phase is
 * phi_h = 2 pi frac(h_k u_i + 0.5 (k mod 2)) -- the half cycle is e^{-i pi k}: the frame starts 512 samples before its centre.  Then
 *     phase0 = arg(w e^{i phi_h} + sqrt(max(1 - w^2, 0)) e^{i phi_rand}),   phi_rand = rand_phase_dev's element (NULL: 0).
 * Unvoiced frames, and elements whose sum is exactly 0, keep phi_rand.  ss_griffinlim is unchanged: it receives mag and phase0.
 *
 * Kernel.  One workgroup of 256 threads per (frame, row) runs the whole fit in one launch with no global traffic inside the loop, no
 * atomics and every sum in one fixed order: the same bits on every run.  The basis sits in LDS in ss_mel_nnls_pack's form -- the same
 * buffer, the same 3072-double cap and the same clamping, so a corrupt buffer changes numbers, never addresses -- beside amp, r, the
 * 513-bin model, its gradient and the harmonics' atoms (41804 bytes for 80 bands at the cap, at most 53452).  u is a serial recurrence:
 * one wave per row runs it in registers, 64 frames per load; the fill runs per (frame, row) over 513 bins.
 * Shapes: mel [B][max_frames][n_mels] f32; f0_hz [B][max_frames]; mag, share, rand_phase, phase0 [B][max_frames][513].  frames_dev and the
 * ragged rules are ss_mel_to_linear's: row b is bit for bit the result of running it alone at min(max(frames[b], 4), max_frames) frames;
 * nothing at or beyond them is read in mel, f0_hz, share or rand_phase (they may hold NaN); there mag is left as the caller's route wrote
 * it, and share and phase0 are zeros.  No engine needed, no allocation inside, asynchronous on `stream`.
 * Refused before anything is enqueued, with a message that names the argument: null required pointers (rand_phase_dev may be NULL),
 * B < 1, max_frames outside 4 .. SS_MAX_EVAL_FRAMES, n_mels outside 1 .. 4096, packed_doubles outside 2 n_mels .. 515 n_mels or above 3072,
 * f_top outside 1000 .. 8000 or NaN, n_iter outside 0 .. 100000, negative or NaN floor, scratch_bytes below
 * ss_harmonic_phase_scratch_bytes(B, max_frames) or scratch_dev not 256-byte aligned. */
int  ss_mel_to_linear_harmonic(const float* mel_dev, const double* f0_hz_dev, const double* inv_basis_dev, const double* packed_dev,
                               long packed_doubles, const int* frames_dev, int B, int max_frames, int n_mels, double f_top, int n_iter,
                               double floor, double* mag_dev /* in/out */, double* share_dev /* out */, void* stream);
long ss_harmonic_phase_scratch_bytes(int B, int max_frames); /* host only; -1 + ss_last_error on bad arguments */
int  ss_harmonic_phase(const double* f0_hz_dev, const double* share_dev, const double* rand_phase_dev, const int* frames_dev, int B,
                       int max_frames, double f_top, double* phase0_dev /* out */, void* scratch_dev, long scratch_bytes, void* stream);
/* test hook: the recurrence alone, u_dev [B][max_frames] (zeros on unvoiced frames and behind a row's own) */
int  ss_op_harmonic_u(const double* f0_hz_dev, const int* frames_dev, int B, int max_frames, double* u_dev, void* stream);
/* test hooks, each half alone: spec [B][max_frames][513][2] (re, im); ss_op_istft takes the same scratch as ss_griffinlim */
int  ss_op_stft (const double* wav_dev,  const int* frames_dev, int B, int max_frames, double* spec_dev, void* stream);
int  ss_op_istft(const double* spec_dev, const int* frames_dev, int B, int max_frames, double* wav_dev,
                 void* scratch_dev, long scratch_bytes, void* stream);

/* ---- conversion scores: mel-cepstral distortion along a dynamic-time-warping (DTW) path, and F0 / voicing error along the same path ----
 * Nothing to mirror: the reference never scores a conversion.  What a converted utterance is compared with -- the source, or a recording of
 * the target speaker -- has another length (a rhythm conversion changes it by construction), so the comparison runs along an alignment.
 *
 * Cepstra.  mel f32 [B][max_t][n_mels], dct f64 [n_ceps][n_mels] (the host computes it), out f64 [B][max_t][n_ceps]:
 *     c[b][t][d] = sum_m dct[d][m] * (double)mel[b][t][m],  m = 0, 1, ... in order; multiply-adds may be fused.
 * The Python layer passes rows d = 1 .. n_ceps of the orthonormal DCT-II, sqrt(2 / n_mels) cos(pi d (m + 1/2) / n_mels); row 0, the level,
 * is left out.  Rows at or beyond len[b] are exact zeros.
 *
 * Frame distance.  d(i, j) = scale * sqrt(sum_k (fx[i][k] - fy[j][k])^2): k runs in order, the root comes after the sum and `scale` is
 * applied after the root.  This project's mels are S = (dB + 100) / 100, so ln|A| = (100 S - 84) ln 10 / 20 and the usual
 * (10 / ln 10) sqrt(2 sum dc^2) of the log-amplitude cepstra is scale = 50 sqrt(2) on the cepstra of S; the Python layer passes that value.
 *
 * DTW.  Steps (1,1), (1,0), (0,1), each of weight 1; both ends are fixed.
 *     D(0,0) = d(0,0);   D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)),   predecessors outside the lattice are absent.
 * The candidates are tried in that order with a strict <: on a tie the diagonal wins, then (i-1, j).  Backtrack from (Tx-1, Ty-1) to (0,0);
 * the path is reported first step to last as (i, j) pairs, P is its length, max(Tx, Ty) <= P <= Tx + Ty - 1;
 * total = D(Tx-1, Ty-1) and mcd = total / P.  There is no band and no slope constraint.
 *
 * F0 along the path.  f0x [B][max_tx], f0y [B][max_ty] follow ss_pitch_track's convention: ln Hz, -1e10 for unvoiced frames; a frame is
 * voiced when its value is finite and > -1e9.  Over the P steps (lx = f0x[i], ly = f0y[j]): n_vv counts the steps where both frames are
 * voiced, n_vu those where exactly one is;
 *     f0_rmse_cents = (1200 / ln 2) sqrt(sum (lx - ly)^2 / n_vv)            NaN when n_vv == 0
 *     f0_corr       = sxy / sqrt(sxx syy), the Pearson correlation of (lx, ly) over the both-voiced steps: the means first, then the
 *                     centred sums sxx, syy, sxy                              NaN when n_vv < 2 or sxx or syy is 0
 *     vuv_error     = n_vu / P
 * Sums run in path order, one term at a time.
 *
 * Float64 throughout, no atomics: the same bits on every run, and a pair inside a ragged batch gives, bit for bit, what it gives alone (D
 * depends on one add per cell, so the kernel's tiling cannot show).  No engine needed, no allocation inside, asynchronous on `stream`.
 * Shapes: fx [B][max_tx][dim], fy [B][max_ty][dim]; out [B][3] = total, P, mcd; path i32 [B][max_tx + max_ty - 1][2], entries beyond P
 * are -1; path_len i32 [B]; stats out [B][5] = n_vv, n_vu, f0_rmse_cents, f0_corr, vuv_error.  path_dev and path_len_dev of the DTW call are
 * both NULL (totals only) or both given.  The statistics call clamps every path entry into the lattice and path_len into
 * 0 .. max_tx + max_ty - 1 (NULL: that many), so a corrupt path changes numbers, never addresses.
 * len_dev / tx_dev / ty_dev i32[B] (NULL: every row is full): row b is the result of running that pair alone at min(max(len[b], 1), max)
 * frames -- a length outside 1 .. max spoils that row only; frames at or beyond it are never read (they may hold NaN).
 * The scratch (backpointers of 2 bits a cell, and one boundary row of D a pair):
 *     B * (align256(max_tx * ceil(max_ty / 4)) + align256(8 max_ty)) bytes, in long arithmetic.
 * Refused before anything is enqueued, with a message that names the argument: null required pointers, B outside 1 .. 65535, max_t / max_tx /
 * max_ty outside 1 .. SS_MAX_EVAL_FRAMES, n_mels outside 1 .. 128, n_ceps or dim outside 1 .. 40, scale not finite or <= 0, path_dev and
 * path_len_dev not both NULL or both given, scratch_bytes below what the scratch query returns, scratch_dev not 256-byte aligned. */
int  ss_mel_cepstra(const float* mel_dev, const int* len_dev, int B, int max_t, int n_mels, const double* dct_dev, int n_ceps,
                    double* out_dev, void* stream);
long ss_dtw_scratch_bytes(int B, int max_tx, int max_ty);     /* host only; -1 + ss_last_error on bad arguments */
int  ss_dtw(const double* fx_dev, const int* tx_dev, const double* fy_dev, const int* ty_dev, int B, int max_tx, int max_ty, int dim,
            double scale, double* out_dev /* [B][3] total, P, mcd */, int* path_dev /* [B][max_tx+max_ty-1][2] or NULL */,
            int* path_len_dev /* [B] or NULL */, void* scratch_dev, long scratch_bytes, void* stream);
int  ss_path_f0_stats(const int* path_dev, const int* path_len_dev, const double* f0x_dev, const double* f0y_dev, int B, int max_tx,
                      int max_ty, double* out_dev /* [B][5] n_vv, n_vu, f0_rmse_cents, f0_corr, vuv_error */, void* stream);

/* ---- waveform scores: short-time objective intelligibility (STOI) and its extended form (ESTOI) ----
 * Nothing to mirror: the reference never scores a waveform.  STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016)
 * compare a degraded waveform y with a TIME-ALIGNED clean one x.  Float64 throughout.  Both signals are at 10 kHz and have n samples.
 * eps = 2^-52.  What follows is the whole definition, the order of every sum included; a sum "in order" adds one term at a time, index
 * ascending, and multiply-adds are not fused.
 *
 * Constants.  Frame 256, hop 128, transform 512 points (257 bins).  J bands (15 for the project), segment length N = 30 frames,
 * beta = -15 dB, dynamic range 40 dB.  Window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0 .. 255 (numpy.hanning(258)[1:-1]), evaluated
 * on the host as 0.5 - 0.5 * cos(2.0 * pi * (i + 1) / 257.0) with the C library's cosine.
 *
 * Silent-frame removal.  Frames f = 0 .. F-1 start at 128 f, F = floor((n - 256) / 128) + 1 (F = 0 when n < 256).
 *     e_f = 20 log10(sqrt(sum_i (w[i] x[128 f + i])^2) + eps),   i in order.
 * Frame f is kept when e_f > max_f e_f - 40.  The K kept frames, in order (inv[c] is the c-th kept frame), are overlap-added at hop 128 into
 * x' of 128 (K - 1) + 256 samples, and y' is built the same way with x's mask.  The overlap-add is a gather: with c = s / 128, r = s % 128,
 *     x'[s] = w[r + 128] x[128 inv[c-1] + r + 128]  +  w[r] x[128 inv[c] + r],
 * the earlier frame's term first; a term whose frame index is outside 0 .. K-1 is absent (the other term is then the sample, unrounded).
 * The window is applied once and there is no division by a window sum.
 *
 * Band envelopes.  Transform frames of x' and y' start at 128 m for m = 0 .. M-1, M = K - 1: the starts strictly below len - 256, as in the
 * authors' published code (the last full frame is left out).  Each frame is windowed by w, zero-padded to 512 and transformed;
 *     X[j][m] = sqrt(sum_{k in [lo_j, hi_j)} (re_k^2 + im_k^2)),   k in order, each term the sum of its two squares.
 * lo and hi are inputs.  The Python layer passes third-octave bands: cf_j = 150 * 2^(j/3), edges cf_j 2^(-1/6) and cf_j 2^(+1/6), each mapped
 * to the nearest of the bin frequencies k * 10000 / 512:
 *     lo = 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174      hi = 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219
 *
 * Segments.  S = M - N + 1; segment s is frames s .. s+29 of both envelopes, X_j and Y_j its rows (t = 0 .. 29).
 * "Normalising" a vector v of c elements: mean = (sum v, in order) / c; v <- v - mean; v <- v / (sqrt(sum v^2, in order) + eps).
 *   STOI, per band j:  alpha = sqrt(sum_t X_j[t]^2) / (sqrt(sum_t Y_j[t]^2) + eps);   Y'_j[t] = min(alpha Y_j[t], X_j[t] (1 + 10^(15/20)));
 *         X_j and Y'_j are normalised over t;   d_{s,j} = sum_t X_j[t] Y'_j[t];   d_s = (sum_j d_{s,j}) / J.         Every sum in order.
 *   ESTOI:  every row of both blocks is normalised over t; then every column of both is normalised over j;
 *         c_t = sum_j X_j[t] Y_j[t];   d_s = (sum_t c_t) / N.                                                          Every sum in order.
 * score = (sum_s d_s) / S, s in order.  When S < 1 (fewer than 31 kept frames) the score is NaN and S is reported as 0; the constant the
 * published code returns in that case is deliberately not copied.
 *
 * What this does NOT claim: parity with pystoi is unpinned (that package adds random noise in its normalisation and resamples with its own
 * filter; the Python layer here resamples with ss_resample).
 *
 * Ragged batches.  x_dev, y_dev [B][max_n]; n_dev i32[B] (NULL: every row is full): row b is the result of running that pair alone at
 * min(max(n[b], 1), max_n) samples, to the bit -- a length outside 1 .. max_n spoils that row only; samples at or beyond it are never
 * read (they may hold NaN).  No atomics, every sum in a fixed order: the same bits on every run.  No engine needed, no allocation inside,
 * asynchronous on `stream`.  band_lo / band_hi are HOST arrays of n_bands ints.  out [B][3] = score, S, K as doubles.
 * The scratch, with F = floor((max_n - 256) / 128) + 1, L = 128 (F - 1) + 256, M = F - 1, S = max(M - 29, 0), every part rounded up to 256
 * bytes: frame levels 8 B F, the inverse map 4 B F, K 4 B, x' and y' 8 B L each, two envelopes 8 B 32 M each, d_s 8 B S.  Every index read
 * back from it (inverse map, K) is clamped into the row's own frames: a corrupt scratch changes numbers, never addresses.
 *
 * Test hooks.  ss_op_stoi_compact runs the first three stages: e [B][F] (-inf behind a row's frames), inv i32 [B][F] (-1 behind the K kept
 * frames), k i32 [B], x' and y' [B][L] (zeros behind a row's samples).  With from_map = 1 the energies and the mask are skipped: inv_dev and
 * k_dev are INPUTS, read with the clamps above, and e_dev may be NULL.  ss_op_stoi_bands gives the envelopes [B][n_bands][Mmax] of sig_dev
 * [B][max_len] (len_dev i32[B] or NULL, clamped to 1 .. max_len; Mmax = ceil((max_len - 256) / 128); zeros at and behind a row's M frames).
 *
 * Refused before anything is enqueued, with a message that names the argument: null required pointers, B outside 1 .. 65535, max_n below
 * 256 (max_len below 257) or so large that the scratch does not fit a long, n_bands outside 1 .. 32, a band with lo < 0, hi > 257 or
 * lo >= hi, extended or from_map outside 0 / 1, scratch_bytes below what the scratch query returns, scratch_dev not 256-byte aligned. */
long ss_stoi_scratch_bytes(int B, int max_n);                 /* host only; -1 + ss_last_error on bad arguments */
int  ss_stoi(const double* x_dev, const double* y_dev, const int* n_dev, int B, int max_n, const int* band_lo, const int* band_hi,
             int n_bands, int extended, double* out_dev /* [B][3]: score, S, K */, void* scratch_dev, long scratch_bytes, void* stream);
int  ss_op_stoi_compact(const double* x_dev, const double* y_dev, const int* n_dev, int B, int max_n, int from_map,
                        double* e_dev /* [B][F] */, int* inv_dev /* [B][F] */, int* k_dev /* [B] */, double* xp_dev /* [B][L] */,
                        double* yp_dev /* [B][L] */, void* stream);
int  ss_op_stoi_bands(const double* sig_dev, const int* len_dev, int B, int max_len, const int* band_lo, const int* band_hi, int n_bands,
                      double* env_dev /* [B][n_bands][Mmax] */, void* stream);

/* Batch producer on the GPU side (replaces the host loop of MyCollator.__call__, reference data_loader.py:101-128, for a
 * corpus kept resident in HBM): utterance b of the batch is rows [row0[b], row0[b] + len[b]) of the concatenated corpus
 * mel_cat [rows, n_mel] / f0_cat [rows]; the host only draws the crops (same generator calls, same order as the reference).
 * mel [B,T,n_mel] = clip(crop, 0, 1) zero-padded, f0 [B,T] = crop padded with -1e10, emb [B,emb_dim] = emb_tab[item[b]].
 * All pointers are device pointers; row0 is int64, len / item int32.  No engine needed. */
int ss_collate(const float* mel_cat_dev, const float* f0_cat_dev, const float* emb_tab_dev, const long* row0_dev,
               const int* len_dev, const int* item_dev, int B, int T, int n_mel, int emb_dim, float* mel_dev, float* f0_dev,
               float* emb_dev, void* stream);

/* Asynchronous failures.  The engine keeps a STATUS WORD that kernels set and no step clears:
 *   SS_STATUS_ABORT   a persistent recurrence kernel's bounded wait expired on this device (e.g. the GPU is shared and the
 *                     256-workgroup grid was not co-resident): that step's gradients are garbage;
 *   SS_STATUS_REMOTE  another data-parallel rank reported the same through the gradient arena's status slot (the last four
 *                     floats of the arena; the all-reduce sums it);
 *   SS_STATUS_RANGE   a parameter is not finite or reached |p| >= 2048, outside what the fixed scale of the WEIGHTS' fp16 x 2
 *                     split is valid for (activations and gradients carry data-dependent scales and have no such limit).
 * While it is non-zero the Adam kernel SKIPS the update on the device (parameters, moments and step counter untouched --
 * no host round trip is involved), every later ss_*_forward / ss_*_train_step / ss_adam_step returns an error without
 * enqueueing anything, and ss_check() keeps failing until ss_clear_abort().  ss_check synchronises `stream`;
 * ss_status() reads the word without synchronising.
 * LOCKSTEP mode (data parallel; switched on by ss_comm_init with world > 1, or by ss_set_lockstep for ranks that exchange their
 * gradients outside the engine): the entry points do NOT refuse -- the word is set asynchronously, ranks would notice it at different
 * iterations and the survivors would wait in a collective for ever.  Every rank keeps enqueueing (the device-side skip protects the
 * weights, the status slot carries the failure to every rank within the same step) and learns of it from ss_check(), which all
 * ranks call at the same iteration; all of them then either stop or call ss_clear_abort() and go on together. */
#define SS_STATUS_ABORT 1u
#define SS_STATUS_REMOTE 2u
#define SS_STATUS_RANGE 4u
int ss_check(ss_engine* e, void* stream);
unsigned ss_status(const ss_engine* e);
int ss_clear_abort(ss_engine* e, void* stream);
int ss_set_lockstep(ss_engine* e, int on);

/* ---- test / profiling hooks ---- */
/* C[M,N] = A . B^T style fp32 MFMA GEMM used by every contraction on the path (flags: 1 = A stored [K,M], 2 = B stored [K,N], 8 = bf16-rounded
 * operands, 16 = fp16 x 2 split).  Any base address and row stride: operands on 16-byte aligned bases with strides that are multiples of 4 floats
 * take the vector kernels, everything else the scalar instances of the fp32-MFMA kernel; c_dev rows are ldc >= N floats apart and nothing
 * outside the M x N extent is written.  Flag 1 without flag 2 (no contraction of the step has that form) runs on the fp32-MFMA kernel in every
 * arithmetic mode; flag 8 rounds the operands to bf16 on whichever kernel runs.  ksplit > 1 ADDS the partial products into C (atomics): C must
 * hold zeros (or the value to accumulate onto) on entry. */
int ss_op_gemm(const float* a_dev, long lda, const float* b_dev, long ldb, float* c_dev, long ldc, const float* bias_dev,
               int M, int N, int K, int flags, int ksplit, void* stream);
/* One bidirectional LSTM recurrence on haloed slabs (speechsplit_amd/csrc/kernels.h): gates [B,T+4,8H] holds
 * x.W_ih^T + b on entry and the activated gates on exit; out / csave [B,T+4,2H]; whh_* [4H,H].  For H <= 32 not a power of
 * two the rows of out / csave / d_out are 2H rounded up to a multiple of 4 floats apart (columns past 2H untouched).  H <= 32 runs the
 * single-launch kernel, H in {64,128,256,512} one launch per time step and needs scratch of at least
 * 8*H*H + 4*ceil16(B)*H floats (forward) / 8*H*H + 16*ceil16(B)*H + 2*B*H floats (backward).  H in {256,512} with
 * 2*ceil(B/16)*(H/16) <= 256 runs as ONE persistent launch (the engine's schedule) when, for the backward, scratch also
 * holds its exchange tiles and flags: 4*ceil(B/16)*(H/16)^2*1024 + 8192 bytes (the hook zeroes them: the tiles carry step tags). */
int ss_op_lstm_fwd(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, float* out_dev, float* csave_dev,
                   float* scratch_dev, long scratch_floats, int B, int T, int H, void* stream);
/* ss_op_lstm_fwd over a ragged batch (len_dev i32[B], see ss_g3_forward_ragged; NULL: ss_op_lstm_fwd itself): row b's recurrence covers
 * frames [0, len[b]) -- the reverse direction starts at frame len[b] - 1 from the zero state -- and out / csave hold zeros for t >= len[b].
 * The gates rows t >= len[b] may hold anything on entry (NaN included) and are unspecified on exit.  Forward only. */
int ss_op_lstm_fwd_ragged(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, float* out_dev, float* csave_dev,
                          float* scratch_dev, long scratch_floats, const int* len_dev, int B, int T, int H, void* stream);
/* BPTT of the same: d_out [B,T+4,2H]; gates is replaced by the pre-activation gradients. */
int ss_op_lstm_bwd(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, const float* d_out_dev,
                   const float* csave_dev, float* scratch_dev, long scratch_floats, int B, int T, int H, void* stream);
/* The two persistent recurrences (H in {256,512}) launched with every option the engine passes them.  Slabs, weights and d_out as for
 * ss_op_lstm_fwd / _bwd.  No fall-back: a shape the persistent kernels do not take, an option without its operand, a misplaced image or a
 * short scratch is refused before anything is enqueued.  scratch: 8*ceil(B/16)*(H/32)*1024 + 8192 bytes (forward) /
 * 4*ceil(B/16)*(H/16)^2*1024 + 8192 bytes (backward), 16-byte aligned -- the exchange buffer and the sync words, which the hooks zero.
 * Every optional pointer may be NULL (option off).
 *   forward
 *     xc_dev / xf     the layer's input repeats in blocks of xf frames (xf >= 1, T % xf == 0): the pre-activations are given once per block,
 *                     [B][T/xf][8H], and the gates slab is only written (what it holds on entry is not read).
 *     out_img_dev     the operand image of `out`, written beside it: the geometry of the out slab [B][T+4][2H]; real rows only (halo rows
 *                     and the rows of padded utterances are not written).  img_bf16 == 0: format v2 with the scale 16 (what
 *                     ss_op_split_image makes of out), base 32-byte aligned; img_bf16 != 0: the plain bf16 tensor (2 bytes per element,
 *                     round to nearest even), base 8-byte aligned.
 *     hi_only         the recurrent product from the high fp16 pieces of h and W_hh alone (the 16-bit data path).
 *     len_dev         i32[B], a ragged batch as for ss_op_lstm_fwd_ragged; out, csave and the image hold zeros for t >= len[b].
 *   backward
 *     amax_dev        one word: receives max |pre-activation gradient| over the real rows by an atomic max on the float's bit pattern, so
 *                     it only ever grows: zero it first.
 *     gbias_f_dev /   [2][4H] each, (b_ih, b_hh) gradient accumulators of the forward / reverse direction: the sum over utterances and
 *     gbias_b_dev     time of the pre-activation gradients is ADDED to both halves (one float64 sum per tile of 16 utterances, f32 atomics).
 *     dgs_dev / xf    the pre-activation gradients additionally summed per block of xf frames, [B][T/xf][8H], every element overwritten;
 *                     fp32 sums in walking order (forward direction: t descending, reverse direction: ascending).
 *     dimg_dev        the pre-activation gradients once more as a plain bf16 tensor of the gates slab's geometry [B][T+4][8H] (real rows
 *                     only), base 8-byte aligned.  img_only != 0 (needs dimg_dev): the fp32 slab is NOT written and keeps the forward's
 *                     activated gates; every other output is as without it.
 *     hi_only         as the forward's, for da . W_hh. */
int ss_op_lstm_seq_fwd(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, float* out_dev, float* csave_dev, float* scratch_dev,
                       long scratch_floats, const float* xc_dev, int xf, float* out_img_dev, int img_bf16, int hi_only, const int* len_dev,
                       int B, int T, int H, void* stream);
int ss_op_lstm_seq_bwd(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, const float* d_out_dev, const float* csave_dev,
                       float* scratch_dev, long scratch_floats, float* amax_dev, float* gbias_f_dev, float* gbias_b_dev, float* dgs_dev, int xf,
                       float* dimg_dev, int img_only, int hi_only, int B, int T, int H, void* stream);
/* Test hook for the fused weight / bias gradient kernel of the encoder BLSTMs (csrc/lstm_wgrad.hip; hidden size <= 32): from the pre-activation
 * gradients dg [R][8H], the layer input x [R][In] (row stride x_ld) and the layer output hout [R][2H] (haloed slabs flattened to R rows, halo
 * rows zero) ACCUMULATE dW_ih [2][4H][In], dW_hh [2][4H][H] and the bias gradients gb [2][2][4H] (b_ih, b_hh per direction).  scratch:
 * >= 16 * 4096 * tiles + roundup(tiles, 64) floats with tiles = ceil(8H / 64) * (ceil(In / 64) + (4H % 64 == 0 ? 1 : 2)) -- the partial
 * slabs and one arrival counter per tile; H in 1..32, hout rows 2H apart. */
int ss_op_lstm_wgrad(const float* dg_dev, const float* x_dev, long x_ld, const float* hout_dev, float* gwih_dev, float* gwhh_dev, float* gb_dev,
                     float* scratch_dev, long scratch_floats, long R, int H, int In, void* stream);
/* The GroupNorm + ReLU kernels (speechsplit_amd/csrc/elementwise.hip; 16 channels per group, eps 1e-5 inside the square root, biased variance
 * over 16 x T) on the CALLER's haloed slabs, in every form the engine launches.  The hooks call the kernel launchers and nothing else: no
 * convolution, no engine, no copy into private slabs.  A slab pointer is slab row 0: frame t of utterance b is row t + 2, at
 * p + b * bs + (t + 2) * ld floats, with ld >= C, ld % 4 == 0, bs % 4 == 0 and a 16-byte aligned base -- so a block inside a wider slab is
 * its first column with the slab's strides.  The two halo rows on either side of an INPUT slab (x, and dy without the scatter form) are zero;
 * the halo rows of the outputs y (plain and ragged form) and dy are neither read nor written.  gamma / beta [C] 16-byte aligned,
 * stats [B][C/16][2] = (mean, rstd) per group, C % 64 == 0, B >= 1, T >= 1.  Every optional pointer may be NULL (option off).
 * Refused before anything is enqueued, each with its own ss_last_error text: a null pointer, C % 64 != 0, T < 1, T > 256 with a backward, a
 * mask, a gather or a scatter, T > SS_MAX_EVAL_FRAMES, a short or misaligned scratch, a stride or base that breaks the rules above, an
 * incomplete plan, P outside 1 .. 258, and an image that is misplaced (y_ld % 8, y_bs % 8, base alignment) -- the launcher would drop such
 * an image silently; the hook never returns success without the image it was asked for.
 *   ss_op_gn_relu_scratch  bytes of scratch ss_op_gn_relu_fwd needs: 0 for T <= 256, else 2 * B * (C/16) * ceil(T/64) float64 words (8-byte aligned).
 *   ss_op_gn_relu_fwd
 *     plain form     y rows [2, 2 + T) = relu(gamma * (x - mean) * rstd + beta), stats written.  T <= 256: one register-resident launch;
 *                    T > 256: three chunked launches with float64 partial sums in scratch_dev.
 *     len_dev        i32[B], the ragged form: the statistics of row b run over its L = min(max(len[b], 0), T) frames, x rows t >= L are never
 *                    read (they may hold NaN), y rows t >= L are zeros.  A row with len[b] == 0 gives zeros in y and disturbs no other row;
 *                    its stats entries are then NaN (0 * inf: the mean of no frames) -- harmless, eval mode has no backward.
 *     i0_dev, lam_dev [B][P], nrows_dev [B], P
 *                    the gather form (T <= 256; excludes len_dev): y is the RESAMPLED output, P real rows at y rows [2, 2 + P), row r <
 *                    nrows[b] = (1 - lam[r]) * act[i0[r]] + lam[r] * act[i0[r] + 1] (three roundings; act row T reads as zeros), rows r >=
 *                    nrows[b] zeros; the normalised slab itself is not written.  stats as the plain form's, bit for bit.
 *     y_img_dev      (gather form only) the image of y, in the geometry of the y slab (real rows only): img_bf16 == 0 format v2 split with
 *                    *img_scale_dev (NULL: 16), base 32-byte aligned; img_bf16 != 0 the plain bf16 tensor (2 bytes per element, round to
 *                    nearest even), base 16-byte aligned.  Both need y_ld % 8 == 0 and y_bs % 8 == 0.
 *   ss_op_gn_relu_mask     mask [B][T][C] dense = 1.0f where the GroupNorm output z > 0, from x and stats (the branch every kernel here takes).
 *   ss_op_gn_relu_bwd      T <= 256.  dy (gradient of the ReLU output) is replaced in place, real rows only, by the gradient of x; the sums over
 *                    utterances and time of d_gamma, d_beta and d_x are ADDED to g_gamma_dev, g_beta_dev, g_bias_dev [C] (f32 atomics).
 *     amax_dev       one word: receives max |dx| by an atomic max on the float's bit pattern, so it only ever grows: zero it first.
 *     part_dev       [B][3][C] floats of scratch, used only under ss_tune("deterministic", 1) (ignored otherwise, as in the launcher): the
 *                    per-utterance sums go there and are added to the accumulators in utterance order, so that repeats agree in every bit.
 *     lam_dev [B][P], start_dev [B][T+1], P, src_dev, src_ld, src_bs
 *                    the scatter form: dy on entry is NOT read; the gradient of the ReLU output is the adjoint of the gather taken from src,
 *                    the gradient of the resampled output (a slab of P real rows, as the gather form's y):
 *                    dy[t] = sum_{i0[r] == t} (1 - lam[r]) src[r] + sum_{i0[r] == t - 1} lam[r] src[r] over r < nrows.
 *     dy_img_dev     dx once more as a plain bf16 tensor of the dy slab's geometry (real rows only; round to nearest even), base 8-byte
 *                    aligned, dy_ld % 8 == 0 and dy_bs % 8 == 0.
 * PLAN CONTRACT.  Plans are device-resident: the hooks cannot validate their contents, the caller must.  0 <= i0[b][r] < T and i0 non-decreasing
 * in r for r < nrows[b]; 0 <= nrows[b] <= P <= 258; start[b][i] = number of rows r < nrows[b] with i0[b][r] < i, for i in 0 .. T (so it is
 * non-decreasing and start[b][T] = nrows[b] <= P), as csrc/interp.hip defines it.  The Python wrappers assert this on the host. */
long ss_op_gn_relu_scratch(int B, int T, int C);
int ss_op_gn_relu_fwd(const float* x_dev, long x_ld, long x_bs, float* y_dev, long y_ld, long y_bs, const float* gamma_dev, const float* beta_dev,
                      float* stats_dev, const int* len_dev, const int* i0_dev, const float* lam_dev, const int* nrows_dev, int P, float* y_img_dev,
                      const float* img_scale_dev, int img_bf16, void* scratch_dev, long scratch_bytes, int B, int T, int C, void* stream);
int ss_op_gn_relu_mask(const float* x_dev, long x_ld, long x_bs, const float* gamma_dev, const float* beta_dev, const float* stats_dev,
                       float* mask_dev, int B, int T, int C, void* stream);
int ss_op_gn_relu_bwd(const float* x_dev, long x_ld, long x_bs, float* dy_dev, long dy_ld, long dy_bs, const float* gamma_dev, const float* beta_dev,
                      const float* stats_dev, float* g_gamma_dev, float* g_beta_dev, float* g_bias_dev, float* amax_dev, float* part_dev,
                      const float* lam_dev, const int* start_dev, int P, const float* src_dev, long src_ld, long src_bs, float* dy_img_dev, int B,
                      int T, int C, void* stream);
/* The kernels that stand between the heavy families in a training step (speechsplit_amd/csrc/elementwise.hip, input_grads.hip), engine-free
 * and on the CALLER's memory: the hooks hand their views to the kernel launchers and do nothing else -- no engine, no copy into private
 * buffers, so memory around an operand is the caller's to watch.  A VIEW is (p, ld, bs): row t of utterance b starts at p + b * bs + t * ld
 * floats, p being frame 0 (no halo is added).  Every refusal is made before anything is enqueued, each with its own ss_last_error text.
 *   ss_op_mse_loss   loss = mean over B T C of (out - tgt)^2 (float64 sum of 8 B fp32 block partials, rounded once);
 *                    d_out = (out - tgt) * (float(2 / (B T C)) * grad_scale), C columns of every row, nothing else written.
 *                    partials_dev: at least 8 B floats of scratch; loss_dev: one float.  Refused: a null pointer, B / T / C below 1, a row
 *                    stride below C.
 *   ss_op_ce_loss    softmax cross-entropy of logits [B][T][C] (a view) against tgt_dev i32 [B][T] dense, mean over the B T rows;
 *                    d_out = (softmax - onehot) * (float(1 / (B T)) * grad_scale).  partials_dev: at least B T floats (the per-row losses);
 *                    loss_dev: one float.  The result depends on a row's logits only through their differences from the row maximum
 *                    (shift-invariant: logits near 1000 are as accurate as logits near 0).  TARGETS MUST LIE IN [0, C): they are read on the
 *                    device and NOT CHECKED there -- an out-of-range target reads outside the row.  Refused: a null pointer, B / T / C
 *                    below 1, a row stride below C.
 *   ss_op_colsum_scratch_doubles(cols)
 *                    float64 words of scratch the chunked column sum needs: (ceil(1024 / nb) + 1) * nb * 64 with nb = ceil(cols / 64);
 *                    0 for cols < 1.
 *   ss_op_colsum     column sums of in [R][cols] (row stride ld), float64 accumulation in a fixed order, ADDED to the outputs (one fp32
 *                    rounding of the sum, one of the addition).  two_dir == 0: cols = C, o0[c] += sum (o1 .. o3 must be NULL).
 *                    two_dir != 0: cols = 2 C, columns [0, C) go to o0 and (if not NULL) o1, columns [C, 2 C) to o2 and (if not NULL) o3
 *                    -- the (b_ih, b_hh) pairs of a BLSTM's two directions.  part_dev / ctr_dev both NULL: the single-chunk form, one
 *                    workgroup per 64 columns.  Both given: up to min(ceil(1024 / nb), ceil(R / 16)) row chunks per column block hand
 *                    float64 partials through part_dev; ctr_dev holds one arrival counter per column block, ZERO on entry and zero again
 *                    when the launch retires, used by nobody else meanwhile.  The sums are the same bits whatever the arrival order.
 *                    Refused: a null in / o0, two_dir without o2, R or C below 1, ld < cols, one of part / ctr without the other,
 *                    part_doubles below ss_op_colsum_scratch_doubles(cols), ctr_words below ceil(cols / 64), a misaligned scratch.
 *   ss_op_dec_in     the decoder input from up to four encoder BLSTM output slabs (ss_code_src: o [B][T+4][ld_i] haloed, the 2 H real
 *                    columns first) and the speaker rows emb [B][emb_dim] (emb_dim 0: none).  Columns [col, col + H) of frame t are the
 *                    forward half at the LAST frame of t's block of freq frames, [col + H, col + 2 H) the backward half at its FIRST frame;
 *                    columns [emb_col, emb_col + emb_dim) the speaker row; every other column of the ld is written zero.  f == 0: the
 *                    slab form, dst [B][T+4][ld], rows [2, 2 + T) written, halo rows untouched.  f > 0: the compact form, dst [B][T/f][ld],
 *                    one row per block (every source's freq == f).  Column ranges must not overlap (not checked).
 *   ss_op_dec_in_grad  the adjoint: d_o [B][T+4][ld_i] of every source gets, in its 2 H real columns of rows [2, 2 + T) and nowhere else,
 *                    the sum over the block's freq frames (fp32, frames ascending) of d_in's columns at the one frame of the block where
 *                    the half was sampled, and zero at every other frame.  f == 0: d_in is the slab [B][T+4][ld]; f > 0: d_in is
 *                    [B][T/f][ld] and already holds the sums.
 *   ss_op_dec_in_codes_grad  the adjoint with respect to DENSE codes (what ss_*_decode_backward runs; up to three sources in one launch):
 *                    d_o of source i is here the dense code gradient [B][T/freq_i][2 H_i] (ld_i is only checked to be >= 2 H_i, o is not
 *                    read) and gets, per element, the sum over the block's freq_i frames (fp32, frames ascending, no atomics) of d_in's
 *                    column col_i + c.  f == 0: d_in is the slab [B][T+4][ld]; f > 0: d_in is [B][T/f][ld] and already holds the sums.
 *                    Nothing outside the dense code gradients is written; of d_in only rows [2, 2 + T) and the sources' columns are read.
 *   ss_op_dec_in_codes  ss_op_dec_in by way of dense codes (up to three sources): export the codes into codes_dev (at least the sum over
 *                    the sources of B (T / freq_i) 2 H_i floats, each rounded up to 4; 16-byte aligned), then build dst from them.
 *                    Refused by all three: a null pointer, nsrc outside 1 .. 4 (codes: 3), B / T below 1, T % freq_i != 0, columns
 *                    beyond ld, ld_i < 2 H_i, f that does not divide T, the compact form with a freq_i != f.
 *   ss_op_spk_grad   out [B][E] = sum_g (sum over rows r of dg[b][r][g]) * W(g, col0 + j), g < 2 H4, W = [w_f ; w_r] ([H4][w_ld] each);
 *                    dg row r of utterance b at dg + b * b_stride + r * ld.  Fixed order throughout.  Refused: a null pointer, E outside
 *                    1 .. 1024, H4 / rows / B below 1, more than 64 KiB of LDS (2 H4 + floor(1024 / E) E floats), ld < 2 H4,
 *                    w_ld < col0 + E. */
typedef struct ss_code_src {
    const float* o;       /* forward: the BLSTM output slab */
    float* d_o;           /* backward: its gradient slab */
    int H, freq, col, ld;
} ss_code_src;
int ss_op_mse_loss(const float* out_dev, long out_ld, long out_bs, const float* tgt_dev, long tgt_ld, long tgt_bs, float* d_out_dev, long d_ld,
                   long d_bs, int B, int T, int C, float grad_scale, float* partials_dev, float* loss_dev, void* stream);
int ss_op_ce_loss(const float* logits_dev, long ld, long bs, const int* tgt_dev, float* d_out_dev, long d_ld, long d_bs, int B, int T, int C,
                  float grad_scale, float* partials_dev, float* loss_dev, void* stream);
long ss_op_colsum_scratch_doubles(int cols);
int ss_op_colsum(const float* in_dev, long ld, int R, int C, int two_dir, float* o0_dev, float* o1_dev, float* o2_dev, float* o3_dev,
                 double* part_dev, long part_doubles, unsigned* ctr_dev, int ctr_words, void* stream);
int ss_op_dec_in(const ss_code_src* src, int nsrc, const float* emb_dev, int emb_dim, int emb_col, float* dst_dev, int ld, int B, int T, int f,
                 void* stream);
int ss_op_dec_in_grad(const ss_code_src* src, int nsrc, const float* d_in_dev, int ld, int B, int T, int f, void* stream);
int ss_op_dec_in_codes_grad(const ss_code_src* src, int nsrc, const float* d_in_dev, int ld, int B, int T, int f, void* stream);
int ss_op_dec_in_codes(const ss_code_src* src, int nsrc, const float* emb_dev, int emb_dim, int emb_col, float* codes_dev, long codes_floats,
                       float* dst_dev, int ld, int B, int T, int f, void* stream);
int ss_op_spk_grad(const float* dg_dev, long ld, long b_stride, int rows, const float* w_f_dev, const float* w_r_dev, long w_ld, int col0, int H4,
                   int E, float* out_dev, int B, void* stream);
/* The fused weight gradients of the encoder BLSTMs (speechsplit_amd/csrc/lstm_wgrad.hip) as the engine launches them: a TABLE of 1 .. 8 tasks
 * in one launch, each with its own H (1 .. 32), In, R and strides, on the CALLER's memory.  Per task, with dg [R][8 H] dense, x [R][In] (row
 * stride x_ld) and hout [R][2 H] (row stride h_ld; the columns behind 2 H are never read), for both directions d:
 *     gwih[d][n][k] += sum_r dg[r][d 4H + n] x[r][k]                  gwih [2][4 H][In]
 *     gwhh[0][n][k] += sum_r dg[r + 1][n] hout[r][k]                  gwhh [2][4 H][H]    (r + 1 < R)
 *     gwhh[1][n][k] += sum_r dg[r][4H + n] hout[r + 1][H + k]         (r + 1 < R)
 *     gb[d][0][n] and gb[d][1][n] += sum_r dg[r][d 4H + n]            gb [2][2][4 H]      (b_ih and b_hh have the same gradient)
 * ROW 0 OF dg MUST BE ZERO (it is a halo row in every slab): the forward direction's bias is summed beside its W_hh, over dg[r + 1], so a
 * non-zero row 0 would be missing from gb[0].  Not checked: dg is device data.
 * The rows are cut into row_groups groups of ceil(ceil(R / row_groups) / 64) 64 rows (the last ones may be empty); a group's sum is one fp32
 * chain of fused multiply-adds in row order, the groups' sums are added in float64 in group order, rounded to fp32 once and added (fp32) to
 * what the output holds.  The same bits on every call, whatever the order the workgroups arrive in.  part_dev: scratch of at least
 * ss_op_lstm_wgrad_table_floats(t, n, row_groups) = tiles row_groups 4096 floats, 16-byte aligned; ctr_dev: at least
 * ss_op_lstm_wgrad_table_counters(t, n) = tiles words, ZERO on entry and zero again when the launch retires (tiles: the sum over the tasks of
 * ceil(8 H / 64) (ceil(In / 64) + (4 H % 64 == 0 ? 1 : 2))).  Both size functions return 0 for a table the hook would refuse.  Refused before
 * anything is enqueued: a null pointer, n outside 1 .. 8, row_groups outside 1 .. 1024, H outside 1 .. 32, In or R below 1, x_ld < In,
 * h_ld < 2 H, dg not 16-byte aligned, more than 65535 tiles, scratch or counters too small or misaligned. */
typedef struct ss_wgrad_task {
    const float* dg;
    const float* x;
    long x_ld;
    const float* hout;
    long h_ld;
    float *gwih, *gwhh, *gb;
    int H, In;
    long R;
} ss_wgrad_task;
long ss_op_lstm_wgrad_table_floats(const ss_wgrad_task* t, int n, int row_groups);
int ss_op_lstm_wgrad_table_counters(const ss_wgrad_task* t, int n);
int ss_op_lstm_wgrad_table(const ss_wgrad_task* t, int n, int row_groups, float* part_dev, long part_floats, unsigned* ctr_dev, int ctr_words,
                           void* stream);
/* The random-resampling kernels (speechsplit_amd/csrc/interp.hip; reference InterpLnr, model.py:355-436, and quantize_f0_torch,
 * utils.py:62-74), engine-free and on the CALLER's memory: each hook hands its arguments to one kernel launcher and does nothing else.
 * Every refusal is made before anything is enqueued.  A PLAN for B utterances is (i0 i32 [B][P], lam f32 [B][P], nrows i32 [B]) and, for the
 * adjoint, start i32 [B][T + 1].
 *   ss_op_interp_plan  the index path, bit-exact to the reference: per utterance b and segment s < S, candidate j < ncand has the fp32
 *                    quotient q = j / scales[b S + s] (IEEE division), fl = floor(q), lam = q - fl, and is KEPT when fl < len_seg[b S + s] - 1
 *                    and fl + off < len - 1, off being the sum of the utterance's earlier len_seg and len = len_seq_dev[b] (len_seq_dev
 *                    NULL: len_seq_const).  The kept candidates in (s, j) order are the output rows: counts[b] is their number,
 *                    nrows[b] = min(counts[b], P), i0[b][r] = fl + off and lam[b][r] for r < nrows[b], and ZERO in both for nrows[b] <= r < P.
 *                    start[b][i] = the number of rows r < nrows[b] with i0[b][r] < i, for i = 0 .. T (i0 is non-decreasing in r).  Any S,
 *                    ncand <= 64, P <= 512 and T.  The scales must be positive with j / scale inside an int, and len_seq <= T if the plan is to
 *                    index T frames: both are device data, NOT CHECKED.  Refused: a null pointer (len_seq_dev may be NULL), B / S / T below 1,
 *                    ncand outside 1 .. 64, P outside 1 .. 512, len_seq_const outside 0 .. T when it is used.
 *   ss_op_interp_gather  y(b, r, c) = (1 - lam) * x(b, i0, c) + lam * x(b, i0 + 1, c) for r < nrows[b] -- fp32, the two products and the sum
 *                    rounded separately, subnormal products kept (no flush to zero) -- and +0.0 for nrows[b] <= r < P; x and y are VIEWS
 *                    (p, ld, bs) with p at frame 0.  Rows of x other than i0 and i0 + 1 of a live row are never read.  y_img_dev (nullable):
 *                    also the image of y (what ss_op_split_image makes of y at the scale *img_scale_dev, NULL: 16), same geometry as y.
 *                    Refused: a null pointer, B / P outside 1 .. 65535, C below 1, a row stride below C, img_scale_dev without y_img_dev, and
 *                    an image when C % 8, x_ld % 4, x_bs % 4, y_ld % 8 or y_bs % 8 is not 0, x / y is not 16-byte or y_img not 32-byte aligned
 *                    (the launcher would drop the image silently).
 *   ss_op_interp_quant  the training step's outer resampling: mel [B][T][CM] and f0 [B][T] dense.  ymel(b, r, c < CM) as the gather; f as
 *                    the gather of f0; the class q = 0 when not f > 0 (unvoiced, -0.0, NaN), else min(rint(f * 255) + 1, NOH - 1), rint
 *                    to nearest even, the product in fp32; qidx[b][r] = q; yoh(b, r, c) = (c == q) for ALL yo_ld columns of the row (the
 *                    padding columns behind NOH are written zero).  Rows nrows[b] <= r < P: ymel zeros, class 0.  f * 255 must fit an int
 *                    (not checked).  Refused: a null pointer, B / P outside 1 .. 65535, T below 2, CM below 1, NOH below 2, ym_ld < CM,
 *                    yo_ld < NOH.
 *   ss_op_interp_scatter  the gather's adjoint through start: dx(b, i, c) = sum over the rows r with i0 = i, ascending, of (1 - lam_r)
 *                    dy(b, r, c), then over the rows with i0 = i - 1 of lam_r dy(b, r, c): one fp32 chain of fused multiply-adds from 0, the
 *                    weight 1 - lam_r rounded to fp32 first.  Every frame i < T of every utterance is written: +0.0 where no row contributes.
 *                    The same bits on every call.  Refused: a null pointer, B / P outside 1 .. 65535, T or C below 1, a row stride below C. */
int ss_op_interp_plan(const float* scales_dev, const int* len_seg_dev, const int* len_seq_dev, int len_seq_const, int S, int ncand, int P, int T,
                      int B, int* i0_dev, float* lam_dev, int* nrows_dev, int* counts_dev, int* start_dev, void* stream);
int ss_op_interp_gather(const int* i0_dev, const float* lam_dev, const int* nrows_dev, int P, const float* x_dev, long x_ld, long x_bs, float* y_dev,
                        long y_ld, long y_bs, int C, int B, float* y_img_dev, const float* img_scale_dev, void* stream);
int ss_op_interp_quant(const int* i0_dev, const float* lam_dev, const int* nrows_dev, int P, int T, const float* mel_dev, const float* f0_dev, int CM,
                       float* ymel_dev, long ym_ld, long ym_bs, float* yoh_dev, long yo_ld, long yo_bs, int NOH, int* qidx_dev, int B, void* stream);
int ss_op_interp_scatter(const float* lam_dev, const int* start_dev, int P, int T, const float* dy_dev, long dy_ld, long dy_bs, float* dx_dev,
                         long dx_ld, long dx_bs, int C, int B, void* stream);
/* The re-layout and guard kernels of a training step (speechsplit_amd/csrc/elementwise.hip, input_grads.hip), engine-free and on the CALLER's
 * memory like the hooks above: each hands its operands to one kernel launcher and does nothing else.  Every move is exact: no hook here
 * rounds anything but the images.  An IMAGE beside an fp32 tensor of n elements is, with img_bf16 == 0, what ss_op_split_image makes of that
 * tensor at scale 16 (n % 8 == 0, base 32-byte aligned) and, with img_bf16 != 0, the tensor rounded to bf16 (to nearest even; 2 bytes per
 * element, base 8-byte aligned).  Every refusal is made before anything is enqueued.
 *   ss_op_conv_pack  conv weight w [Co][Ci][5] -> the forward pack wf [Co][5][Cp], wf[co][k][c] = w[co][c][k] for c < Ci and ZERO for
 *                    Ci <= c < Cp, and (wb_dev not NULL) the input-gradient pack wb [Ci][5][Co], wb[ci][k][co] = w[co][ci][4 - k] (taps
 *                    flipped); wf_img / wb_img (nullable): their images.  Refused: a null w / wf, a dimension below 1, Co % 4 != 0,
 *                    Cp % 4 != 0, Cp below Ci, wb_img without wb, wf / wb not 16-byte aligned, an image that breaks the rule above.
 *   ss_op_conv_pack_many  1 .. 8 such tasks in one launch, the same bits as one ss_op_conv_pack each.
 *   ss_op_conv_pack_dx  wb [Ci][5][Co] alone, for any Ci and Co.
 *   ss_op_conv_unpack  packed weight gradient gp [Co][5][Cp] -> g [Co][Ci][5], g[co][ci][k] = gp[co][k][ci] (acc == 0) or g += (acc != 0);
 *                    the columns Ci <= c < Cp of gp are never read.  ss_op_conv_unpack_many: 1 .. 8 tasks in one launch.  Refused: a null
 *                    pointer, a dimension below 1, Cp below Ci.
 *   ss_op_prep       1 .. 48 tasks dst[i] = a[i] + b[i] (b NULL: dst is a COPY OF THE BITS of a, -0.0 and NaN payloads included), i < n, and
 *                    (img not NULL) the image of dst.  A task moves as float4 when n % 4 == 0 and a, b, dst are 16-byte aligned, else
 *                    element by element, with the same result.  Refused: a null a / dst, n below 1, a task with an image that could not
 *                    take the float4 path (the kernel would drop the image), an image that breaks the rule above.
 *   ss_op_transpose  out [C][R] = in [R][C]^T, both dense.  Refused: a null pointer, R or C below 1, R above 65535 * 32.
 *   ss_op_copy_rows  dst(b, t, c) = src(b, t, c) for c < C, both VIEWS (p, ld, bs) as above.  len_dev (nullable; i32 [B]): rows at or beyond
 *                    L_b = min(max(len[b], 0), T) of src are never read and dst gets +0.0 there.  Nothing else of dst is written (halo
 *                    rows and row gaps keep their bits).  Refused: a null src / dst, B outside 1 .. 65535, T or C below 1, a row stride
 *                    below C.
 *   ss_op_act_scales  out[i] for 1 .. 8 blocks: with bound = fmaf(sqrtf(16 T), max|gamma_i|, max|beta_i|) over the block's C_i channels
 *                    (fp32, one fused multiply-add), out[i] = min(16, the largest power of two s >= 2^-20 with
 *                    bound * s <= 32768).  A bound of +inf KEEPS 16: no scale makes that block's products finite, ss_op_param_guard's kernel
 *                    reports the parameter and the step that computed the scale is skipped.  A NaN element does not enter the maxima (the
 *                    guard reports it as well).  C_i == 0: bound 0, 16.  Refused: a null array, n outside 1 .. 8, T below 1, C_i < 0, a null
 *                    gamma_i / beta_i with C_i > 0.
 *   ss_op_param_guard  *sticky_dev |= SS_STATUS_RANGE if any of p[0 .. n) is NaN, infinite or has |p| >= limit; no other bit of the word
 *                    changes and a clean arena leaves it as it was.  Refused: a null pointer, n not a positive multiple of 4, p_dev not
 *                    16-byte aligned. */
typedef struct ss_conv_pack_task {
    const float* w;
    float *wf, *wb, *wf_img, *wb_img;
    int Co, Ci, Cp;
} ss_conv_pack_task;
typedef struct ss_conv_unpack_task {
    const float* gp;
    float* g;
    int Co, Ci, Cp;
} ss_conv_unpack_task;
typedef struct ss_prep_task {
    const float* a;
    const float* b;
    float* dst;
    long n;
    float* img;
} ss_prep_task;
int ss_op_conv_pack(const float* w_dev, int Co, int Ci, int Cp, float* wf_dev, float* wb_dev, float* wf_img_dev, float* wb_img_dev, int img_bf16,
                    void* stream);
int ss_op_conv_pack_many(const ss_conv_pack_task* t, int n, int img_bf16, void* stream);
int ss_op_conv_pack_dx(const float* w_dev, int Co, int Ci, float* wb_dev, void* stream);
int ss_op_conv_unpack(const float* gp_dev, int Co, int Ci, int Cp, float* g_dev, int acc, void* stream);
int ss_op_conv_unpack_many(const ss_conv_unpack_task* t, int n, int acc, void* stream);
int ss_op_prep(const ss_prep_task* t, int n, int img_bf16, void* stream);
int ss_op_transpose(const float* in_dev, int R, int C, float* out_dev, void* stream);
int ss_op_copy_rows(const float* src_dev, long s_ld, long s_bs, float* dst_dev, long d_ld, long d_bs, const int* len_dev, int B, int T, int C,
                    void* stream);
int ss_op_act_scales(const float* const* gamma_dev, const float* const* beta_dev, const int* C, int n, int T, float* out_dev, void* stream);
int ss_op_param_guard(const float* p_dev, long n, float limit, unsigned* sticky_dev, void* stream);
/* Test hook: the optimiser kernels behind ss_set_weight_decay / ss_set_ema on the caller's own buffers, at any length.  state is 256 bytes of
 * device scratch that takes the place of the workspace's head; the hook fills it from the scalars below (as ss_set_adam, ss_set_weight_decay and
 * ss_set_ema would), runs the step's prepare kernel (skip_status: nullable device float, non-zero = the step is skipped) and then
 *   mode 0: the extended Adam update over the elements [lo, hi) of p, g, m, v and (ema non-null) ema, all given by their BASE; clip_coef > 0
 *           takes the clipped form with that coefficient; n_runs > 0 the decayed-run table (ss_set_weight_decay's which = 1), 0 decays every element;
 *   mode 1: ema[i] += w * (p[i] - ema[i]) over [lo, hi) alone; with step < 0 under the state an earlier call left in `state` (nothing is
 *           copied or waited for and no prepare runs: the one launch, for timing it);
 *   mode 2: the exchange p[i] <-> ema[i] over [lo, hi) (no state is written, no prepare runs).
 * lo, hi: multiples of 4; arenas 16-byte aligned; the runs must follow each other without a hole or an overlap and cover [lo, hi).  Refused: null required pointers, a mode outside 0 .. 2, mode 0 with neither term on. */
typedef struct ss_optim_ext_op {
    float *p, *m, *v, *ema;
    const float* g;
    void* state;
    const float* skip_status;
    long lo, hi;
    double lr, beta1, beta2, eps;
    long step;
    float grad_scale, clip_coef, weight_decay;
    double ema_decay;
    int ema_warmup;
    long ema_updates;
    int n_runs;
    const long* run_start;
    const int* run_len;
    const int* run_decayed;
    int mode;
} ss_optim_ext_op;
int ss_op_optim_ext(const ss_optim_ext_op* op, void* stream);
/* Test hook, host side only: the runs of [0, arena) by "decayed under ss_set_weight_decay(which = 1)" that an engine of this kind and these
 * hyper-parameters builds from its parameter table -- up to cap of them into start / len / decayed; returns their number (negative: refused).
 * The runs cover the arena without a hole: a tensor's run takes the alignment gap behind it, the status slot is the last run, not decayed. */
int ss_op_wd_runs(int kind, const ss_hparams* hp, long* start, int* len, int* decayed, int cap);
/* Test hook, engine-free: lr_dev[i] = lr_t of ss_set_lr_schedule's definition at t = steps_dev[i] (n device longs -> n device doubles), by the
 * __device__ function the optimiser's prepare kernels call, one thread per value.  Refused: what ss_set_lr_schedule refuses, null pointers,
 * n outside 1 .. 2^24. */
int ss_op_lr_schedule(int kind, double base, int warmup_steps, double warmup_start, int total_steps, double gamma, int period, double min_lr,
                      const long* steps_dev, long n, double* lr_dev, void* stream);
/* The GEMM over operand images (speechsplit_amd/csrc/gemm_img.hip), the engine's default for every large contraction: an IMAGE has the
 * geometry of its fp32 matrix (4 bytes per element) with every aligned group of 8 elements along the contiguous axis replaced by 16 bytes of
 * hi pieces and 16 bytes of lo pieces of the fp16 x 2 split of scale * x (scale a power of two).
 *   ss_op_split_image: fp32 [rows][cols] (row stride ld) -> image (row stride ldi; cols % 8 == 0).
 *   ss_op_gemm_img:    C[M,N] (+)= sum_k A(m,k) B(n,k) (+ bias) over two images split with scale_a / scale_b.  flags: 1 = A stored [K,M],
 *                      2 = B stored [K,N], 4 = accumulate into C, 8 = single-piece form: both operands are plain bf16 matrices (2 bytes
 *                      per element, ld in elements, no scales; K % 64 == 0 for a K-contiguous operand) -- the 16-bit data path of
 *                      SS_PRECISION_BF16, where a slab stored in bf16 is its own image.  a_seglen / a_segstride: segmented K axis of a K-contiguous A (k = seg *
 *                      seglen + w lives at column seg * segstride + w: a k=5 convolution over a haloed slab), 0 = none.  ksplit > 1 needs
 *                      part_dev (ksplit * M * N floats of scratch; partial slabs, added in a fixed order).  zeros_dev: >= 1 KB of zero bytes
 *                      (needed when both operands are reduction-major and K % 32 != 0).  cfg: -1 = choose the tile, 0 = 256 x 256,
 *                      1 = 128 x 128, 2 = 256 x 128. */
int ss_op_split_image(const float* src_dev, long ld, long rows, int cols, float scale, float* img_dev, long ldi, void* stream);
/* ss_op_gemm in its fp16 x 2 mode (flags: 1 = A stored [K,M], 2 = B stored [K,N]) as the engine's weight-gradient launches call it: each operand
 * optionally comes with its image (split with the scale 16; null = none), which the kernel takes where the form it picks can load that operand
 * in whole groups -- the pipelined k-loop of ss_tune("gemm_pipe") brings an image of B in by LDS-DMA -- and with part_dev (ksplit * M * N
 * floats, nullable) a split-K launch writes partial slabs that are added into C in a fixed order instead of meeting there through atomics. */
int ss_op_gemm_pre(const float* a_dev, long lda, const float* a_img_dev, const float* b_dev, long ldb, const float* b_img_dev, float* c_dev, long ldc,
                   float* part_dev, int M, int N, int K, int flags, int ksplit, void* stream);
int ss_op_gemm_img(const float* a_img_dev, long lda, const float* b_img_dev, long ldb, float* c_dev, long ldc, const float* bias_dev, int M, int N,
                   int K, int flags, int ksplit, int cfg, float scale_a, float scale_b, int a_seglen, long a_segstride, float* part_dev,
                   const void* zeros_dev, void* stream);
/* Descriptor-level TEST HOOKS of the two GEMM launchers: one plain struct carries every field a product launch sets, and the hook hands it to
 * the launcher unchanged (launch_gemm / launch_gemm_img in speechsplit_amd/csrc/common.h, where each field is specified) and does nothing else.
 * An operand's element (row, col) of batch b lives at p + b * bstride + row * ld + (col / seglen) * segstride + col % seglen (seglen == 0:
 * + col), all in elements; the result at c + b * cstride + m * ldc + n.  flags: 1 = A stored [K,M], 2 = B stored [K,N], 4 = accumulate into C;
 * ss_op_gemm_desc also 8 = bf16-rounded operands, 16 = fp16 x 2 split.  row_period > 0: row m is stored only if (m + row_off) % row_period
 * lies in [row_lo, row_hi).  Every optional pointer may be NULL.
 *   ss_op_gemm_desc      want: least number of workgroups the tile choice should produce (0: the library default).  amax_a / amax_b: device
 *                        words holding max|operand| (fp16 x 2: the scale is the power of two that brings it into [128, 256)); a_pre / b_pre:
 *                        the operand's image (same geometry); a_pre_scale / b_pre_scale: device words holding a fixed scale (NULL: 16);
 *                        part: batch * ksplit * M * N floats for the ordered split-K (NULL: atomics).
 *   ss_op_gemm_img_desc  a / b are IMAGES (bf16 != 0: plain bf16 tensors, 2 bytes per element).  rm_T > 0 (A K-contiguous, rm_T >= 32):
 *                        logical row m of A and C is memory row (m / rm_T) * rm_TP + m % rm_T.  scale_a / scale_b: device words (NULL: 16);
 *                        zeros: >= 1 KB of zero bytes; cfg: -1 .. 3 as ss_op_gemm_img.  The work-queue form stays with ss_op_gemm_img.
 * Refused before anything is enqueued, each with its own ss_last_error text: a null descriptor or a null a / b / c, a negative size, an
 * unknown flag, a row mask outside its period, ksplit > 1 without the accumulate flag (ss_op_gemm_desc) or without part (ss_op_gemm_img_desc),
 * and whatever the image GEMM does not support (its alignment rules, rm_T with a row mask, a row mask with ksplit > 1). */
typedef struct ss_gemm_desc {
    const float *a, *b;
    float* c;
    const float *bias, *amax_a, *amax_b, *a_pre, *b_pre, *a_pre_scale, *b_pre_scale;
    float* part;
    long lda, a_bstride, a_segstride, ldb, b_bstride, b_segstride, ldc, cstride;
    int a_seglen, b_seglen, M, N, K, batch, flags, want, row_period, row_off, row_lo, row_hi, ksplit;
} ss_gemm_desc;
typedef struct ss_gemm_img_desc {
    const void *a, *b;
    float* c;
    const float *bias, *scale_a, *scale_b;
    float* part;
    const void* zeros;
    long lda, a_bstride, a_segstride, ldb, b_bstride, b_segstride, ldc, cstride;
    int a_seglen, b_seglen, M, N, K, batch, flags, row_period, row_off, row_lo, row_hi, rm_T, rm_TP, ksplit, cfg, bf16;
} ss_gemm_img_desc;
int ss_op_gemm_desc(const ss_gemm_desc* desc, void* stream);
int ss_op_gemm_img_desc(const ss_gemm_img_desc* desc, void* stream);
/* One relu(GroupNorm(ConvNorm(x))) block (model.py:61-67,76-77; 16 channels per group) through the engine's own block
 * routines, forward and -- when dy is given -- backward.  x [B,T,Ci], w [Co,Ci,5], bias/gamma/beta [Co], y/dy [B,T,Co],
 * dx [B,T,Ci] (nullable), gw [Co,Ci,5], gb/ggamma/gbeta [Co]; scratch of ss_op_conv_block_scratch() floats.  T <= 256 with a
 * backward; forward only (dy NULL) up to SS_MAX_EVAL_FRAMES, where the GroupNorm runs the chunked long-sequence kernels. */
long ss_op_conv_block_scratch(int B, int T, int Ci, int Co);
int ss_op_conv_block(const float* x_dev, const float* w_dev, const float* bias_dev, const float* gamma_dev, const float* beta_dev,
                     const float* dy_dev, float* y_dev, float* dx_dev, float* gw_dev, float* gb_dev, float* ggamma_dev,
                     float* gbeta_dev, float* scratch_dev, long scratch_floats, int B, int T, int Ci, int Co, void* stream);
/* The forward of ss_op_conv_block over a ragged batch (len_dev i32[B]; NULL: the plain forward): x rows t >= len[b] are never read, the
 * GroupNorm statistics of row b run over its len[b] frames, y rows t >= len[b] are zeros.  T up to SS_MAX_EVAL_FRAMES; same scratch. */
int ss_op_conv_block_ragged(const float* x_dev, const float* w_dev, const float* bias_dev, const float* gamma_dev, const float* beta_dev,
                            const int* len_dev, float* y_dev, float* scratch_dev, long scratch_floats, int B, int T, int Ci, int Co,
                            void* stream);
/* The ReLU branch the engine took in conv block `block` ("enc1.c1_0" .. "enc1.c2_2", "enc3.c_0" .. "enc3.c_2", "enc2.c") of
 * the last forward: mask [B,T,Co] dense, 1.0f where the GroupNorm output is > 0.  A GroupNorm output within fp32 rounding
 * of 0 may fall on either side in two correct implementations; parity tests hand this mask to the oracle so that the
 * comparison of gradients does not depend on that coin flip. */
int ss_debug_relu_mask(ss_engine* e, const char* block, float* mask_dev, void* stream);
/* tuning knobs (process-global; every value leaves the results correct): "lstm_nw" 4|8|16, "lstm_g" 0..16,
 * "gemm_want" >= 1, "overlap" 0|1, "persist" 0|1, "gemm_mode" 0 (fp32 MFMA) | 1 (split arithmetic on
 * the 16-bit pipe), "fwd_f16x2" / "bwd_f16x2" 0|1 (fp16 x 2 instead of bf16 x 3 for the forward / the scaled gradient
 * contractions), "seq_spin_log2" 0..24 (log2 of the persistent kernels' bounded wait; 0 makes it expire at once -- how the
 * tests exercise the abort path), "deterministic" 0|1, "seq_tag" 0|1 (forward persistent recurrence: step tag in the hand-off
 * payload where every group sits on one XCD | always the flag line), "seq_var" 0|2|4 (backward persistent recurrence: form of its warm-up
 * reads: whole 1 KB runs | one dword per 128-byte line (default) | one per 64 bytes; results bit-identical), "gemm_ws" 0|1|2 (wave-specialised form of
 * the 128 x 128 fp16 x 2 GEMM: never | where it measured faster in isolation | always), "dp_model" 0|2..64 and "dp_buckets" 0|1 (data-parallel schedule, see ss_g3_dp_train_step),
 * "compact0" 0|1 (decoder layer 0 on one row per block of repeated input frames), "op_time_major" 0|1 (ss_op_lstm_fwd / _bwd
 * read their slabs as [T+4,B,C]; persistent kernels only -- a layout experiment); schedule of the end of the backward (round 4,
 * tools/real_timeline.py): "dec_tail_split" 0..10 (which stream takes the decoder's layer-0 / layer-1 and the head's weight gradients; default 9),
 * "conv_dw_off" 0|1 (Generator_6: conv weight gradients off the trunk's dependent chain), "early_dw" 0|1 (16-bit mode: a decoder
 * layer's weight gradients beside the next backward recurrence, off); "gemm_pipe" 0|1 (fp16 x 2 GEMM: the pipelined k-loop for launches
 * whose B operand is an image and both operands are reduction-major -- the weight gradients; default 1, same results bit for bit).  The timing experiments that produce WRONG results ("lstm_mode",
 * "gemm_diag", "seq_prio" > 1) are compiled out of this library; `make -C speechsplit_amd/csrc diag` builds
 * libspeechsplit_hip_diag.so with them for tools/ (never loaded by the package unless SS_DIAG_LIB=1 is set). */
int ss_tune(const char* key, int value);
/* Arithmetic of the contractions (convolutions, LSTM input projections, all weight / input gradients, head).
 * SS_PRECISION_F32 (default) -- the 1e-4 parity mode.  Operands, accumulation and storage are fp32; every PRODUCT is formed
 *   on the 16-bit matrix pipe from a split of both fp32 operands:
 *     fp16 x 2 (default wherever an operand's magnitude is known): y = s*x = h + l, h = fp16(y), l = fp16(y - h), s a power of
 *       two; 3 v_mfma_f32_32x32x16_f16 per k-step (h.l, l.h, h.h): 22 significand bits relative to the operand's scaled
 *       maximum (elements more than 2^22 below it lose relative precision; the residual goes subnormal 2^-3 below the
 *       maximum's binade and flushes at 2^-33 of it).  Scales: WEIGHTS, hidden states (|h| < 1) and the network inputs use the fixed
 *       s = 16 (|x| < 4094 survives); the conv blocks' outputs use min(16, the power of two that keeps sqrt(16 T) max|gamma| +
 *       max|beta| inside fp16) computed on the device from their GroupNorm affine every step (a gamma of 100 or 1000 trains in this
 *       mode, at the same 1e-4 parity); gradient operands the power of two for the maximum their producer kernel measured.  What is
 *       refused -- status SS_STATUS_RANGE, the Adam update skipped on the device -- is a parameter that is not finite or reaches
 *       |p| >= 2048, checked inside every forward (there is no silent overflow and no automatic change of split).
 *     bf16 x 3 (head, encoder BLSTMs, unaligned shapes; everything with ss_tune("fwd_f16x2" / "bwd_f16x2", 0)): exact
 *       3-way truncation split x = h + m + l, 6 v_mfma_f32_32x32x16_bf16 per k-step, dropped terms <= 2^-24 relative.
 *     ss_tune("gemm_mode", 0): true fp32 MFMA (v_mfma_f32_32x32x2_f32), the A/B reference.  (In SS_PRECISION_BF16 the contractions carry the
 *       bf16 flag and this kernel rounds their operands to bf16 like every other: the products are then fp32-wide over bf16-rounded
 *       operands, not the unrounded fp32 reference -- take that in SS_PRECISION_F32.)
 *   Against fp64 the three measure 1.3-2.2e-6, 1.2e-6 and 1.3e-6 of max|C| (profiles/r02/f16x2_error.txt).
 *   ss_tune("gemm_mode", 0) together with ss_tune("persist", 0) (the decoder recurrences as one fp32-MFMA launch per time step) is the mode in
 *   which EVERY product of the step is fp32-wide -- the reference's arithmetic; bench.py times it as alt_precisions.all_fp32_mfma.
 * SS_PRECISION_BF16 (BASELINE configs 3-5) -- the 16-bit data path (round 4).  Whoever produces an operand of a large contraction also stores
 *   it as a plain bf16 tensor of the same geometry (round to nearest even), and the contraction runs from there on the single-piece form of
 *   the image GEMM (csrc/gemm_img.hip: one v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation, no scales): packed conv weights and
 *   stacked W_ih (per-step re-layouts), decoder hidden states (the forward recurrence's storing wave), resampled trunk activations (the
 *   fused GroupNorm + gather), pre-activation gradients (the backward recurrence's storing wave), conv-output gradients (the GroupNorm
 *   backward).  The persistent recurrences multiply the HIGH fp16 pieces of h and W_hh only (one v_mfma_f32_16x16x32_f16 per product, half the
 *   hand-off payload, 11 significand bits per operand).  fp32 throughout: master weights, gradients' accumulation and the gradient arena,
 *   cell state, gate pre-activations, GroupNorm statistics, losses, the resampling index path (bit-exact as in the fp32 mode), Adam.
 *   Contractions without images (layer-0 convolutions over the 80 / 264-channel inputs, the decoder's 164-column layer-0 input, the head's
 *   weights, the encoder BLSTM projections) round their fp32 operands to bf16 inside round 2's GEMM kernel; the encoder BLSTMs' weight
 *   gradients are exact fp32 sums in both modes (csrc/lstm_wgrad.hip).  ss_tune("bf16_img", 0) selects round 3's form of the
 *   mode (fp32 slabs only, operands rounded inside the GEMM, fp16 x 2 recurrences) for A/B runs.
 * When it may be called.  On any engine, bound or not, stepped or not, BETWEEN steps or accumulation cycles.  The two modes lay the image
 *   buffers out differently, so the next call that runs a forward (train step, ss_*_forward*, ss_g3_rhythm*) plans the workspace again and
 *   re-zeroes it, as after a change of (B, T): its result does not depend on what the engine ran in the other mode
 *   (tests/test_gpu_same_shape_history.py).  That costs one memset per switch (0.1 - 0.2 ms) and nothing per step; the same holds for
 *   ss_tune("bf16_img").  A change of the precision DISCARDS the forward in flight: a forward of one precision cannot be differentiated
 *   in the other, so ss_*_backward*, ss_train_finish after it fail ("without a preceding ...") until a new forward has run.  Setting
 *   the precision the engine already has changes nothing. */
#define SS_PRECISION_F32 0
#define SS_PRECISION_BF16 1
int ss_set_precision(ss_engine* e, int precision);
/* Live timing of the step's kernels inside a caller's own timed region.  ss_profile(e, mask) makes the engine bracket every
 * launch of the classes whose bit (1u << class) is set with hipEvents on the stream the launch goes to (a non-zero mask clears
 * the record, 0 stops recording; at most 8192 launches are kept).  A bracket costs 4-8 us of stream time (the launch behind it cannot
 * start before the one in front has retired and signalled): all 71 per step are +4.5 % on the step, the dominant class + the recurrences
 * (18 per step) +2.9 % (round 3; the step has become shorter, the brackets have not).  ss_profile_sample(e, n) therefore brackets only
 * every n-th training step (n = 1: every step; the count starts again with every ss_profile call).  ss_profile_read synchronises on the recorded events of one class and returns their count, their summed duration
 * and their summed algorithmic FLOPs (2*M*N*K per GEMM; 2 * 2 directions * B * T * 4H * H per recurrence launch). */
#define SS_PROF_DEC_PROJ 0  /* decoder input projection, layers >= 1 (NT, M = B*T, N = 8H, K = 2H) */
#define SS_PROF_DEC_PROJ0 1 /* decoder input projection, layer 0 (K = 164 / 66) */
#define SS_PROF_DEC_DW 2    /* decoder weight gradients dW_ih, dW_hh (TN, split-K) */
#define SS_PROF_DEC_DX 3    /* decoder input gradients (NN) */
#define SS_PROF_CONV_FWD 4  /* conv trunk forward (segmented-K NT) */
#define SS_PROF_CONV_DW 5   /* conv weight gradients (TN) */
#define SS_PROF_CONV_DX 6   /* conv input gradients */
#define SS_PROF_REC_FWD 7   /* persistent decoder recurrence, forward (one launch per layer) */
#define SS_PROF_REC_BWD 8   /* persistent decoder recurrence, backward */
#define SS_PROF_ENC_LSTM 9  /* encoder BLSTM projections / gradients (small GEMMs) */
#define SS_PROF_HEAD 10     /* LinearNorm head forward / gradients */
#define SS_PROF_CLASSES 11
/* timeline-only classes (no flops; ss_profile_timeline / tools/real_timeline.py): the non-GEMM launches on the step's dependent chains */
#define SS_PROF_ENC_REC 11  /* encoder BLSTM recurrences (one launch per layer and pass) */
#define SS_PROF_GN 12       /* GroupNorm + ReLU forward / gather / backward */
#define SS_PROF_WGRAD 13    /* fused encoder-BLSTM weight gradients */
#define SS_PROF_ADAM 14     /* optimiser launches */
#define SS_PROF_PREP 15     /* per-step weight re-layouts */
int ss_profile(ss_engine* e, unsigned class_mask);
int ss_profile_sample(ss_engine* e, int every_nth_step);
int ss_profile_read(ss_engine* e, int klass, int* launches, double* total_us, double* total_flops);
/* The same brackets as a timeline: out[3 * i .. 3 * i + 2] = (class + 100 x stream [0 main, 1 side, 2 / 3 branch streams], start, end) of record i in enqueue order, microseconds relative to the
 * first record's start; returns the number of records written (<= cap), negative on error.  (tools/real_timeline.py) */
int ss_profile_timeline(ss_engine* e, double* out, int cap);
/* timing experiment: with ss_tune("gemm_diag", 16) the 128x128 NT bf16x3 GEMM accumulates, for its first 64 workgroups, the
 * s_memtime ticks every wave spends per k-loop phase; out24 = [4 waves][split+store, barrier, load issue, fragments+MFMA,
 * barrier, k-tiles (wave 0 only)].  Synchronises the device. */
int ss_debug_gemm_phases(unsigned long long* out24, int reset);
/* Placement probe: n_wg workgroups (threads, lds_bytes each) write their (XCC_ID, HW_ID) hardware registers to out_dev[2 * n_wg] in launch
 * order and stay resident for hold_us microseconds.  (How workgroup indices map to XCDs is what the persistent recurrences' group slots
 * and the image GEMM's XCD filter rely on: tools/xcd_overlap_probe.py.) */
/* Placement log of ss_op_gemm_img's last work-queue launch made with ss_tune("img_xcc", mask | 0x100): words [0] tiles handed out,
 * [1] started flag, then per workgroup of the launch (from word 4) XCD (| 0x100: left without work), tiles taken, first and last tick (100 MHz). */
int ss_debug_img_wq(unsigned* out_host, int words);
int ss_debug_xcc_map(int n_wg, int threads, int lds_bytes, int hold_us, unsigned* out_dev, void* stream);
/* named internal slab of the last call ("enc1.xf2", "dec.out2", ...); layout [B, T+4, C], frame t at row t+2 */
int ss_debug_buffer(ss_engine* e, const char* name, float** ptr_dev, long* rows, long* cols);
int ss_debug_names(ss_engine* e, char* buf, int cap);
/* The kernel instance the last launch of one kind picked, as text: what = "gemm" (launch_gemm's kernels: "<tile> <NT|NN|TN|TA> <bf16x3|f16x2|bf16|f32>"
 * followed by " tr" (transposing LDS reads), " ws" (wave-specialised), " pipe" (pipelined k-loop), " apre" (A an image in that loop) or
 * " scalar" (fp32-MFMA kernel without vector loads), e.g. "128x128 TN f16x2 tr pipe apre"), "lstm_step_fwd" / "lstm_step_bwd" (the
 * per-step recurrence kernels: "<H> <NW> <G>", e.g. "512 8 4").  A host-side record written when the launcher chooses (process-global, like
 * the ss_tune knobs that steer the choice; empty before the first launch): no device work and no effect on any launch -- it lets a test that
 * sets a knob prove which instance ran.  "<kind>_seen": every DISTINCT text of that kind since the last reset, one per line in order of first
 * appearance (at most 64) -- what a whole training step launched, not only its last launch.  "reset": forgets all of it (returns 0), so that a
 * text read afterwards was written by a launch made afterwards.  Copies at most n - 1 characters into buf; returns the text's length,
 * negative for an unknown kind. */
int ss_debug_last_variant(const char* what, char* buf, int n);

#ifdef __cplusplus
}
#endif
#endif
