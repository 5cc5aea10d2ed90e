// Internal launcher prototypes for the SpeechSplit gfx950 kernels.
//
// Activation layout used by every kernel on the path ("haloed time-major"): [B, TP = T + 4, C] fp32, channels
// contiguous, real frame t at row t + 2, two all-zero rows on either side of every utterance.  The halo rows give
// the k=5 "same" convolution its zero padding, give the LSTM recurrences h(-1) = c(-1) = 0 without a branch, and
// let every weight-gradient contraction run as ONE GEMM over the flat row index b*TP + row.
#pragma once
#include <string>

#include "common.h"

namespace ss {

constexpr int HALO = 2;

// B utterances of rows: row t of utterance b starts at p + b * bs + t * ld (floats).  For EVERY launcher that takes one, p is frame 0, the
// first real row; the launchers whose kernels add the halo themselves (the GroupNorm family) step back to slab row 0 inside.
struct CRows {
    const float* p = nullptr;
    long ld = 0, bs = 0;
    static CRows slab(const float* row0, long ld, long T) { return {row0 + HALO * ld, ld, (T + 2 * HALO) * ld}; }      // a haloed slab, from its row 0
    static CRows dense(const float* p, long C, long T) { return {p, C, T * C}; }                                        // a caller's [B][T][C]
    CRows col(long c) const { return {p + c, ld, bs}; }            // the same rows from column c on
    const float* row0() const { return p - HALO * ld; }
};
struct Rows {             // the same, writable
    float* p = nullptr;
    long ld = 0, bs = 0;
    static Rows slab(float* row0, long ld, long T) { return {row0 + HALO * ld, ld, (T + 2 * HALO) * ld}; }
    static Rows dense(float* p, long C, long T) { return {p, C, T * C}; }
    Rows col(long c) const { return {p + c, ld, bs}; }
    float* row0() const { return p - HALO * ld; }
    operator CRows() const { return {p, ld, bs}; }
};

// ---------------------------------------------------------------- interp.hip
struct InterpPlan {
    int S;          // segments per utterance (max_len_seq / min_len_seg + 1 = 7)
    int ncand;      // candidate positions per segment (2 * max_len_seg = 64)
    int P;          // output rows (max_len_pad)
    int T;          // input rows
    int* i0;        // [B, P]
    float* lam;     // [B, P]
    int* nrows;     // [B]   rows kept = min(count, P)
    int* counts;    // [B]   un-truncated count (model.py:418)
    int* start;     // [B, T + 1] inverse map for the backward
};
hipError_t interp_plan(const InterpPlan& p, const float* scales, const int* len_seg, const int* len_seq,
                       int len_seq_const, int B, hipStream_t s);
// y_img (nullable): also write the pre-split image of y (GemmDesc::a_pre), same geometry as y
// img_scale (nullable: 16): device word with the power-of-two scale the image is split with (act_scales)
hipError_t interp_gather(const InterpPlan& p, CRows x, Rows y, int C, int B, hipStream_t s, float* y_img = nullptr, const float* img_scale = nullptr);
hipError_t interp_quant(const InterpPlan& p, const float* mel, const float* f0, int CM, Rows ymel, Rows yoh, int NOH, int* qidx, int B, hipStream_t s);
hipError_t interp_scatter(const InterpPlan& p, CRows dy, Rows dx, int C, int B, hipStream_t s);

// ---------------------------------------------------------------- elementwise.hip
// GroupNorm(16 channels per group, eps 1e-5, biased variance over 16 x T) + ReLU on rows [HALO, HALO+T) of haloed slabs.
hipError_t gn_relu_fwd(CRows x, Rows y, const float* gamma, const float* beta, float* stats /*[B, C/16, 2] mean, rstd*/, int B, int T, int C,
                       hipStream_t s, double* scratch = nullptr, const int* len = nullptr);
// len (nullable; device i32[B], eval-mode forwards only): a RAGGED batch.  Row b holds len[b] frames (every kernel that takes it uses
// min(max(len[b], 0), T)); the frames behind them are padding that is never read: the statistics run over t < len[b] with
// inv_n = 1 / (16 len[b]) and the outputs for t >= len[b] are zeros.  nullptr launches the kernels as compiled without the predicate.
// T <= 256: one register-resident kernel, scratch unused.  T > 256 (eval-mode inference only; no backward exists for it): three
// chunked launches that need gn_relu_fwd_scratch_bytes(B, T, C) bytes of scratch (8-byte aligned) for their float64 chunk partials.
long gn_relu_fwd_scratch_bytes(int B, int T, int C);
// the same followed by the training forward's random resampling of the block output (interp_gather), in one pass: y is the resampled
// slab from the block's first column on (p.P output rows); bit-identical to the two kernels
struct GnGather {
    float* y_img = nullptr;             // the image of y, at y's position
    const float* img_scale = nullptr;   // as interp_gather's
    bool img_bf16 = false;              // y_img is the plain bf16 tensor (element offsets, 2 bytes each) instead of a format-v2 image (common.h ss_store_img4)
};
hipError_t gn_relu_gather(CRows x, Rows y, const float* gamma, const float* beta, float* stats, const InterpPlan& p, int B, int T, int C,
                          hipStream_t s, const GnGather& o = {});
// dy (grad of the ReLU output) is replaced in place by the grad of the GroupNorm input (= conv output).
// g_gamma / g_beta / g_bias [C]: every utterance's d_gamma, d_beta, d_convbias are ACCUMULATED here (f32 atomics).
struct GnBwd {
    float* amax = nullptr;              // receives max |conv-output gradient| written, as for lstm_seq_bwd
    float* part = nullptr;              // [B][3][C] scratch; in deterministic mode the per-utterance sums go there and are added in utterance order
    // scatter / src: take the adjoint of the training forward's gather on the fly from src (the gradient of the resampled output, from the
    // block's first column on) instead of reading dy (interp_scatter fused in; dy is then only written)
    const InterpPlan* scatter = nullptr;
    CRows src;
    float* dy_img = nullptr;            // dy also as a plain bf16 tensor, at slab row 0 (same geometry; halo rows are the caller's: zero)
};
hipError_t gn_relu_bwd(CRows x, Rows dy, const float* gamma, const float* beta, const float* stats, float* g_gamma, float* g_beta, float* g_bias,
                       int B, int T, int C, hipStream_t s, const GnBwd& o = {});
// test hook: mask [B, T, C] dense = 1.0f where the block's GroupNorm output is > 0 (the ReLU branch the kernels above take)
hipError_t gn_relu_mask(CRows x, const float* gamma, const float* beta, const float* stats, float* mask, int B, int T, int C, hipStream_t s);
// out[c] += sum_r in[r*ld + c], float64 accumulation in a fixed order (elementwise.hip).  part / ctr (nullable): scratch of
// colsum_scratch_doubles(columns) float64 words and cdiv(columns, 64) zeroed counters (left zero again); without them one workgroup per 64 columns
long colsum_scratch_doubles(int cols);
hipError_t colsum_acc(const float* in, long ld, int R, int C, float* out, double* part, unsigned* ctr, hipStream_t s);
// column sums of a BLSTM layer's [R][2 x C] gradient slab added to (b_ih, b_hh) of both directions
hipError_t colsum_bias(const float* in, long ld, int R, int C, float* bih0, float* bhh0, float* bih1, float* bhh1, double* part, unsigned* ctr,
                       hipStream_t s);
// len (nullable, as gn_relu_fwd): source rows t >= len[b] are not read and the destination gets zeros there
hipError_t copy_rows(CRows src, Rows dst, int B, int T, int C, hipStream_t s, const int* len = nullptr);
// batch assembly from a device-resident corpus: see collate_kernel (crop rows, clip mel to [0,1], pad mel with 0 / F0 with -1e10)
hipError_t collate(const float* mel_cat, const float* f0_cat, const float* emb_tab, const long* row0, const int* len,
                   const int* item, int B, int T, int C, int E, float* mel, float* f0, float* emb, hipStream_t s);
// conv weight [Co][Ci][5] -> forward pack [Co][5][Cp] (zero-filled for ci >= Ci) and input-grad pack [Ci][5][Co] (taps flipped)
// wf_img / wb_img (nullable): pre-split images of wf / wb (Cp % 4 == 0, Co % 4 == 0)
hipError_t conv_pack(const float* w, int Co, int Ci, int Cp, float* wf, float* wb, float* wf_img, float* wb_img, hipStream_t s, int img_bf16 = 0);
// packed weight grad [Co][5][Cp] -> grad arena [Co][Ci][5] (overwrite)
// every conv block's per-step weight re-layout in ONE launch (seven launches of 6 - 17 us were a chain the trunk's second layer waited for)
struct ConvPackTask {
    const float* w;
    float *wf, *wb, *wf_img, *wb_img;
    int Co, Ci, Cp;
};
struct ConvPackTable {
    ConvPackTask t[8];
    int n;
    int img_bf16;
};
hipError_t conv_pack_many(const ConvPackTable& tb, hipStream_t s);
// acc: g += the unpacked gradient instead of g = (a step that accumulates onto the arena, SS_STEP_ACCUMULATE); a kernel of its own per form
hipError_t conv_unpack_grad(const float* gp, int Co, int Ci, int Cp, float* g, hipStream_t s, bool acc = false);
constexpr int CONV_UNPACK_MAX = 8;
struct ConvUnpackTask {
    const float* gp;      // packed gradient [Co][5][Cp]
    float* g;             // parameter gradient [Co][Ci][5]
    int Co, Ci, Cp;
};
struct ConvUnpackTable {
    ConvUnpackTask t[CONV_UNPACK_MAX];
    int n;
};
hipError_t conv_unpack_grads(const ConvUnpackTable& tb, hipStream_t s, bool acc = false);      // several blocks, one launch
hipError_t transpose2d(const float* in, int R, int C, float* out, hipStream_t s);   // out[c][r] = in[r][c]
// out[i] = a[i] + b[i]
hipError_t add_vec(const float* a, const float* b, float* out, int n, hipStream_t s);
// dst = a + b (b null: copy) for a table of up to PREP_MAX vectors, one launch
constexpr int PREP_MAX = 48;
struct PrepTask {
    const float* a;
    const float* b;
    float* dst;
    long n;
    float* img;           // nullable: the pre-split image of dst (GemmDesc::b_pre), written beside it; needs n % 4 == 0 and 16-byte alignment
};
struct PrepTable {
    PrepTask t[PREP_MAX];
    int n;
    int img_bf16;         // the tasks' images are plain bf16 tensors instead of format v2
};
hipError_t prep_run(const PrepTable& tb, hipStream_t s);

struct CodeSrc {          // one encoder BLSTM output feeding the decoder input (model.py:87, 223-227, 301-309)
    const float* o;       // [B, TP, ld], the 2*H real columns first
    float* d_o;           // gradient slab of the same shape (backward only)
    int H, freq, col;     // col: first column inside the decoder input
    int ld;               // row stride of o / d_o (lstm_small_ld(H))
};
hipError_t build_dec_in(const CodeSrc* src, int nsrc, const float* emb, int emb_dim, int emb_col, float* dec_in, int ld,
                        int B, int T, hipStream_t s);
hipError_t dec_in_grad(const CodeSrc* src, int nsrc, const float* d_dec_in, int ld, int B, int T, hipStream_t s);
// compact forms for a decoder input that repeats in blocks of f frames (all codes up-sampled by the same f): one row per block,
// xc / d_xc [B][T/f][ld]; d_xc holds the gradient already summed over each block's frames
hipError_t build_dec_in_compact(const CodeSrc* src, int nsrc, const float* emb, int emb_dim, int emb_col, float* xc, int ld, int B, int T,
                                int f, hipStream_t s);
hipError_t dec_in_grad_compact(const CodeSrc* src, int nsrc, const float* d_xc, int ld, int B, int T, int f, hipStream_t s);
// ---- codes as caller-owned tensors (ss_g3_encode / ss_g3_decode / ss_g6_encode / ss_g6_decode): a code is dense fp32 [B, T / freq, 2H],
//      cat(forward half at the last frame of each block, backward half at the first) (model.py:84-87, 223-227)
struct CodeOut {          // one code to export from an encoder BLSTM's output slab
    const float* o;       // [B, TP, ld], the 2*H real columns first
    float* dst;           // [B, T / freq, 2H]
    int H, freq, ld;
    int vec;              // set by export_codes: the halves move as float4
};
// every code of the table in ONE launch (up to three); len (nullable, i32[B]): zeros in code rows at or beyond len[b] / freq
hipError_t export_codes(const CodeOut* out, int n, int B, int T, hipStream_t s, const int* len = nullptr);
struct CodeIn {           // one code feeding the decoder input
    const float* p;       // [B, T / freq, 2H]
    int H, freq, col;     // col: first column inside the decoder input
};
// The decoder input from codes and speaker rows emb [B, emb_dim] (emb_dim 0: none), in either form decoder layer 0 consumes: f == 0 the
// slab dst [B, TP, ld] (halo rows untouched, as build_dec_in), f > 0 the compact dst [B, T / f, ld] (every code's freq == f, as
// build_dec_in_compact).  Padding columns are written zero.  len (nullable): rows at or behind len[b] are zeros, their codes are not read.
hipError_t dec_in_from_codes(const CodeIn* src, int nsrc, const float* emb, int emb_dim, int emb_col, float* dst, int ld, int B, int T, int f,
                             hipStream_t s, const int* len = nullptr);
struct CodeGrad {         // one code whose gradient is wanted (ss_g3_decode_backward / ss_g6_decode_backward)
    float* dst;           // [B, T / freq, 2H], dense
    int H, freq, col;     // col: first column inside the decoder input
};
// The adjoint of dec_in_from_codes for the codes (input_grads.hip): dst_i[b][blk][c] = the sum over the block's freq_i frames, frames
// ascending, of d_in[.][col_i + c].  f == 0: d_in is the slab [B, TP, ld]; f > 0: the compact [B, T / f, ld], which already holds the sums
// (every freq_i == f).  Up to three codes in ONE launch; fixed order, no atomics.
hipError_t dec_in_codes_grad(const CodeGrad* g, int n, const float* d_in, int ld, int B, int T, int f, hipStream_t s);

// loss = mean((tgt - out)^2) over B*T*C real elements (solver.py:166); d_out = 2 (out - tgt) / N * scale
hipError_t mse_loss(CRows out, CRows tgt, Rows d_out, int B, int T, int C, float grad_scale, float* partials, float* loss, hipStream_t s);
// softmax cross-entropy over C classes against integer targets in [0, C) (not checked on the device); mean over B*T rows.  Shift-invariant:
// the log-softmax is (x - max) - log(sum exp(x - max)), never through max + log(..)
hipError_t ce_loss(CRows logits, const int* tgt, Rows d_out, int B, int T, int C, float grad_scale, float* partials, float* loss, hipStream_t s);

struct LrSchedState;      // the learning-rate schedule (below); sch, nullable, in the launchers that prepare a step: NULL is "off"
struct AdamState {        // device-resident so a captured graph can replay the step
    double lr, beta1, beta2, eps;
    long step;
    float step_size, bc2_sqrt, f_beta1, f_beta2, f_eps;
    unsigned skip;        // set by adam_prepare when this step's gradients must not be applied (see adam_step)
};
// Engine status word ("sticky": host-visible, survives steps, cleared only by ss_clear_abort): bit 0 a persistent recurrence kernel's
// bounded wait expired on this rank, bit 1 another rank reported it (data parallel), bit 2 a parameter left the range the
// fixed-scale fp16 x 2 forward products are valid for (or is not finite).
constexpr unsigned SS_STICKY_ABORT = 1u, SS_STICKY_REMOTE = 2u, SS_STICKY_RANGE = 4u;
// sticky (nullable) / status (nullable: the gradient arena's status slot, summed over the ranks by the all-reduce): when
// either is non-zero the update is SKIPPED -- parameters, moments and the step counter stay as they are.
hipError_t adam_prepare(AdamState* st, unsigned* sticky, const float* status, hipStream_t s, LrSchedState* sch = nullptr);
hipError_t adam_range(float* p, const float* g, float* m, float* v, long n, AdamState* st, float grad_scale, hipStream_t s);
hipError_t adam_step(float* p, const float* g, float* m, float* v, long n, AdamState* st, float grad_scale, unsigned* sticky,
                     const float* status, hipStream_t s, LrSchedState* sch = nullptr);
// ---- gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, norm_type 2; no statement of the reference: its solver never clips)
// Device-resident beside AdamState in the workspace's first 256 bytes (byte 128), so it survives what the Adam state survives.
struct ClipState {
    float norm;           // grad_scale * ||g|| of the last optimiser step, BEFORE clipping (parameter elements only)
    float coef;           // min(1, max_norm / (norm + 1e-6)) that step applied; 0 when it was skipped as non-finite
    float clipped;        // optimiser steps with coef < 1 since ss_set_grad_clip   (floats: the four words are handed out as one float4;
    float skipped;        // optimiser steps skipped because the norm was not finite   exact up to 2^24 steps)
};
constexpr long CLIP_STATE_BYTE = 128;
// The runs of PARAMETER elements of the arena: neighbouring tensors without an alignment gap between them are one run.  Every start is
// a multiple of 4 floats; the gaps behind tensors whose element count is not (the 257-float head bias) and the status slot are in no run.
constexpr int GRAD_SEG_MAX = 96;
struct GradSegTable {
    int n;
    int len[GRAD_SEG_MAX];
    long start[GRAD_SEG_MAX];
};
// Workgroups (= float64 partials) of one grad_sumsq launch over n floats: a function of n alone, so every schedule that splits the
// arena at the same offsets adds the same partials in the same order.
constexpr int GRAD_SUMSQ_MAX_WGS = 512;
inline int grad_sumsq_wgs(long n) {
    const long w = (n / 4 + 2047) / 2048;            // >= 8 float4 per thread before a second workgroup is worth its launch slot
    return (int)(w < 1 ? 1 : (w > GRAD_SUMSQ_MAX_WGS ? GRAD_SUMSQ_MAX_WGS : w));
}
// partials[0 .. grad_sumsq_wgs(hi - lo)) = per-workgroup float64 sums of g[i]^2 over the table's elements inside [lo, hi)
// (lo a multiple of 4; float4 loads, grid-stride, no atomics)
hipError_t grad_sumsq(const float* g, const GradSegTable& tb, long lo, long hi, double* partials, hipStream_t s);
// *out = grad_scale * sqrt(partials[0] + .. + partials[n - 1])   (one workgroup, fixed order)
hipError_t grad_norm_finish(const double* partials, int n, float grad_scale, float* out, hipStream_t s);
// adam_prepare with the clip in front: norm as grad_norm_finish into clip->norm, clip->coef = min(1, max_norm / (norm + 1e-6)).
// A norm that is not finite sets st->skip for THIS step only (parameters, moments, step counter untouched; clip->skipped + 1; neither
// sticky nor the status slot is set); the sticky / status skip of adam_prepare comes first and counts as neither.
hipError_t adam_prepare_clip(AdamState* st, ClipState* clip, unsigned* sticky, const float* status, const double* partials, int n,
                             float grad_scale, float max_norm, hipStream_t s, LrSchedState* sch = nullptr);
// adam_range with g * grad_scale * *coef (a coefficient of exactly 1.0f gives adam_range's bits)
hipError_t adam_range_clip(float* p, const float* g, float* m, float* v, long n, AdamState* st, float grad_scale, const float* coef,
                           hipStream_t s);
// ---- decoupled weight decay (torch.optim.AdamW, single-tensor formulas) and an exponential moving average of the parameters
// (torch.optim.swa_utils.get_ema_avg_fn), both inside the optimiser step.  For an APPLIED step t (AdamState::skip == 0):
//   decayed element:  p1 = p * decay_mul, decay_mul = (float)(1 - lr * wd) with the current lr (not lr / bc1); Adam then acts on p1
//   every element:    ema' = ema + ema_w * (p' - ema), p' the parameter the step has just written, ema_w = (float)(1 - d_t),
//                     d_t = decay, or with warm-up min(decay, (1 + n) / (10 + n)), n = EMA updates applied before this one
// A skipped step changes none of it.  Device-resident beside AdamState and ClipState in the workspace's first 256 bytes (byte 144): the
// prepare kernels form decay_mul and ema_w in double and advance n behind their skip decisions, once per step, so every range of one step
// sees the same values.
struct OptExtState {
    float stats[4];       // {n, d_t of the last update, decay_mul of the last step, 0}: handed out as one float4 (ss_ema_stats)
    double ema_decay;
    long n;               // EMA updates applied
    float wd, decay_mul, ema_w;
    unsigned flags;       // OPT_EXT_EMA: the average is on; OPT_EXT_WARMUP: d_t warms up
};
constexpr long OPT_EXT_STATE_BYTE = 144;
constexpr unsigned OPT_EXT_EMA = 1u, OPT_EXT_WARMUP = 2u;
// Runs of the arena by "decayed or not" for weight decay on the tensors with ndim >= 2 only.  The runs cover [0, arena) without a hole
// (a tensor's run takes the alignment gap behind it; the status slot is the last run), so starts and lengths are multiples of 4 floats.
constexpr int WD_RUN_MAX = 96;
struct WdRunTable {
    int n;
    int len[WD_RUN_MAX];
    int decayed[WD_RUN_MAX];
    long start[WD_RUN_MAX];
};
// What an optimiser step does beyond Adam.  ext (nullable: both terms off -- the launchers below then do exactly what they did before
// the terms existed); wd: decay is on; runs (nullable: every element is decayed); ema (nullable: no average), the arena's base.
struct AdamExt {
    OptExtState* ext = nullptr;
    bool wd = false;
    const WdRunTable* runs = nullptr;
    float* ema = nullptr;
    bool on() const { return ext && (wd || ema); }
};
// adam_prepare / adam_prepare_clip that also set the step's decay_mul, ema_w and n (x.on(); otherwise the plain ones)
hipError_t adam_prepare_ext(AdamState* st, const AdamExt& x, unsigned* sticky, const float* status, hipStream_t s,
                            LrSchedState* sch = nullptr);
hipError_t adam_prepare_clip_ext(AdamState* st, ClipState* clip, const AdamExt& x, unsigned* sticky, const float* status, const double* partials,
                                 int n, float grad_scale, float max_norm, hipStream_t s, LrSchedState* sch = nullptr);
// adam_range / adam_range_clip (coef non-null) over the elements [lo, hi) of arenas given by their BASE pointers, with decay and the fused
// average under the step state the prepare set (lo, hi multiples of 4).  !x.on(): the plain launch on the offset pointers.
hipError_t adam_range_ext(float* p, const float* g, float* m, float* v, long lo, long hi, AdamState* st, float grad_scale, const float* coef,
                          const AdamExt& x, hipStream_t s);
// ema[i] += ema_w * (p[i] - ema[i]) over n floats (a multiple of 4) under the step state: nothing when the step was skipped
hipError_t ema_range(float* ema, const float* p, long n, const AdamState* st, const OptExtState* ext, hipStream_t s);
// a[i] <-> b[i] over n floats (a multiple of 4)
hipError_t arena_swap(float* a, float* b, long n, hipStream_t s);
// ---- learning-rate warm-up and decay, keyed on the device's own step counter.  For an APPLIED step t (1-based, the t of the bias
// corrections), s = t - 1, base = AdamState::lr:
//   warm-up (W > 0 and s < W):  lr_t = base * (sf + (1 - sf) * (s / W))
//   otherwise, k = s - W:       constant     base
//                               cosine       kk = min(k, N); min_lr + (base - min_lr) * (0.5 * (1 + cospi(kk / N)))
//                               linear       kk = min(k, N); base + (min_lr - base) * (kk / N)
//                               exponential  max(base * pow(gamma, k), min_lr)
//                               step         max(base * pow(gamma, k / P), min_lr), integer division
// in float64 without contraction, by the prepare kernels' one thread right behind st->step += 1: step_size = (float)(lr_t / bc1) and
// decay_mul = (float)(1 - lr_t * wd) are formed from that one value, so every range of one step sees it.  A skipped step changes none
// of it.  Device-resident in the workspace's first 256 bytes (byte 192), beside the Adam, clip and weight-decay / EMA states.
constexpr int LR_OFF = 0, LR_CONSTANT = 1, LR_COSINE = 2, LR_LINEAR = 3, LR_EXPONENTIAL = 4, LR_STEP = 5;
struct LrSchedState {
    float stats[4];       // {(float)lr_t of the last applied step, lr_t / base, t, kind}: handed out as one float4 (ss_lr_stats)
    double sf, gamma, min_lr;
    int W, N, P, kind;
};
constexpr long LR_SCHED_STATE_BYTE = 192;
// what ss_set_lr_schedule and ss_op_lr_schedule refuse, in one place; NULL: the options are valid
inline const char* lr_schedule_refusal(int kind, int warmup_steps, double warmup_start, int total_steps, double gamma, int period, double min_lr) {
    if (kind < LR_OFF || kind > LR_STEP) return "kind must be 0 (off), 1 constant, 2 cosine, 3 linear, 4 exponential or 5 step";
    if (kind == LR_OFF) return nullptr;         // off reads none of the others
    if (warmup_steps < 0) return "warmup_steps must be >= 0";
    if (!(warmup_start > 0.0 && warmup_start <= 1.0)) return "warmup_start must lie in (0, 1]; NaN is refused";
    if ((kind == LR_COSINE || kind == LR_LINEAR) && total_steps < 1) return "total_steps must be >= 1 for cosine and linear";
    if ((kind == LR_EXPONENTIAL || kind == LR_STEP) && !(gamma > 0.0 && gamma <= 1.0)) return "gamma must lie in (0, 1]; NaN is refused";
    if (kind == LR_STEP && period < 1) return "period must be >= 1";
    if (!(min_lr >= 0.0 && min_lr <= 1.7976931348623157e308)) return "min_lr must be >= 0 and finite; negative, NaN and inf are refused";
    return nullptr;
}
// lr[i] = lr_t at t = steps[i] under the schedule q (q.stats unused) and the base rate: the prepare kernels' own __device__ function,
// one thread per value (test hook)
hipError_t lr_schedule_eval(const LrSchedState& q, double base, const long* steps, long n, double* lr, hipStream_t s);
// *status = (*sticky != 0)   (one thread; enqueued behind the decoder's recurrences, in front of the all-reduce that sums it)
hipError_t status_publish(const unsigned* sticky, float* status, hipStream_t s);
// Scale of the fp16 x 2 split for the OUTPUT of each conv block (GroupNorm + ReLU, then resampled: a convex combination), from its affine
// parameters: |y| <= sqrt(16 T) max|gamma| + max|beta| = bound; out[i] = min(16, largest power of two with bound * scale <= 32768).
// 16 -- the scale every other forward operand uses -- whenever bound <= 2048, i.e. for any sane GroupNorm affine.  The floor is 2^-20.
// A bound of +inf (an infinite parameter, or sqrt(16 T) max|gamma| overflowing) keeps 16: param_guard reports it and the step is skipped.
// NaN elements do not enter the maxima (fmaxf); param_guard reports them too.
constexpr int ACT_SCALE_MAX = 8;
struct ActScaleTable {
    const float* gamma[ACT_SCALE_MAX];
    const float* beta[ACT_SCALE_MAX];
    int C[ACT_SCALE_MAX];
    int n;
};
hipError_t act_scales(const ActScaleTable& tb, int T, float* out, hipStream_t s);
// sticky |= SS_STICKY_RANGE if any of the n parameters is not finite or |p| >= limit
hipError_t param_guard(const float* p, long n, float limit, unsigned* sticky, hipStream_t s);

// ---------------------------------------------------------------- features.hip  (offline feature extraction, float64)
// x [n] -> S [frames][n_mels] float32, frames = (n + 256) / 256 (utils.py:18-31, make_spect_f0.py:57-60); mel [513][n_mels]
hipError_t melspec(const double* x, int n, const double* mel, int n_mels, float* out, int frames, hipStream_t s);
// utils.py:35-42 with mean / std over the voiced frames (make_spect_f0.py:64-66); -1e10 marks unvoiced frames
hipError_t f0_normalize(const double* f0, int n, float* out, hipStream_t s);

// ragged batches.  n (nullable; device i32[B]): row b has n_b = min(max(n[b], 513), max_n) samples and F_b = n_b / 256 + 1 frames of
// F = max_n / 256 + 1; it is computed as if it were alone, samples at or beyond n_b are never read, frames at or beyond F_b are filler.
constexpr int FEAT_MAX_ROWS = 65535;   // the batch is the grid's y dimension
// wav [B][max_n] -> out [B][F][n_mels] float32 with the FFT of fft_lds.h; zeros in frames at or beyond F_b
hipError_t melspec_batch(const double* wav, const int* n, int B, int max_n, const double* mel, int n_mels, float* out, hipStream_t s);
// f0 [B][F] -> out [B][F] float32: f0_normalize on each row's own F_b frames; `unvoiced` in unvoiced frames and behind F_b
hipError_t f0_normalize_batch(const double* f0, const int* n, int B, int max_n, double unvoiced, float* out, hipStream_t s);

// ---------------------------------------------------------------- filtfilt.hip  (scipy.signal.filtfilt to the bit, float64)
// x, dither (nullable), y [B][max_n]; scratch [B][max_n + 36] doubles.  y = filtfilt(b, a, x) * gain + (dither - 0.5) * dither_scale on each
// row's own n_b samples, zeros behind them.  The coefficients travel by value (struct FiltCoef, filtfilt_step.h).
constexpr int FILT_NCOEF = 6, FILT_PAD = 3 * FILT_NCOEF;    // scipy's default padlen = 3 * max(len(a), len(b))
struct FiltCoef {
    double b[FILT_NCOEF], a[FILT_NCOEF], zi[FILT_NCOEF - 1];
};
long filtfilt_scratch_bytes(int B, int max_n);
hipError_t filtfilt(const double* x, const int* n, int B, int max_n, const FiltCoef& c, double gain, const double* dither,
                    double dither_scale, double* y, double* scratch, hipStream_t s);

// ---------------------------------------------------------------- resample.hip  (scipy.signal.resample_poly to the bit, float64)
// x [B][max_n], h [n_taps] (device; n_taps odd), y [B][M], M = resample_len(max_n, up, down).  n (nullable; device i32[B]): row b has
// n_b = min(max(n[b], 1), max_n) samples and m_b = resample_len(n_b, up, down) outputs; y[b][m] = 0.0 + sum_k x[b][k] h[m down + half - k up]
// over the k in [0, n_b) whose tap exists, k ascending; zeros in columns m_b .. M - 1; x at or beyond n_b is never read.
constexpr int RESAMPLE_MAX_RATE = 1024;
long resample_len(long n, int up, int down);                 // ceil(n up / down)
long resample_scratch_bytes(int up, int n_taps);             // 0: the kernel reads h as it is given
hipError_t resample(const double* x, const int* n, int B, int max_n, int up, int down, const double* h, int n_taps, double* y, hipStream_t s);

// ---------------------------------------------------------------- silence.hip  (trim the ends, cap the pauses: float64, to the bit)
// x, y [B][max_n]; Jmax = silence_blocks(max_n) blocks of 256 samples; e [B][Jmax] levels (zeros behind a row's J_b blocks); inv [B][Jmax] the
// kept blocks ascending (-1 behind the K kept ones), k [B]; m [B] the new lengths.  n (nullable; device i32[B]): row b has
// n_b = min(max(n[b], 1), max_n) samples; nothing at or beyond n_b is read.  include/speechsplit_amd.h states the definition.
constexpr int SIL_MAX_BLOCKS = 8191;   // 256 * SIL_MAX_BLOCKS samples a row at most: the mask kernel's LDS holds a row's blocks
struct SilenceScratch {
    double* e;
    int *inv, *k;
};
int silence_blocks(int max_n);
long silence_scratch_bytes(int B, int max_n);
SilenceScratch silence_scratch(void* base, int B, int max_n);
hipError_t silence_levels(const double* x, const int* n, int B, int max_n, double* e, hipStream_t s);
// cnt (nullable) holds a row's samples (cnt_is_samples: the n above) or its blocks, clamped into 1 .. Jmax
hipError_t silence_mask(const double* e, const int* cnt, bool cnt_is_samples, int B, int max_n, double ratio, int hang, int edge, int pause,
                        int* inv, int* k, hipStream_t s);
// g: host [128], the fade-in gains; inv and k are read with every index clamped into the row's own blocks
hipError_t silence_gather(const double* x, const int* n, int B, int max_n, const int* inv, const int* k, const double* g, double* y, int* m,
                          hipStream_t s);

// ---------------------------------------------------------------- mtrand.hip  (numpy.random.RandomState.rand to the bit: MT19937)
// state u32[625] on the device, in/out: numpy's key [624], then pos (above 624 reads as 624).  out [count] float64: draw i is
// ((w[2i] >> 5) 2^26 + (w[2i+1] >> 6)) / 2^53 of the tempered stream words w from pos on.  Afterwards the state is what numpy holds after the
// same draws: the whole last regenerated block and pos' = pos + 2 count - 624 ((pos + 2 count - 1) / 624).  count == 0: nothing is enqueued.
constexpr long MT_MAX_COUNT = 1L << 40;
hipError_t mt19937_rand(unsigned* state, long count, double* out, hipStream_t s);
// draws [count], first i64[B], n i32[B] (all device) -> out [B][max_n]: out[b][i] = draws[first[b] + i] for i < n_b = min(max(n[b], 0), max_n),
// zeros behind; first[b] is clamped into [0, max(count - n_b, 0)] and nothing outside draws[0 .. count) is read
hipError_t dither_rows(const double* draws, long count, const long* first, const int* n, int B, int max_n, double* out, hipStream_t s);

// ---------------------------------------------------------------- vocoder.hip  (Griffin-Lim: mel -> linear magnitude -> waveform, float64)
// Shapes: mel [B][max_frames][n_mels] f32, mag [B][max_frames][513], spec [B][max_frames][513][2] (re, im), wav [B][256 (max_frames - 1)].
// frames (nullable; device i32[B]): row b has F_b = min(max(frames[b], 4), max_frames) frames and 256 (F_b - 1) samples; it is computed as if
// it were alone, mel / mag / spec / phase0 frames at or beyond F_b are never read, outputs behind a row's own extent are zeros.
constexpr int VOC_MAX_ROWS = 65535;   // the batch is the grid's y dimension
constexpr int VOC_MAX_MELS = 4096;    // one frame's amplitudes sit in LDS
struct VocoderScratch {
    double* frame_buf;   // [B][max_frames][1024]   window * irfft of every frame, what the overlap-add gathers from
    double* proj;        // [B][max_frames][513][2] S ang, the spectrum the next ISTFT takes
    double* tprev;       // [B][max_frames][513][2] the previous round's STFT
};
long vocoder_scratch_bytes(int B, int max_frames);
VocoderScratch vocoder_scratch(void* base, int B, int max_frames);
// mag = max(floor, 10^((100 mel - 100 + 16) / 20) . inv_basis), inv_basis [n_mels][513]
hipError_t mel_to_linear(const float* mel, const double* inv_basis, const int* frames, int B, int max_frames, int n_mels, double floor,
                         double* mag, hipStream_t s);
// Non-negative mel inversion by projected FISTA, one workgroup per frame, the whole iteration in one launch (see vocoder.hip).  packed is
// ss_mel_nnls_pack's form of the [513][n_mels] basis: per band (first bin, run length), then the bands' runs of weights; it sits in LDS with
// amp, r and y, mel_nnls_lds_bytes(n_mels, packed_doubles) bytes -- at NNLS_MAX_PACKED no more than 40980, under the 64 KiB a launch gets
// without asking.  n_iter == 0 is mel_to_linear to the bit.
constexpr long NNLS_MAX_PACKED = 3072;
long mel_nnls_lds_bytes(int n_mels, long packed_doubles);
hipError_t mel_to_linear_nnls(const float* mel, const double* inv_basis, const double* packed, long packed_doubles, const int* frames, int B,
                              int max_frames, int n_mels, int n_iter, double step, double floor, double* mag, hipStream_t s);
// F0-guided harmonic inversion (see vocoder.hip and the header): on the voiced frames of f0_hz [B][max_frames] (Hz; voiced: 40 .. 1000) one
// amplitude per harmonic is fitted to the mel by projected FISTA, one workgroup per frame, and mag (in/out) and share (out) are written;
// every other frame keeps its mag and gets share 0.  The LDS image is the NNLS one plus the model, its gradient and the harmonics' atoms:
// mel_harmonic_lds_bytes(n_mels, packed_doubles), 41804 bytes for 80 bands at NNLS_MAX_PACKED and at most 53452 (1536 empty bands).
constexpr int HARM_MAX = 190;         // harmonics a frame can have: 7600 / 40
long mel_harmonic_lds_bytes(int n_mels, long packed_doubles);
hipError_t mel_to_linear_harmonic(const float* mel, const double* f0_hz, const double* inv_basis, const double* packed, long packed_doubles,
                                  const int* frames, int B, int max_frames, int n_mels, double f_top, int n_iter, double floor,
                                  double* mag, double* share, hipStream_t s);
// u [B][max_frames]: the fundamental's phase at the frame centres in cycles, one wave per row (the recurrence is serial)
long harmonic_phase_scratch_bytes(int B, int max_frames);
hipError_t harmonic_u(const double* f0_hz, const int* frames, int B, int max_frames, double* u, hipStream_t s);
// harmonic_u into u, then phase0 = arg(share e^{i phi_h} + sqrt(1 - share^2) e^{i rand}) on voiced frames, rand elsewhere (nullptr: zeros)
hipError_t harmonic_phase(const double* f0_hz, const double* share, const double* rand, const int* frames, int B, int max_frames,
                          double f_top, double* phase0, double* u, hipStream_t s);
// melspec_kernel's framing with a 1024-point FFT in LDS, one workgroup per frame
hipError_t stft(const double* wav, const int* frames, int B, int max_frames, double* spec, hipStream_t s);
// window * irfft per frame into frame_buf, then a gather per output sample over the frames that cover it, over the sum of their squared windows
hipError_t istft(const double* spec, const int* frames, int B, int max_frames, double* wav, double* frame_buf, hipStream_t s);
// Griffin-Lim with momentum (see vocoder.hip); phase0 [B][max_frames][513] or nullptr (zeros).  1 + 3 n_iter + 2 launches.
hipError_t griffinlim(const double* mag, const double* phase0, const int* frames, int B, int max_frames, int n_iter, double momentum,
                      double* wav, const VocoderScratch& sc, hipStream_t s);

// ---------------------------------------------------------------- pitch.hip  (RAPT-style pitch tracker: waveform -> ln F0 per hop, float64)
// Shapes: wav [B][max_n], phi [B][F][K], rms [B][F], f0 [B][F] with F = max_n / 256 + 1 and K = lmax - lmin + 1 lags.
// n (nullable; device i32[B]): row b has n_b = min(max(n[b], 513), max_n) samples and F_b = n_b / 256 + 1 frames; it is computed as if it were
// alone, samples at or beyond n_b are never read, phi / rms beyond F_b are zeros and f0 beyond F_b is -1e10.
constexpr int PITCH_MAX_ROWS = 65535;                      // the batch is the grid's y dimension
constexpr int PITCH_STATES = 20;                           // the unvoiced state and at most 19 candidates per frame
constexpr int PITCH_MIN_LAG = 16, PITCH_MAX_LAG = 400;     // 1000 Hz .. 40 Hz at 16 kHz: the segment (120 + lmax samples) sits in LDS
struct PitchLags {
    int lmin, lmax;      // floor(16000 / hi_hz), ceil(16000 / lo_hz)
};
// false if a bound is NaN or not positive, not lo < hi, or the lags leave PITCH_MIN_LAG .. PITCH_MAX_LAG or are fewer than 3
bool pitch_lags(double lo_hz, double hi_hz, PitchLags* g);
struct PitchScratch {
    double* phi;         // [B][F][K]   the NCCF (ss_pitch_track only; the hook takes the caller's)
    double* rms;         // [B][F]      likewise
    double* cost;        // [B][F][20]  local cost per state
    double* lag;         // [B][F][20]  refined lag per state (entry 0 unused)
    double* lnlag;       // [B][F][20]  its logarithm
    int* cnt;            // [B][F]      states in use
    unsigned char* bp;   // [B][F][32]  backpointers
};
long pitch_scratch_bytes(int B, int max_frames, int K);
PitchScratch pitch_scratch(void* base, int B, int max_frames, int K);
// the same scratch with the stationarity track S [B][F] behind it (256-byte aligned), and where that track begins
long pitch_stat_scratch_bytes(int B, int max_frames, int K);
double* pitch_stat_track(void* base, int B, int max_frames, int K);
// steps 1 and 2 of the header's algorithm: one workgroup per (frame, utterance)
hipError_t pitch_nccf(const double* wav, const int* n, int B, int max_n, double scale, const PitchLags& g, double* phi, double* rms,
                      hipStream_t s);
// steps 3 and 4, the recurrence and the backtrack: a frame-parallel candidate kernel, then one wavefront per utterance.  stat [B][F]
// (nullable): the stationarity track, added to the voicing transitions (dp_kernel<true>); null runs the tracker without the term
hipError_t pitch_dp(const double* phi, const double* rms, const double* stat, const int* n, int B, int max_n, const PitchLags& g, double* f0,
                    const PitchScratch& sc, hipStream_t s);
// the header's "spectral stationarity": S_i per frame from two LPC analyses, one workgroup per (frame, utterance); stat [B][F]
hipError_t pitch_stationarity(const double* wav, const int* n, int B, int max_n, double scale, double* stat, hipStream_t s);

// ---------------------------------------------------------------- dtw.hip  (conversion scores: cepstra, DTW path and cost, F0 error along a path)
// Shapes: mel [B][max_t][n_mels] f32, dct [n_ceps][n_mels], cepstra [B][max_t][n_ceps]; fx [B][max_tx][dim], fy [B][max_ty][dim],
// out [B][3] (total, P, mcd), path [B][max_tx + max_ty - 1][2] (i, j; -1 beyond P), path_len [B]; f0x [B][max_tx], f0y [B][max_ty],
// stats [B][5] (n_vv, n_vu, f0_rmse_cents, f0_corr, vuv_error).  Lengths (nullable; device i32[B]): a row has min(max(len[b], 1), max)
// frames, is computed as if it were alone, and frames at or beyond its length are never read.
constexpr int DTW_MAX_ROWS = 65535;   // ss_dtw_scratch_bytes' corner: the product stays inside a long
constexpr int DTW_MAX_DIM = 40;       // a row of fx sits in registers: 80 VGPRs at 40 doubles
constexpr int DTW_STRIP = 64;         // rows of the lattice swept at a time, one per lane of a wavefront
struct DtwScratch {
    unsigned char* bp;   // [B][bp_stride]    backpointers, 2 bits a cell: row i of a pair at i * ceil(max_ty / 4)
    double* brow;        // [B][brow_stride]  the bottom row of D of the strip before
    long bp_stride, brow_stride;
};
long dtw_scratch_bytes(int B, int max_tx, int max_ty);
DtwScratch dtw_scratch(void* base, int B, int max_tx, int max_ty);
hipError_t mel_cepstra(const float* mel, const int* len, int B, int max_t, int n_mels, const double* dct, int n_ceps, double* out,
                       hipStream_t s);
// one workgroup of four wavefronts per pair: the recurrence over row strips, the backtrack and the path, in one launch; path and path_len
// may both be nullptr
hipError_t dtw(const double* fx, const int* tx, const double* fy, const int* ty, int B, int max_tx, int max_ty, int dim, double scale,
               double* out, int* path, int* path_len, const DtwScratch& sc, hipStream_t s);
hipError_t path_f0_stats(const int* path, const int* path_len, const double* f0x, const double* f0y, int B, int max_tx, int max_ty,
                         double* out, hipStream_t s);

// ---------------------------------------------------------------- stoi.hip  (waveform scores: STOI and ESTOI of y against an aligned x at 10 kHz)
// Shapes: x, y [B][max_n]; with F = stoi_frames(max_n), L = 128 (F - 1) + 256, M = F - 1, S = M - 29 (StoiShape): e [B][F] frame levels in
// dB, inv i32 [B][F] (inv[slot] = frame, -1 behind the K kept frames), K i32 [B], xp, yp [B][L], envelopes [B][n_bands][M], d [B][S],
// out [B][3] (score, S, K).  n (nullable; device i32[B]): a row has min(max(n[b], 1), max_n) samples, is computed as if it were alone,
// and samples at or beyond its length are never read.
constexpr int STOI_MAX_ROWS = 65535;  // rows ride on gridDim.y
constexpr int STOI_MAX_BANDS = 32;    // a band per thread of the segment kernel's wavefront, 30 frames of each in its LDS
constexpr int STOI_FRAME = 256, STOI_HOP = 128, STOI_SEG = 30;
constexpr double STOI_RANGE_DB = 40.0, STOI_BETA_DB = -15.0;
__host__ __device__ inline int stoi_frames(int n) { return n >= STOI_FRAME ? (n - STOI_FRAME) / STOI_HOP + 1 : 0; }
struct StoiTables {                   // passed to the kernels by value: the host's own cosine makes the window
    double w[STOI_FRAME];             // 0.5 - 0.5 cos(2 pi (i + 1) / 257)
    int lo[STOI_MAX_BANDS], hi[STOI_MAX_BANDS], n_bands;      // band j sums bins lo[j] .. hi[j] - 1 of the 512-point transform
};
struct StoiShape {
    int F, L, M, S;                   // frames, compacted samples, transform frames and segments a row of max_n samples can have
};
struct StoiScratch {
    double* e;
    int *inv, *K;
    double *xp, *yp, *ex, *ey, *d;    // ex, ey are laid out for the n_bands of the call, inside room for STOI_MAX_BANDS
};
StoiShape stoi_shape(int max_n);
int stoi_bands_frames(int max_len);   // transform frames of a signal of max_len samples: the starts 128 m strictly below max_len - 256
long stoi_scratch_bytes(int B, int max_n);
StoiScratch stoi_scratch(void* base, int B, int max_n);
void stoi_tables(const int* band_lo, const int* band_hi, int n_bands, StoiTables* tb);      // host: the window and the band edges
// energies, mask and map (skipped with from_map: inv and K are then inputs, and e is not touched), then the compacting overlap-add
hipError_t stoi_compact(const double* x, const double* y, const int* n, int B, int max_n, const StoiTables& tb, bool from_map, double* e,
                        int* inv, int* K, double* xp, double* yp, hipStream_t s);
// band envelopes of sig [B][max_len] (len nullable) -> env [B][n_bands][stoi_bands_frames(max_len)]
hipError_t stoi_bands(const double* sig, const int* len, int B, int max_len, const StoiTables& tb, double* env, hipStream_t s);
hipError_t stoi(const double* x, const double* y, const int* n, int B, int max_n, const StoiTables& tb, int extended, double* out,
                const StoiScratch& sc, hipStream_t s);

// ---------------------------------------------------------------- lstm_small.hip  (hidden <= 32: whole recurrence in one launch)
// Row stride of a small BLSTM's output, cell-state and output-gradient slabs: 2H for H a power of two (the default widths keep their
// layout), else 2H rounded up to a multiple of 4 floats (16-byte rows: vector loads and the GEMMs' aligned path).  The padding columns
// are never written: zero, like the halo rows.  (Hidden sizes above 32 use 2H: the decoder's 256 / 512.)
constexpr int lstm_small_ld(int H) { return (H > 32 || (H & (H - 1)) == 0) ? 2 * H : (2 * H + 3) & ~3; }
// gates: [B, TP, 8H] holds x.W_ih^T + b_ih + b_hh on entry (column = dir*4H + gate*H + j, gate order i,f,g,o) and the
// activated gates on exit.  out: [B, TP, lstm_small_ld(H)].  csave: the cell states, same geometry.  whh: [2][4H][H].  H in 1..32.
// len (nullable; device i32[B]): ragged eval-mode batch.  Row b's recurrence covers its own L = min(max(len[b], 0), T) frames (the reverse
// direction starts at frame L - 1 from the zero state); out and csave are zero for t >= L; gates rows t >= L are neither read nor written.
hipError_t lstm_small_fwd(float* gates, const float* whh_f, const float* whh_b, float* out, float* csave, int B, int T,
                          int H, hipStream_t s, const int* len = nullptr);
// d_out: [B, TP, lstm_small_ld(H)] gradient of out.  gates is replaced in place by the pre-activation gradients.
hipError_t lstm_small_bwd(float* gates, const float* whh_f, const float* whh_b, const float* d_out, const float* csave,
                          int B, int T, int H, hipStream_t s);

// ---------------------------------------------------------------- lstm_step.hip  (hidden % 64 == 0: one launch per time step)
// MFMA operands are streamed from fragment-major copies (see lstm_step.hip):
//   wfrag  [2][H/16][4][H/16][64][4]   W_hh for the forward step        (lstm_pack_w, transposed = 0)
//   wfragT [2][H/16][4H/16][64][4]     W_hh^T for the backward step     (lstm_pack_w, transposed = 1)
//   hf     [2 ping-pong][2][ceil(B/16)][H/16][64][4]    h(t)   written by the forward epilogue, zero before step 0
//   gf     [2 ping-pong][2][ceil(B/16)][4H/16][64][4]   da(t)  written by the backward epilogue, zero before step 0
hipError_t lstm_pack_w(const float* whh_f, const float* whh_b, float* frag, int H, int transposed, hipStream_t s);
// len (nullable; device i32[B]): ragged eval-mode batch, rows at frames t >= min(max(len[b], 0), T) leave the step with c = h = 0
hipError_t lstm_step_fwd(float* gates, const float* wfrag, const float* hf_cur, float* hf_next, float* out, float* csave,
                         int B, int T, int H, int step, hipStream_t s, const int* len = nullptr);
// dc: [2][B][H] running cell-state gradient (no initialisation needed).
hipError_t lstm_step_bwd(float* gates, const float* wfragT, const float* gf_cur, float* gf_next, const float* d_out,
                         const float* csave, float* dc, int B, int T, int H, int step, hipStream_t s);

// ---------------------------------------------------------------- lstm_seq.hip  (persistent: one launch per layer)
// gates / out / csave / d_out as above; whh_* are the parameter tensors themselves ([4H][H] row-major): each workgroup
// splits its slice into fp16 x 2 pieces once and keeps it in registers.  xbuf = lstm_seq_xbytes() bytes of exchange buffer
// (forward: h(t) as fp16 pieces in MFMA fragment order; backward: partial-dh tiles, whose dwords carry their step's tag in bit 0),
// sync = LSTM_SEQ_SYNC_WORDS unsigned words (completion flags, XCD masks, abort word at [0]); both must be all zero at launch.
constexpr int LSTM_SEQ_SYNC_WORDS = 2048;   // [0] abort, [1..) XCD masks per group, [64 + 32*group + member] completion flags
bool lstm_seq_supported(int B, int H);
long lstm_seq_xbytes(int B, int H, bool backward);
// A launch on exchange tags or sync words that are not zero waits out its bounded spin and sets the sticky abort word, so the launcher
// zeroes both itself unless state_zeroed says that the caller has.
struct SeqFwd {
    unsigned* sticky = nullptr;    // engine-wide word, host-visible, that a launch ORs 1 into when its bounded wait expires (never cleared by a step)
    // xc / xf: a layer whose input repeats in blocks of xf frames -- input projections given once per block [B][T/xf][8H]
    const float* xc = nullptr;
    int xf = 0;
    float* out_img = nullptr;      // pre-split image of `out` (GemmDesc::a_pre / b_pre), same shape
    bool img_bf16 = false;         // out_img is the plain bf16 tensor, not a format-v2 image
    bool hi_only = false;          // products from the high fp16 pieces alone
    bool state_zeroed = false;     // the caller has zeroed xbuf and sync itself
    bool time_major = false;       // the slabs are [T+4][B][C] instead of [B][T+4][C]
    // ragged eval-mode batch, device i32[B] -- after the cell update of a step at frame t, rows with t >= min(max(len[b], 0), T) take
    // c = h = 0 (select), and the zero h goes through the hand-off with the step's tag
    const int* len = nullptr;
};
hipError_t lstm_seq_fwd(float* gates, const float* whh_f, const float* whh_b, void* xbuf, float* out, float* csave, unsigned* sync, int B, int T,
                        int H, hipStream_t s, const SeqFwd& o = {});
struct SeqBwd {
    unsigned* sticky = nullptr;    // as SeqFwd's
    // device word that receives max |pre-activation gradient| written (atomic max of the float's bit pattern; zero it first) -- the scale
    // the fp16 x 2 GEMMs that consume the gradient slab need
    float* amax = nullptr;
    // [2][4H] gradient accumulators of (b_ih, b_hh) of the forward / reverse direction; the kernel adds the sum over utterances and time
    // of the pre-activation gradients to both halves (f32 atomics)
    float *gbias_f = nullptr, *gbias_b = nullptr;
    // dgs / xf: a layer whose input repeats in blocks of xf frames -- pre-activation gradients additionally written summed per block
    // [B][T/xf][8H]
    float* dgs = nullptr;
    int xf = 0;
    float* dimg = nullptr;         // the gradients also as a plain bf16 tensor (slab geometry)
    bool img_only = false;         // (with dimg) the gradients ONLY as the bf16 tensor
    bool hi_only = false;          // products from the high fp16 pieces alone
    bool state_zeroed = false, time_major = false;      // as SeqFwd's
};
hipError_t lstm_seq_bwd(float* gates, const float* whh_f, const float* whh_b, void* xbuf, const float* d_out, const float* csave, unsigned* sync,
                        int B, int T, int H, hipStream_t s, const SeqBwd& o = {});

// ---- lstm_wgrad.hip: weight and bias gradients of the encoder BLSTMs (H <= 32), every layer of every block in one launch
constexpr int WGRAD_MAX = 8;
struct WgradTask {
    const float* dG;          // pre-activation gradients [R][8H] (halo rows zero)
    const float* X;           // the layer's input rows [R][In], row stride x_ld
    long x_ld;
    const float* Hout;        // the layer's output [R][2H], row stride h_ld (halo rows zero)
    float *gwih0, *gwih1;     // += dW_ih of the forward / reverse direction [4H][In]
    float *gwhh0, *gwhh1;     // += dW_hh [4H][H]
    float *gbih0, *gbhh0, *gbih1, *gbhh1;      // += bias gradients [4H] (b_ih and b_hh have the same gradient)
    int H, In;
    long R;
    int tile0;                // first blockIdx.y of this task: lstm_small_wgrad_tiles(H, In) tiles each
    int h_ld;                 // row stride of Hout (>= 2H)
};
struct WgradTable {
    WgradTask t[WGRAD_MAX];
    int n, tiles_total, row_groups;
    float* part;              // scratch: tiles_total * row_groups * 4096 floats
    unsigned* ctr;            // tiles_total arrival counters, zero at rest
};
int lstm_small_wgrad_tiles(int H, int In);
hipError_t lstm_small_wgrad(const WgradTable& tb, hipStream_t s);

// seq_gate: the stream goes on once the persistent recurrence that owns `sync` is resident (all groups through round 0), see lstm_seq.hip;
// lstm_seq_free_xcds: how many of the 8 XCDs such a launch leaves free (0: none, or not a persistent shape)
hipError_t seq_gate(const unsigned* sync, int B, int H, hipStream_t s);
int lstm_seq_free_xcds(int B, int H);

// streaming pre-read (results unused) of the slabs a persistent recurrence is about to consume: wide [rows][cw] (gates) and one or two
// narrow ones [rows][cn] (cell states; output gradient), both ends of the sequence first.  Meant for a side stream, beside the recurrence.
struct Prewarm {
    const float *n0 = nullptr, *n1 = nullptr;      // the narrow slabs
    int cn = 0;                                    // their row width
    bool time_major = false;                       // as SeqFwd's
};
hipError_t slab_prewarm(const float* wide, int cw, float* sink, int B, int T, hipStream_t s, const Prewarm& o = {});

// ---------------------------------------------------------------- input_grads.hip (gradients w.r.t. the network inputs, on request)
// conv weight [Co][Ci][5] -> input-gradient pack wb [Ci][5][Co] (taps flipped) alone, any Ci / Co (the layer-0 blocks)
hipError_t conv_pack_dx(const float* w, int Co, int Ci, float* wb, hipStream_t s);
// out[b][j] = sum_{r < rows} sum_{g < 2 * H4} dg[b * b_stride + r * ld + g] * W(g, col0 + j), W = [w_f ; w_r] ([H4][w_ld] each), j < E:
// the gradient of a per-utterance input row that a BLSTM layer sees at every frame (the decoder's speaker columns).  Fixed-order fp32 sums.
hipError_t spk_grad(const float* dg, long ld, long b_stride, int rows, const float* w_f, const float* w_r, long w_ld, int col0, int H4, int E,
                    float* out, int B, hipStream_t s);

// ---------------------------------------------------------------- queue_probe.hip (ss_bind)
// three fresh streams that, as far as the device's queue count allows, share no hardware queue with `main` or each other; `report` says
// which candidates were taken.  0, or -1 with ss_last_error() set.
int pick_streams(hipStream_t main, hipStream_t branch[3], std::string& report);

}  // namespace ss
