// Host-side engine: parameter table, workspace plan and the forward / backward / training-step schedules of
// Generator_3 and Generator_6 over the kernels in this directory, behind the C ABI of include/speechsplit_amd.h.
//
// Mirrors (does not translate) reference model.py:46-351 and solver.py:157-172: same operators in the same
// order, but activations live in haloed time-major slabs (kernels.h), the three InterpLnr calls of Encoder_7
// operate on one fused 768-channel slab, channel concats / splits / transposes are pointer arithmetic, and
// every contraction is the one fp32 MFMA GEMM.
#include <dlfcn.h>
#include <array>
#include <map>
#include <string>
#include <vector>
#include <algorithm>
#include <utility>
#include <type_traits>
#include <iterator>
#include <cstring>
#include <cstdio>

#include "common.h"
#include "abi.h"
#include "knobs.h"
#include "kernels.h"
#include "../../include/speechsplit_amd.h"

using namespace ss;

namespace ss {
int g_fwd_f16x2 = 1;   // 1: forward contractions (operands bounded by construction: mel, one-hot, GroupNorm/ReLU outputs, |h| < 1, weights)
                       //    use the fp16 x 2 split (3 MFMAs) instead of bf16 x 3 (6 MFMAs); gradients keep bf16 x 3 (their range is not bounded)
int g_bwd_f16x2 = 1;   // 1: the decoder's and the conv trunk's gradient GEMMs also use fp16 x 2: the gradient operand is scaled by the power
                       //    of two its producer kernel measured (max |value| of the slab), the activation / weight operand by the fixed one
int g_overlap = 1;     // 1: weight-gradient GEMMs on the side stream
int g_dx_batched = 2;  // input-gradient GEMMs per utterance without halo rows; 2: with 128 x 128 tiles from 512 workgroups on
int g_defer_dw = 1;    // 1: the decoder's weight-gradient GEMMs start after its last input gradient (see lstm_bwd)
int g_dp_emulate = 0;      // with dp_model = N: the stand-in collectives multiply their range by N (the sum of N identical ranks), see dp_scale_kernel
int g_dp_model = 0;        // > 1: MODEL a data-parallel run of that many ranks on one GPU: every collective is replaced by a stand-in kernel of
                           // the modelled duration (tools/dp_timeline.sh); no communicator needed
int g_dp_buckets = 1;      // 1: per-layer gradient buckets on the communication stream; 0: round 2's two buckets
int g_bf16_img = 1;        // SS_PRECISION_BF16: the 16-bit data path (round 4) -- operand images are plain bf16 tensors written by their producers (weights,
                           // hidden states, resampled activations, pre-activation / conv-output gradients) and the contractions over them run on the
                           // single-piece form of the image GEMM; 0: round 3's bf16 mode (fp32 slabs, operands rounded inside the GEMM)
                           // (a decoder layer whose gradient consumers all read the bf16 tensor does not get the fp32 copy of its pre-activation gradients,
                           // and the persistent recurrences multiply the high fp16 pieces only: one MFMA per product, half the forward's payload)
int g_compact0 = 1;        // decoder layer 0: input projections, input gradient and W_ih gradient once per block of repeated input frames
int g_persist = 1;     // 1: decoder recurrences run as ONE persistent launch per layer (lstm_seq.hip) when the batch fits
// (hipGraph capture + replay of the fused step: built and measured in rounds 1-3 -- no gain while the step is GPU-bound, and a crash inside
// the ROCm 7.2 runtime's hipGraphLaunch with more parallel branches -- and deleted in round 4; the step is enqueued eagerly.)
int g_own_streams = 0; // 1: every C-ABI call runs on the ENGINE's own main stream (created back to back with its three branch streams at
                       //    ss_bind), ordered behind the caller's stream on entry and in front of it on exit.  Built to make the step time
                       //    independent of how many streams the process created earlier -- it does not: HIP hands a new stream the
                       //    least-loaded of its 4 hardware queues, and which engine stream ends up sharing a queue with the caller's still
                       //    moves the step by 5 % either way (profiles/r02/stream_order_effect.txt: 6.70 - 7.13 ms owned, 6.69 - 7.38 not).
                       //    Off by default until the engine can measure and pick its queue placement.
int g_prio_order = 1;  // 1: within every phase the critical-path launches are ENQUEUED first and the work that only has to be done by the end of
                       //    the step (decoder / encoder-BLSTM weight gradients, Encoder_t) last.  HIP multiplexes streams onto 4 in-order hardware
                       //    queues; when two engine streams share one (other streams in the process, e.g. RCCL's, shift the assignment), enqueue
                       //    order is execution order, and filler work enqueued first would run in front of the critical path.
int g_probe_queues = 1; // 1: ss_bind measures which candidate streams share a hardware queue and picks branch streams that do not (pick_streams)
int g_gn_gather = 1;    // training forward of the independent trunk chains: GroupNorm + ReLU + resampling gather in one kernel (gn_relu_gather)
int g_conv_dw_off = 1;      // Generator_6 (one trunk chain, the second branch stream idle behind lstm's backward): the conv blocks' weight-gradient GEMMs leave
                        // the dependent chain gn backward -> input gradient -> next block for that stream; every block then keeps its own conv-output
                        // gradient slab (d_act_l).  With Encoder_t's backward in front of the BLSTMs' weight gradients (backward_encoder): 2.26 -> 2.17 ms (bf16), 2.50 -> 2.47 (fp32).  Generator_3 has no idle stream there
                        // (tools/real_timeline.py: its four streams end within ~100 us of each other)
int g_dec_tail_split = 9;   // one-GPU step: on the side stream alone the decoder's twelve weight-gradient GEMMs end ~450 us after every other stream
                        // (tools/real_timeline.py).  Layer 0's and the head's leave it for 1: the pitch chain's stream (behind the chain), 2: the third
                        // branch stream (in FRONT of its own work: they start with layer 2's), 3: the main stream (behind the trunk); 4-6 move layer 1
                        // as well (4: -> third, 5: layer 1 -> third + layer 0 -> pitch stream, 6: layer 1 -> pitch stream + layer 0 -> third); 7-10: as
                        // 2 plus single GEMMs of layer 1's reverse direction (7: dW_ih -> third, dW_hh -> pitch; 8: both -> third; 9: dW_hh -> third;
                        // 10: 9 + layer 2's reverse dW_hh -> third).  64 x 128 fp32: 5.16 / 5.05 / 5.04 / 5.16 / 5.03 / 5.12 / 5.14 ms for 0..6;
                        // 2 / 7 / 8 / 9 / 10 on another box: 5.07 / 5.06 / 5.07 / 5.01 / 5.01.  16 x 128: 3.26 -> 3.20 with 2 or 9; the 16-bit mode does
                        // not care (its weight gradients are batched per layer and its end of step is a dependent chain).  With 9 all four streams end
                        // within 200 us of each other under full contention.  Data parallel: layer 0 + head behind the pitch chain on the third stream
                        // +2.5-4 %; layer 0's forward direction + head at the very end of the third stream's and its reverse direction at the end of
                        // the main stream's enqueue order: 5.245 -> 5.226 ms at 64 x 128, +3-5 % at B <= 32: not done.
                        // (Until dec_late took the main stream by pointer, a caller on the null stream -- every PyTorch caller on its default stream --
                        // silently got 0's placement for layer 0 and the head under 3.  The 5.16 quoted for 3 above equals 0's figure and was
                        // PROBABLY taken on such a caller, i.e. is 0's schedule; that is a supposition, nobody has re-measured it, and the real
                        // main-stream placement of 3 is unmeasured.)
int g_early_dw = 0;     // 16-bit data path, B <= 48: decoder layer l + 1's weight gradients as work-queue image GEMMs on the XCDs the backward recurrence of
                        // layer l leaves free (lstm_bwd), instead of beside the encoder backward at the end of the step.  Off: 2.99 -> 2.97 ms at
                        // 32 x 128, 2.68 -> 2.67 at 16, 3.38 -> 3.35 at 48 (tools/real_timeline.py): a work-queue launch ends only when the workgroups
                        // parked on the recurrence's XCDs have run, i.e. with the recurrence, so ONE launch fits a recurrence and the layer's second
                        // one starts with the next recurrence (which it delays: 289 -> 357 us); the recurrence beside a launch stretches 283 -> 297 us;
                        // and the end of the step barely moves, because the encoder backward there is a dependent chain (~700 us at B = 32), not
                        // throughput the decoder's GEMMs were taking.
int g_xcd_dw = 0;       // decoder W_ih gradients beside the backward recurrences on the XCDs they leave free (B <= 48), see ss_engine::wq_pool.
                        // Off: measured 4.16 vs 4.09 ms at 32 x 128, 3.57 vs 3.53 at 16 x 128 -- the GEMM does run on the free XCDs beside the
                        // recurrence, but each recurrence stretches by ~40 us (its operand fetches share HBM with the GEMM's streams), the image
                        // pass and the split-K reduce land beside the input-gradient GEMM on the critical path, and at B <= 32 the encoder
                        // backward that loses the work is chain-bound, not throughput-bound (profiles/r03/xcd_overlap.txt)

// the error string behind ss_last_error(): ONE object for every translation unit that refuses through fail() (abi.h)
thread_local std::string g_err;
int fail(const std::string& m) {
    g_err = m;
    return -1;
}
}

namespace {

struct ParamInfo {
    std::string name;
    long offset;
    int ndim;
    long shape[3];
    long numel() const { return shape[0] * (ndim > 1 ? shape[1] : 1) * (ndim > 2 ? shape[2] : 1); }
};

struct ConvBlk {
    int Ci = 0, Co = 0, Cp = 0;
    long w = 0, b = 0, ga = 0, be = 0;     // arena offsets
    float *wf_img = nullptr, *wb_img = nullptr;      // pre-split images of wf / wb (GemmDesc::b_pre)
    float *wf = nullptr, *wb = nullptr, *gp = nullptr, *cout = nullptr, *stats = nullptr, *part = nullptr;
    int amax_i = -1;                       // slot in ss_engine::amax
    int scale_i = -1;                      // slot in ss_engine::act_scale (scale of the fp16 x 2 split of this block's OUTPUT)
    bool need_dx = false;
    // input gradient w.r.t. the NETWORK input (layer-0 blocks, ss_g*_backward_inputs): wb0 holds the flipped taps [Ci][5][Co] (packed
    // when asked; the target travels in that call's Backward)
    float* wb0 = nullptr;
    bool img_ok() const { return Cp % 8 == 0 && Co % 8 == 0; }       // wf_img / wb_img are written (rows of whole image groups)
};

struct LstmDir {
    long wih, whh, bih, bhh;
};

struct LstmBlk {
    int In = 0, H = 0, L = 0;
    std::vector<LstmDir> pd;               // [L*2]
    std::vector<float*> gates, out, csave; // per layer
    float* bsum = nullptr;                 // [L][2][4H]
    bool out_img_valid = false;            // the last forward wrote out_img
    std::vector<float*> out_img;           // per layer: pre-split image of out (decoder-size blocks on the persistent kernels)
    std::vector<float*> wcat_img;          // per layer: pre-split image of wcat (decoder-size blocks only)
    std::vector<float*> wcat;              // per layer: [W_ih forward ; W_ih reverse] stacked, [8H][In] (input-gradient GEMM over both directions)
    std::vector<float*> wfrag;             // per layer: fragment-major W_hh (forward) / W_hh^T (backward), 2*4H*H floats
    // one launch per time step (persist = 0, or a batch the persistent kernels do not take):
    float* hf = nullptr;                   // ping-pong fragment-major h(t),  2 x [2][ceil16(B)][H]
    float* gf = nullptr;                   // ping-pong fragment-major da(t), 2 x [2][ceil16(B)][4H]
    float* dc = nullptr;                   // [2][B][H]
    unsigned* sync = nullptr;              // persistent kernels: group counters + abort word (one-off ops path)
    // persistent schedule: per-layer start state, contiguous so ONE memset per pass readies every layer's launch.
    //   zf = [L][LSTM_SEQ_SYNC_WORDS] ++ [L][hf]      (forward)        zb = [L][LSTM_SEQ_SYNC_WORDS] ++ [L][exchange tiles]   (backward)
    char *zf = nullptr, *zb = nullptr;
    long zf_bytes = 0, zb_bytes = 0, hf_bytes = 0, gf_bytes = 0;
    unsigned* sync_f(int l) const { return (unsigned*)zf + LSTM_SEQ_SYNC_WORDS * l; }
    unsigned* sync_b(int l) const { return (unsigned*)zb + LSTM_SEQ_SYNC_WORDS * l; }
    void* hf_l(int l) const { return zf + 4L * LSTM_SEQ_SYNC_WORDS * L + hf_bytes * l; }
    int amax0 = -1;                        // first slot in ss_engine::amax (one per layer) when the block's gradient GEMMs may use fp16 x 2
    // backward exchange tiles, one set per layer: the tagged hand-off (lstm_seq.hip) needs them zero at launch
    void* px_l(int l) const { return zb + 4L * LSTM_SEQ_SYNC_WORDS * L + gf_bytes * l; }
    float* dmid[2] = {nullptr, nullptr};   // gradient slabs of inner layer outputs [B,TP,2H]
    // Layer 0's input repeats in blocks of xf frames (decoder: every code is up-sampled by the same factor, the speaker row is constant;
    // xf = 0: not so / not used): compact input xc [B*T/xf][In], its projections xp0 [.][8H], block sums of the pre-activation gradients
    // dgs [.][8H] and the input gradient d_xc [.][In], one row per block
    int xf = 0, xcols = 0;                 // xcols: leading input columns whose gradient is needed (0: all)
    float *xc = nullptr, *xp0 = nullptr, *dgs = nullptr, *d_xc = nullptr;
    bool big() const { return H > 32; }
    // the block's recurrences run on the persistent kernels (lstm_seq.hip) at the engine's current batch
    bool persist(const ss_engine* e) const;
    // ... and its weight-gradient GEMMs are held back until its whole backward chain is through (lstm_bwd)
    bool defers_weights(const ss_engine* e) const;
    // image of the stacked W_ih of layer l (written by lstm_prep when its rows are whole image groups)
    const float* wimg(int l) const { return (!wcat_img.empty() && wcat_img[l] && in_of(l) % 8 == 0) ? wcat_img[l] : nullptr; }
    int in_of(int l) const { return l == 0 ? In : 2 * H; }
    // row stride of the out / csave / dmid slabs and of the block's output-gradient slab: 2H, padded for odd hidden sizes (kernels.h)
    long ow() const { return lstm_small_ld(H); }
};

struct Slab {   // view of a haloed slab: p points at slab row 0, first channel of interest
    float* p = nullptr;
    long ld = 0;
    const float* img = nullptr;      // the slab's pre-split image at the same position, if its producer wrote one (GemmDesc::a_pre / b_pre)
    const float* scale = nullptr;    // device word: power-of-two scale of the fp16 x 2 split of this slab's values (null: 16); conv-block outputs carry one
    Rows rows(int T) const { return Rows::slab(p, ld, T); }      // its T real frames, as the launchers of kernels.h take them
};

// What the functions of ONE backward pass (and the optimiser step behind it) tell each other.  The ABI entry point makes one on its stack
// and hands it down; a default-constructed one is the plain backward (nothing early, no input gradients), and nothing outlives the call.
struct Backward {
    // ---- asked by the entry point
    // ss_g*_backward_inputs: the layer-0 blocks whose input gradient goes, dense ([B][T] rows, row stride ld), to a caller buffer
    struct InputGrad {
        const ConvBlk* cb = nullptr;
        float* p = nullptr;
        long ld = 0;
    } in_grad[3];
    // SS_STEP_ACCUMULATE: this backward ADDS its parameter gradients to what the arena holds -- no arena memset, the conv weight gradients
    // unpacked with += (every other producer adds already)
    bool accumulate = false;
    const InputGrad* input_grad_of(const ConvBlk& cb) const {
        for (const InputGrad& t : in_grad)
            if (t.cb == &cb && t.p) return &t;
        return nullptr;
    }
    // Early Adam (one GPU, Adam inside the step): the decoder + head range of the arenas (80 % of the bytes) is updated on the side stream
    // right behind its last weight-gradient GEMM, beside the encoder backward (GEMM-bound, HBM mostly idle), instead of at the step's end
    bool adam_early = false;               // the fused train steps want it
    float adam_gs = 1.0f;
    // ---- recorded by the pass
    bool dec_w_pending = false;            // backward_decoder(late): the decoder's + head's weight gradients are still to be enqueued (backward_encoder)
    long adam_early_from = -1;             // >= 0: the range [adam_early_from, arena) has been enqueued, the step state prepared
    long clip_early_from = -1;             // >= 0: the squares' partial sums of [clip_early_from, status_off) have been enqueued (side stream)
    WgradTable wg{};                       // encoder-BLSTM weight gradients waiting for their fused launch (lstm_wgrad.hip): lstm_weight_grads appends, wgrad_flush launches
    bool wg_defer = false;                 // backward_encoder collects every small block's layers and flushes once at the end
    ConvUnpackTable unpack{};              // conv weight gradients waiting for their re-layout (conv_block_bwd)
    bool unpack_later = false;
};

// what the fused training step adds to its forward
struct FusedForward {
    const float *late_org = nullptr, *late_emb = nullptr;   // x_org / emb still to be copied in (done on the Encoder_t branch)
    bool prezero = false;                  // zero the gradient arena (and the backward recurrences' start state) on a branch stream meanwhile
    bool keep_grads = false;               // ... except the arena itself (SS_STEP_ACCUMULATE): the per-backward state is still readied there
};

// how one lstm_weight_grads call differs from the plain one
struct DwRoute {
    int part = 0;                          // 0 everything; 2 everything except the W_ih gradient (it went out through lstm_wih_gemm_queued)
    bool queue = false;                    // image GEMMs in the work-queue form
    hipStream_t over_ih = nullptr, over_hh = nullptr;   // unbatched decoder path: the reverse direction's dW_ih / dW_hh go to these streams (tail split)
};

}  // namespace

struct ss_engine {
    int kind;
    ss_hparams hp;
    int maxB, maxT;
    int bound_max_len_pad = 0;             // hp.max_len_pad as given to ss_create: what a step WITHOUT SS_STEP_BUCKET runs with
    int precision = SS_PRECISION_F32;
    std::vector<ParamInfo> params;
    long arena = 0;                        // floats per arena, INCLUDING the 4-float status slot at the end
    long status_off = 0;                   // gradient arena: G[status_off] = 1 when this rank's step is invalid; the data-parallel
                                           // all-reduce sums it, so every rank's Adam kernel sees a non-zero value and skips
    void* comm = nullptr;                  // ncclComm_t of ss_comm_init (RCCL, dlopen'd)
    int comm_rank = 0, comm_world = 1;
    // data-parallel step in flight: gradient ranges are all-reduced on comm_s as soon as their producers are through (dp_bucket).
    // One step long, but kept on the engine: dp_done / dp_rec below are filled under it by the schedule functions (dp_bucket) and read
    // after the step's backward (dp_finish, ss_dp_profile_read)
    bool dp_on = false;
    hipStream_t comm_s = nullptr;
    hipEvent_t ev_comm = nullptr;
    std::vector<std::pair<long, long>> dp_done;      // [offset, end) ranges already handed to a collective in this step
    // ss_dp_profile: hipEvent brackets round every collective of the LAST data-parallel step on the communication stream, plus one event at
    // the backward's end on the main stream -- where each bucket's all-reduce starts and ends relative to it (the overlap a scaling run achieved)
    bool dp_prof = false;
    struct DpRec {
        long off, count;
        hipEvent_t a, b;
    };
    std::vector<DpRec> dp_rec;             // this step's
    std::vector<hipEvent_t> dp_ev_pool;    // events are created once and reused
    int dp_ev_used = 0;
    hipEvent_t dp_bwd_end = nullptr;
    bool lockstep = false;                 // data-parallel member: entry points never refuse on the status word (entry_check)
    unsigned* sticky = nullptr;            // engine status word in host-coherent pinned memory (kernels.h SS_STICKY_*): written by
                                           // kernels, read by the host without synchronising; cleared only by ss_clear_abort

    float *P = nullptr, *G = nullptr, *Mm = nullptr, *Vv = nullptr;
    long accum_count = 0;                  // backward passes summed into G since it was last cleared (ss_grad_accum_count; host-side)
    bool bwd_accumulate = false;           // the backward in flight adds to the arena: chosen where it starts (backward_decoder), read by
                                           // ss_train_finish for the second half of a SS_STEP_SPLIT_BACKWARD step
    char* ws = nullptr;
    long ws_bytes = 0;
    int curB = 0, curT = 0;
    int cur_img16 = -1;                    // img16() when geometry() last zeroed the plan: the byte layout the zero halo rows of the images hold for
    // ---- what a forward leaves for its backward (possibly a later ABI call): set by forward_core, cleared as a whole wherever the
    // geometry or the workspace changes
    struct FwdState {
        bool have = false;                 // there is a forward to differentiate
        bool training = false;
        int enc_plan0 = 0;                 // plan[] index of the first encoder InterpLnr call
        bool xf_img_valid = false;         // its gathers wrote xf_img
        bool grads_zeroed = false;         // fused training step: the gradient arena was zeroed on a branch stream during the forward
        bool bwd_sync_zeroed = false;      // the same for the backward recurrences' sync words / exchange tiles and the work-queue words
        bool ragged = false;               // it ran over per-row lengths (ss_*_forward_ragged): eval-only, no backward exists for it
        bool decode = false;               // it was ss_*_decode_train: the decoder alone on caller codes, only ss_*_decode_backward may follow
    } fwd;
    // ---- bookkeeping of the backward in flight: written by the decoder's lstm_bwd, read later in the same backward (and by
    // speaker_input_grad behind it); backward_decoder starts it from zero
    struct BwdMarks {
        int dec_ih_done = 0;               // bit l: decoder layer l's W_ih gradient went out beside a recurrence (lstm_late_weights skips it)
        int dec_w_done = 0;                // bit l: ALL of decoder layer l's weight gradients went out beside a recurrence (early_dw)
        int dg16_written = 0;              // 16-bit data path: bit l = decoder layer l's backward recurrence wrote dg_img[l] (plain bf16)
        int dg32_skipped = 0;              // ... and NOT the fp32 slab: gates[l] still holds the forward's activated gates (gemm_on refuses to read it)
        int wq_next = 0;                   // work-queue launches handed out of wq_pool
    } bwd;
    // XCD-aware weight gradients (lstm_bwd, ss_tune("xcd_dw")): where the decoder's persistent backward recurrences leave XCDs free
    // (B <= 48: 2 * ceil(B / 16) groups, one XCD each), the W_ih gradient of layer l + 1 runs as a work-queue image GEMM BESIDE the
    // recurrence of layer l -- on the free XCDs, because its 128-144 KB workgroups cannot be dispatched to a CU a recurrence workgroup holds
    unsigned* wq_pool = nullptr;           // zeroed per backward pass: 4 words per work-queue launch
    static constexpr int WQ_SLOTS = 16;
    // column sums (bias gradients): float64 chunk partials from the step's scratch (part) + a ring of arrival counters, zero at rest
    unsigned* colsum_ctr = nullptr;
    static constexpr int COLSUM_CTRS = 2048;
    int colsum_next = 0;
    // Clipping by global norm (ss_set_grad_clip): the norm needs the whole arena before the first element is updated, so a fused step's
    // early range (Backward) sends the PARTIAL SUMS of its squares to the side stream instead of its update; adam_enqueue adds the encoder
    // range's, finalises (norm, coefficient, skip) and updates the arena in one launch.  Partials: [0, wgs(split)) encoder range, then the
    // decoder + head range.
    float clip_max = 0.0f;                 // 0 off, > 0 clip to this norm, +inf measure and refuse non-finite gradients only
    ClipState* clip = nullptr;             // workspace byte 128, beside the Adam state
    double* clip_part = nullptr;
    GradSegTable segs{};                   // runs of parameter elements of the arena (build_table)
    bool segs_ok = false;
    // Decoupled weight decay and the parameter average (ss_set_weight_decay / ss_set_ema; kernels.h, OptExtState).  Host side: which form
    // of the update every route enqueues (opt_ext); device side: the factors and the update counter, set by the step's one prepare.
    float wd = 0.0f;                       // 0 off
    int wd_which = 0;                      // 0 every element, 1 tensors with ndim >= 2 only (wd_runs)
    float* ema = nullptr;                  // the caller's average arena; NULL off
    OptExtState* ext = nullptr;            // workspace byte 144, beside the Adam and clip states
    WdRunTable wd_runs{};                  // runs of [0, arena) by "decayed under which = 1" (build_table)
    bool wd_runs_ok = false;
    // Learning-rate schedule (ss_set_lr_schedule; kernels.h, LrSchedState).  Host side: whether the prepare kernels get the state's address
    // (lr_sched); device side: the options and the stats words of the last applied step.
    int lr_kind = 0;                       // LR_OFF
    LrSchedState* sch = nullptr;           // workspace byte 192, beside the Adam, clip and weight-decay / EMA states

    // components
    ConvBlk c1[3], c2[3], ct;              // Encoder_7 stream 1 / stream 2 (or Encoder_6 in c2), Encoder_t
    LstmBlk l1, l2, lt, ld;                // lstm_1, lstm_2 (or Encoder_6.lstm), Encoder_t.lstm, decoder.lstm
    long head_w = 0, head_b = 0;
    int head_out = 0, dec_in_dim = 0, CE = 0;   // CE = channels of the fused encoder slab (768 for G3, 256 for G6)

    // workspace slabs
    float *in_mel = nullptr, *in_f0 = nullptr, *org = nullptr, *emb = nullptr;
    int f0p = 0;                           // padded one-hot width (264)
    float *act = nullptr, *d_act = nullptr, *d_xf = nullptr, *xf[3] = {nullptr, nullptr, nullptr};
    float* xf_img[3] = {nullptr, nullptr, nullptr};     // pre-split images of xf[0], xf[1] (training forward only: written by the gathers)
    float *act_t = nullptr, *d_act_t = nullptr;
    float *dec_in = nullptr, *d_dec_in = nullptr, *d_top = nullptr;
    float *d_o1 = nullptr, *d_o2 = nullptr, *d_ot = nullptr;
    float *out_slab = nullptr, *d_out_slab = nullptr;
    float* gp_all = nullptr;               // packed conv weight-gradient images (all blocks)
    // gradient slabs as images for the image GEMM: written by split_image with the measured scale (gscale[i] beside amax[i])
    float* dg_img[3] = {nullptr, nullptr, nullptr};       // decoder layers' pre-activation gradients [B, TP, 8H]
    float *d_act_l[2] = {nullptr, nullptr}, *d_img_l[2] = {nullptr, nullptr};      // conv-output gradients of trunk layers 1 and 2 when their weight gradients run off the chain (conv_dw_off)
    float *d_img = nullptr, *d_img_t = nullptr;           // conv-output gradients of the trunk [B, TP, CE] / Encoder_t [B, TP, dim_enc_2]
    float* gscale = nullptr;               // [16]
    float* act_scale = nullptr;            // [8] per conv block: scale of its output's fp16 x 2 split (act_scales, from the GroupNorm affine)
    void* zeros = nullptr;                 // 1 KB of zero bytes (image GEMM: reduction rows past K)
    float* part = nullptr;                 // split-K partial slabs of the image GEMM: a bump allocator over part_cap floats, reset per step
    long part_cap = 0, part_off = 0;
    long scratch_fallbacks = 0;            // launches that found the step's scratch exhausted and took the slower path (ss_scratch_fallbacks): 0 in a healthy run
    float* amax = nullptr;                 // [16] max |gradient| of the slabs the fp16 x 2 gradient GEMMs read: decoder layers 0..2, then the 7 convs
    long gp_bytes = 0;
    float *loss_part = nullptr;
    int* qidx = nullptr;
    InterpPlan plan[4];
    AdamState* adam = nullptr;
    std::map<std::string, std::pair<float*, long>> dbg;   // name -> (ptr, cols)
    // weight-gradient GEMMs of a BLSTM layer run on this side stream while the next layer's recurrence (latency-bound,
    // one launch per time step) proceeds on the caller's stream
    std::string stream_report;            // what pick_streams found (ss_stream_report)
    hipStream_t main_s = nullptr;         // the stream the step's dependency chain runs on (see g_own_streams)
    hipStream_t side = nullptr;
    hipStream_t side2 = nullptr;          // independent branches (per-step weight re-layouts, Encoder_t, second encoder BLSTM)
    hipStream_t side3 = nullptr;          // third independent branch of the encoder backward (Encoder_t)
    hipEvent_t ev_io[2] = {};             // caller stream <-> engine main stream ordering (own_streams)
    hipEvent_t ev_join[4] = {};           // events recorded early: [0] lstm_2 branch's input gradient, [1] decoder chain done, [2] dec_in_grad done, [3] lstm_1 chain done
    hipEvent_t ev_dec[2] = {};            // split step without join: decoder chain done (caller stream) / its weight gradients done (side)
    int dec_pending = 0;                  // 0 none, 1 ev_dec[0] only, 2 both
    hipEvent_t ev[16] = {};
    int ev_next = 0;
    bool side_used = false;
    // ss_profile: hipEvent pairs around the launches of the dominant kernel (decoder input-projection GEMM, layers >= 1)
    // on the stream they are launched on, so a benchmark can report that kernel's duration inside its own timed region
    static constexpr int PROF_CAP = 8192;
    struct ProfRec {
        int klass;
        double flops;
        int stream;                       // 0 caller / main, 1 side, 2 second branch, 3 third branch, -1 other
    };
    std::vector<hipEvent_t> prof_ev;      // 2 per record, created on demand
    std::vector<ProfRec> prof_rec;
    int prof_n = 0;
    unsigned prof_mask = 0;               // bit k set: launches of class k are bracketed
    int prof_every = 1, prof_ctr = 0;     // ss_profile_sample: brackets only in every prof_every-th training step
    bool prof_live = true;                // this step is one of them

    // 16-bit data path: the operand images are plain bf16 tensors (2 bytes per element) instead of format-v2 images (4)
    bool img16() const { return precision == SS_PRECISION_BF16 && g_bf16_img; }
    // image pointer `elems` ELEMENTS behind `base` (an image has its tensor's geometry; the bytes per element depend on the format)
    float* ioff(float* base, long elems) const { return img16() ? (float*)((char*)base + 2 * elems) : base + elems; }
    const float* ioff(const float* base, long elems) const { return img16() ? (const float*)((const char*)base + 2 * elems) : base + elems; }
};

namespace {

bool LstmBlk::persist(const ss_engine* e) const { return big() && g_persist && lstm_seq_supported(e->curB, H); }
bool LstmBlk::defers_weights(const ss_engine* e) const { return persist(e) && e->side && g_overlap && g_defer_dw; }

// every conv block, in the order the workspace plan lays them out (carve: packed gradient images, amax / act_scale slots)
template <class E>
auto conv_blocks(E& e) -> std::array<decltype(&e.ct), 7> {
    return {&e.c1[0], &e.c1[1], &e.c1[2], &e.c2[0], &e.c2[1], &e.c2[2], &e.ct};
}

// ---- named views of the workspace slabs: every pass builds its operands from these
// Encoder_t's conv block output, the input of its BLSTM
Slab enc_t_out(const ss_engine* e) { return {e->act_t, e->hp.dim_enc_2, nullptr, e->act_scale + e->ct.scale_i}; }
// input of trunk chain c (1: content, 2: pitch) at layer i: the network input (i = 0) or layer i - 1's output in the fused slab (i = 3: what
// the chain's BLSTM reads), with the scale word of the block that wrote it; img (nullable): the fused slab's pre-split image
Slab trunk_in(const ss_engine* e, int c, int i, const float* img = nullptr) {
    if (i == 0) return c == 1 ? Slab{e->in_mel, e->hp.dim_freq} : Slab{e->in_f0, e->f0p};
    const int off = (c == 2 && e->kind == SS_GENERATOR_3) ? e->hp.dim_enc : 0;       // first channel of the pitch stream inside the fused slab
    return {e->xf[i - 1] + off, e->CE, img ? e->ioff(img, off) : nullptr, e->act_scale + (c == 1 ? e->c1 : e->c2)[i - 1].scale_i};
}
// the decoder's layer 0 runs on the compact (one row per block of repeated frames) form of its input
bool dec_compact(const ss_engine* e) { return g_compact0 && e->ld.xf > 0 && e->ld.persist(e); }
// the decoder's input and input-gradient slabs in the form its layer 0 runs on
Slab dec_x(const ss_engine* e) { return dec_compact(e) ? Slab{e->ld.xc, e->dec_in_dim} : Slab{e->dec_in, e->dec_in_dim}; }
Slab dec_dx(const ss_engine* e) { return dec_compact(e) ? Slab{e->ld.d_xc, e->dec_in_dim} : Slab{e->d_dec_in, e->dec_in_dim}; }
// the code streams that make up the decoder input, in column order (model.py:301-309 / 341-347); returns how many
int code_srcs(const ss_engine* e, CodeSrc src[3]) {
    const ss_hparams& h = e->hp;
    int n = 0, col = 0;
    auto add = [&](const LstmBlk& lb, int l, float* d_o, int H, int freq) { src[n++] = {lb.out[l], d_o, H, freq, col, (int)lb.ow()}; col += 2 * H; };
    if (e->kind == SS_GENERATOR_3) add(e->l1, 1, e->d_o1, h.dim_neck, h.freq);
    add(e->lt, 0, e->d_ot, h.dim_neck_2, h.freq_2);
    add(e->l2, 0, e->d_o2, h.dim_neck_3, h.freq_3);
    return n;
}

long align4(long x) { return (x + 3) & ~3L; }

// ------------------------------------------------------------------------------------------------ parameter table
struct TableBuilder {
    std::vector<ParamInfo>& v;
    long off = 0;
    long add(const std::string& name, long a, long b = -1, long c = -1) {
        ParamInfo p;
        p.name = name;
        p.offset = off;
        p.ndim = b < 0 ? 1 : (c < 0 ? 2 : 3);
        p.shape[0] = a;
        p.shape[1] = b < 0 ? 1 : b;
        p.shape[2] = c < 0 ? 1 : c;
        v.push_back(p);
        off = align4(off + p.numel());
        return p.offset;
    }
    void conv(const std::string& pre, int ci, int co, ConvBlk& cb) {
        cb.Ci = ci;
        cb.Co = co;
        cb.Cp = (int)align4(ci);
        cb.w = add(pre + ".0.conv.weight", co, ci, 5);
        cb.b = add(pre + ".0.conv.bias", co);
        cb.ga = add(pre + ".1.weight", co);
        cb.be = add(pre + ".1.bias", co);
    }
    void lstm(const std::string& pre, int in, int hid, int layers, LstmBlk& lb) {
        lb.In = in;
        lb.H = hid;
        lb.L = layers;
        lb.pd.clear();
        for (std::vector<float*>* v : {&lb.gates, &lb.out, &lb.csave, &lb.out_img, &lb.wcat_img, &lb.wcat, &lb.wfrag}) v->assign(layers, nullptr);      // filled by carve
        for (int l = 0; l < layers; ++l) {
            const int i = l == 0 ? in : 2 * hid;
            for (int d = 0; d < 2; ++d) {
                const std::string sfx = "_l" + std::to_string(l) + (d ? "_reverse" : "");
                LstmDir pd;
                pd.wih = add(pre + ".weight_ih" + sfx, 4 * hid, i);
                pd.whh = add(pre + ".weight_hh" + sfx, 4 * hid, hid);
                pd.bih = add(pre + ".bias_ih" + sfx, 4 * hid);
                pd.bhh = add(pre + ".bias_hh" + sfx, 4 * hid);
                lb.pd.push_back(pd);
            }
        }
    }
};

void build_table(ss_engine* e) {
    const ss_hparams& h = e->hp;
    TableBuilder tb{e->params};
    if (e->kind == SS_INTERP_ONLY) {
        e->arena = 0;
        return;
    }
    if (e->kind == SS_GENERATOR_3) {      // registration order of model.py:161-191, 59-71, 244-247, 288-290
        for (int i = 0; i < 3; ++i)
            tb.conv("encoder_1.convolutions_1." + std::to_string(i), i == 0 ? h.dim_freq : h.dim_enc, h.dim_enc, e->c1[i]);
        tb.lstm("encoder_1.lstm_1", h.dim_enc, h.dim_neck, 2, e->l1);
        for (int i = 0; i < 3; ++i)
            tb.conv("encoder_1.convolutions_2." + std::to_string(i), i == 0 ? h.dim_f0 : h.dim_enc_3, h.dim_enc_3, e->c2[i]);
        tb.lstm("encoder_1.lstm_2", h.dim_enc_3, h.dim_neck_3, 1, e->l2);
        tb.conv("encoder_2.convolutions.0", h.dim_freq, h.dim_enc_2, e->ct);
        tb.lstm("encoder_2.lstm", h.dim_enc_2, h.dim_neck_2, 1, e->lt);
        e->dec_in_dim = 2 * h.dim_neck + 2 * h.dim_neck_2 + 2 * h.dim_neck_3 + h.dim_spk_emb;
        tb.lstm("decoder.lstm", e->dec_in_dim, 512, 3, e->ld);
        e->head_out = h.dim_freq;
        e->head_w = tb.add("decoder.linear_projection.linear_layer.weight", h.dim_freq, 1024);
        e->head_b = tb.add("decoder.linear_projection.linear_layer.bias", h.dim_freq);
        e->CE = h.dim_enc + h.dim_enc_3;
    } else {                              // model.py:330-332, 107-119, 268-271
        tb.conv("encoder_2.convolutions.0", h.dim_freq, h.dim_enc_2, e->ct);
        tb.lstm("encoder_2.lstm", h.dim_enc_2, h.dim_neck_2, 1, e->lt);
        for (int i = 0; i < 3; ++i)
            tb.conv("encoder_3.convolutions." + std::to_string(i), i == 0 ? h.dim_f0 : h.dim_enc_3, h.dim_enc_3, e->c2[i]);
        tb.lstm("encoder_3.lstm", h.dim_enc_3, h.dim_neck_3, 1, e->l2);
        e->dec_in_dim = 2 * h.dim_neck_2 + 2 * h.dim_neck_3;
        tb.lstm("decoder.lstm", e->dec_in_dim, 256, 2, e->ld);
        e->head_out = h.dim_f0;
        e->head_w = tb.add("decoder.linear_projection.linear_layer.weight", h.dim_f0, 512);
        e->head_b = tb.add("decoder.linear_projection.linear_layer.bias", h.dim_f0);
        e->CE = h.dim_enc_3;
    }
    e->ld.amax0 = 0;                      // decoder layers: slots 0..2 of ss_engine::amax (the convs follow from 3)
    e->status_off = align4(tb.off);
    e->arena = e->status_off + 4;
    // runs of parameter elements (grad_sumsq): tensors that follow each other without an alignment gap merge into one run
    e->segs.n = 0;
    e->segs_ok = true;
    for (const ParamInfo& p : e->params) {
        GradSegTable& g = e->segs;
        if (g.n && g.start[g.n - 1] + g.len[g.n - 1] == p.offset && (long)g.len[g.n - 1] + p.numel() < (1L << 31)) {
            g.len[g.n - 1] += (int)p.numel();
        } else if (g.n < GRAD_SEG_MAX && p.numel() < (1L << 31)) {
            g.start[g.n] = p.offset;
            g.len[g.n++] = (int)p.numel();
        } else {
            e->segs_ok = false;
        }
    }
    // runs by "decayed under ss_set_weight_decay(which = 1)": a tensor's run reaches to the next tensor (its alignment gap included), tensors
    // of the same class that follow each other merge, the status slot closes the table -- [0, arena) without a hole
    e->wd_runs.n = 0;
    e->wd_runs_ok = true;
    for (size_t i = 0; i <= e->params.size(); ++i) {
        WdRunTable& w = e->wd_runs;
        const bool slot = i == e->params.size();
        const long start = slot ? e->status_off : e->params[i].offset;
        const long end = slot ? e->arena : (i + 1 < e->params.size() ? e->params[i + 1].offset : e->status_off);
        const int dec = !slot && e->params[i].ndim >= 2;
        if (start % 4 || end % 4 || end < start || end - start >= (1L << 31)) {
            e->wd_runs_ok = false;
        } else if (w.n && w.decayed[w.n - 1] == dec && w.start[w.n - 1] + w.len[w.n - 1] == start && w.len[w.n - 1] + (end - start) < (1L << 31)) {
            w.len[w.n - 1] += (int)(end - start);
        } else if (w.n < WD_RUN_MAX) {
            w.start[w.n] = start;
            w.len[w.n] = (int)(end - start);
            w.decayed[w.n++] = dec;
        } else {
            e->wd_runs_ok = false;
        }
    }
    e->f0p = (int)((h.dim_f0 + 7) & ~7);      // a multiple of 8: the packed conv weights of convolutions_2[0] then have rows of whole image groups
    for (int i = 0; i < 3; ++i) {
        e->c1[i].need_dx = i > 0;
        e->c2[i].need_dx = i > 0;
    }
    e->ct.need_dx = false;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ workspace plan
namespace {

// The plan of geometry (B, T): every slab in a fixed order, 256-byte aligned; returns its size in bytes.  On an engine it places the
// slabs in e.ws and records every pointer and size; on a CONST engine it is the dry run, which only adds up and cannot write.
template <class E>
long carve(E& e, int B, int T) {
    constexpr bool assign = !std::is_const_v<E>;
    const ss_hparams& hp = e.hp;
    const long TP = T + 2 * HALO;
    const long R = (long)B * TP;
    long off = 0;
    if constexpr (assign) e.dbg.clear();
    auto take = [&](long bytes) -> char* {
        char* p = assign ? e.ws + off : nullptr;
        off += (bytes + 255) & ~255L;
        return p;
    };
    auto put = [&](auto& dst, long bytes) {
        char* p = take(bytes);
        if constexpr (assign) dst = (std::remove_reference_t<decltype(dst)>)p;
    };
    auto slab = [&](auto& dst, const char* name, long cols) {
        put(dst, R * cols * 4);
        if constexpr (assign)
            if (name) e.dbg[name] = {dst, cols};
    };
    auto conv_ws = [&](auto& cb, const std::string& name) {
        if (cb.Co == 0) return;
        put(cb.wf, (long)cb.Co * 5 * cb.Cp * 4);
        if (cb.need_dx) put(cb.wb, (long)cb.Ci * 5 * cb.Co * 4);
        put(cb.wf_img, (long)cb.Co * 5 * cb.Cp * 4);
        if (cb.need_dx) put(cb.wb_img, (long)cb.Ci * 5 * cb.Co * 4);
        slab(cb.cout, (name + ".conv").c_str(), cb.Co);
        put(cb.stats, (long)B * (cb.Co / 16) * 2 * 4);
        put(cb.part, (long)B * 3 * cb.Co * 4);          // deterministic mode: per-utterance affine / bias gradient sums
    };
    auto lstm_ws = [&](auto& lb, const std::string& name) {      // (the per-layer vectors have their L entries since build_table)
        if (lb.L == 0) return;
        for (int l = 0; l < lb.L; ++l) {
            slab(lb.gates[l], (name + ".gates" + std::to_string(l)).c_str(), 8L * lb.H);
            slab(lb.out[l], (name + ".out" + std::to_string(l)).c_str(), lb.ow());
            slab(lb.csave[l], (name + ".c" + std::to_string(l)).c_str(), lb.ow());
        }
        if (lb.big())
            for (int l = 0; l < lb.L; ++l) slab(lb.out_img[l], nullptr, 2L * lb.H);       // halo rows stay zero like those of out
        put(lb.bsum, (long)lb.L * 2 * 4 * lb.H * 4);
        for (int l = 0; l < lb.L; ++l) put(lb.wcat[l], 8L * lb.H * lb.in_of(l) * 4);
        if (lb.big())
            for (int l = 0; l < lb.L; ++l) put(lb.wcat_img[l], 8L * lb.H * lb.in_of(l) * 4);
        if (lb.big()) {
            const long B16 = ((B + 15) / 16) * 16;
            for (int l = 0; l < lb.L; ++l) put(lb.wfrag[l], 2L * lb.H * 4 * lb.H * 4);
            put(lb.hf, 2L * 2 * B16 * lb.H * 4);
            put(lb.gf, 2L * 2 * B16 * 4 * lb.H * 4);
            put(lb.dc, 2L * B * lb.H * 4);
            put(lb.sync, LSTM_SEQ_SYNC_WORDS * 4);
            const long hf_bytes = lstm_seq_xbytes(B, lb.H, false);       // exchange buffers of the persistent kernels
            const long gf_bytes = lstm_seq_xbytes(B, lb.H, true);
            const long zf_bytes = lb.L * (4L * LSTM_SEQ_SYNC_WORDS + hf_bytes);
            const long zb_bytes = lb.L * (4L * LSTM_SEQ_SYNC_WORDS + gf_bytes);
            put(lb.zf, zf_bytes);
            put(lb.zb, zb_bytes);
            if constexpr (assign) {
                lb.hf_bytes = hf_bytes;
                lb.gf_bytes = gf_bytes;
                lb.zf_bytes = zf_bytes;
                lb.zb_bytes = zb_bytes;
            }
        }
        if (lb.L > 1) {
            slab(lb.dmid[0], (name + ".dmid0").c_str(), lb.ow());
            slab(lb.dmid[1], (name + ".dmid1").c_str(), lb.ow());
        }
    };
    auto interp_ws = [&](auto& pl, bool storage) {
        if constexpr (assign) {
            pl.S = hp.max_len_seq / hp.min_len_seg + 1;     // model.py:365
            pl.ncand = 2 * hp.max_len_seg;                  // model.py:389
            pl.P = hp.max_len_pad;
            pl.T = T;
        }
        if (!storage) return;
        put(pl.i0, (long)B * hp.max_len_pad * 4);
        put(pl.lam, (long)B * hp.max_len_pad * 4);
        put(pl.nrows, (long)B * 4);
        put(pl.counts, (long)B * 4);
        put(pl.start, (long)B * (T + 1) * 4);
    };
    put(e.adam, sizeof(AdamState));                    // first: survives geometry changes (offset 0)
    if constexpr (assign) e.clip = (ClipState*)((char*)e.adam + CLIP_STATE_BYTE);      // same 256 bytes
    if constexpr (assign) e.ext = (OptExtState*)((char*)e.adam + OPT_EXT_STATE_BYTE);
    if constexpr (assign) e.sch = (LrSchedState*)((char*)e.adam + LR_SCHED_STATE_BYTE);
    if (e.kind != SS_INTERP_ONLY) put(e.clip_part, 2L * GRAD_SUMSQ_MAX_WGS * sizeof(double));     // scratch, geometry-independent (offset 256)
    if (e.kind == SS_INTERP_ONLY) {                    // a bare InterpLnr module only needs one plan
        for (int i = 0; i < 4; ++i) interp_ws(e.plan[i], i == 3);
        return off;
    }
    slab(e.in_mel, "in.mel", hp.dim_freq);
    slab(e.in_f0, "in.f0", e.f0p);
    slab(e.org, "in.org", hp.dim_freq);
    put(e.emb, (long)B * hp.dim_spk_emb * 4);
    for (int i = 0; i < 3; ++i) {
        conv_ws(e.c1[i], "enc1.c1_" + std::to_string(i));
        conv_ws(e.c2[i], (e.kind == SS_GENERATOR_3 ? "enc1.c2_" : "enc3.c_") + std::to_string(i));
        slab(e.xf[i], ("enc.xf" + std::to_string(i)).c_str(), e.CE);
        if (i < 2) slab(e.xf_img[i], nullptr, e.CE);           // pre-split images of the resampled activations the next layer's convs read
    }
    slab(e.act, "enc.act", e.CE);
    slab(e.d_act, "enc.d_act", e.CE);
    slab(e.d_img, nullptr, e.CE);
    for (int i = 0; i < 2; ++i) {
        slab(e.d_act_l[i], nullptr, e.CE);
        slab(e.d_img_l[i], nullptr, e.CE);
    }
    slab(e.d_img_t, nullptr, hp.dim_enc_2);
    put(e.gscale, 16 * 4);
    put(e.act_scale, 8 * 4);
    put(e.zeros, 1024);
    slab(e.d_xf, "enc.d_xf", e.CE);
    conv_ws(e.ct, "enc2.c");
    {   // packed weight-gradient images of every conv, contiguous so one memset per backward zeroes them all
        long tot = 0;
        for (auto* cb : conv_blocks(e)) tot += align4((long)cb->Co * 5 * cb->Cp);
        put(e.gp_all, tot * 4);
        put(e.amax, 16 * 4);
        if constexpr (assign) {
            e.gp_bytes = tot * 4;
            float* p = e.gp_all;
            int slot = 3;
            for (ConvBlk* cb : conv_blocks(e)) {
                cb->gp = cb->Co ? p : nullptr;
                cb->scale_i = slot - 3;
                cb->amax_i = slot++;
                p += align4((long)cb->Co * 5 * cb->Cp);
            }
        }
    }
    slab(e.act_t, "enc2.act", hp.dim_enc_2);
    slab(e.d_act_t, "enc2.d_act", hp.dim_enc_2);
    lstm_ws(e.l1, "enc1.lstm1");
    lstm_ws(e.l2, e.kind == SS_GENERATOR_3 ? "enc1.lstm2" : "enc3.lstm");
    lstm_ws(e.lt, "enc2.lstm");
    lstm_ws(e.ld, "dec.lstm");
    if (e.ld.big())
        for (int l = 0; l < e.ld.L && l < 3; ++l) slab(e.dg_img[l], nullptr, 8L * e.ld.H);
    if (e.l1.L) slab(e.d_o1, "enc1.d_o1", e.l1.ow());
    slab(e.d_o2, "enc.d_o2", e.l2.ow());
    slab(e.d_ot, "enc2.d_ot", e.lt.ow());
    slab(e.dec_in, "dec.in", e.dec_in_dim);
    slab(e.d_dec_in, "dec.d_in", e.dec_in_dim);
    {
        const int F = hp.freq_2;
        const bool same = hp.freq_3 == F && (e.kind != SS_GENERATOR_3 || hp.freq == F);
        const int xf = (same && F > 1 && T % F == 0 && e.ld.big()) ? F : 0;       // structurally possible; ss_tune("compact0") decides per step
        if constexpr (assign) {
            e.ld.xf = xf;
            e.ld.xcols = e.kind == SS_GENERATOR_3 ? e.dec_in_dim - hp.dim_spk_emb : 0;
        }
        if (xf) {
            const long R8 = (long)B * (T / F);
            put(e.ld.xc, R8 * e.dec_in_dim * 4);
            put(e.ld.xp0, R8 * 8 * e.ld.H * 4);
            put(e.ld.dgs, R8 * 8 * e.ld.H * 4);
            put(e.ld.d_xc, R8 * e.dec_in_dim * 4);
        }
    }
    slab(e.d_top, "dec.d_top", 2L * e.ld.H);
    slab(e.out_slab, "out", e.head_out);
    slab(e.d_out_slab, "d_out", e.head_out);
    put(e.loss_part, ((long)B * T + 8L * B) * 4);
    put(e.qidx, (long)B * TP * 4);
    put(e.wq_pool, ss_engine::WQ_SLOTS * 16);
    put(e.colsum_ctr, ss_engine::COLSUM_CTRS * 4);
    for (int i = 0; i < 4; ++i) interp_ws(e.plan[i], true);
    // flipped taps of the layer-0 blocks' input-gradient GEMMs (ss_g*_backward_inputs only): last in the plan, so every slab above
    // keeps its place.  Three blocks may run at once on different streams, hence one each (2.3 MB for Generator_3).
    for (auto* cb : {&e.c1[0], &e.c2[0], &e.ct})
        if (cb->Co) put(cb->wb0, (long)cb->Ci * 5 * cb->Co * 4);
    return off;
}

}  // namespace

namespace {

// eval: the call is an eval-mode forward (ss_g3_forward / ss_g6_forward with training == 0, ss_g3_rhythm).  Those may run T beyond
// max_frames, up to SS_MAX_EVAL_FRAMES, whenever the plan for (B, T) fits the bound workspace; everything that trains or differentiates
// keeps T <= max_frames (<= 256: the register-resident GroupNorm backward and the fused gathers).
int geometry(ss_engine* e, int B, int T, hipStream_t s, bool eval = false) {
    if (!e->ws) return fail("engine is not bound (call ss_bind first)");
    if (B < 1 || B > e->maxB || T < 1) return fail("batch / frames outside the limits given to ss_create");
    if (T > e->maxT && (!eval || e->kind == SS_INTERP_ONLY))
        return fail("batch / frames outside the limits given to ss_create: frames above max_frames run in eval-mode forwards only "
                    "(training, backward and InterpLnr keep T <= max_frames <= 256)");
    if (T > SS_MAX_EVAL_FRAMES) return fail("eval-mode forward: T above SS_MAX_EVAL_FRAMES (8192)");
    if (e->kind != SS_INTERP_ONLY && (T % e->hp.freq || T % e->hp.freq_2 || T % e->hp.freq_3))
        return fail("T must be a multiple of the code down-sampling factors (model.py:87,223-227)");
    // The plan is what was zeroed: the shape AND the image format.  The 16-bit data path reads the image buffers as plain bf16 tensors at
    // half the byte offsets (ioff), so after a switch of ss_set_precision / ss_tune("bf16_img") the byte ranges that are halo rows in the
    // new layout hold pieces of real rows written in the old one -- and no producer of an image ever writes a halo row.
    const int img16 = e->img16() ? 1 : 0;
    if (B == e->curB && T == e->curT && img16 == e->cur_img16) return 0;
    const long need = carve(std::as_const(*e), B, T);
    if (need > e->ws_bytes) return fail("workspace too small for this batch / frames: grow it to ss_plan_bytes(B, T) with ss_set_workspace");
    // new geometry or image format: halo rows move, so everything the new plan uses, except the Adam state (first 256 bytes), is re-zeroed
    // (0.1 - 0.2 ms per switch at batch 64: the price of a length-bucket change, SS_STEP_BUCKET, or of a precision switch)
    HIPCHK(hipMemsetAsync(e->ws + 256, 0, need - 256, s));
    carve(*e, B, T);
    e->curB = B;
    e->curT = T;
    e->cur_img16 = img16;
    e->fwd = {};
    return 0;
}

constexpr int DW_WGS = 384;       // workgroups a split-K weight-gradient launch aims at (round 2: 384 = 1.5 per CU measured best in the step, 5.38 vs 5.48 ms at 512; 256: 5.5, 768+: 5.7)
int pick_ksplit(int M, int N, long K) {
    const long tiles = (long)cdiv(M, 128) * cdiv(N, 128);
    long ks = DW_WGS / (tiles > 0 ? tiles : 1);
    if (ks > K / 256) ks = K / 256;
    if (ks > 32) ks = 32;
    if (ks < 1) ks = 1;
    return (int)ks;
}

// fp32 mode: the profile classes (bit SS_PROF_*) whose contractions take the image GEMM -- the decoder's input projections, the conv trunk's
// forward and input-gradient GEMMs.  The weight-gradient classes stay on round 2's kernel (split-K through partial slabs, gemm_on).
constexpr int IMG_CLASSES = (1 << SS_PROF_DEC_PROJ) | (1 << SS_PROF_CONV_FWD) | (1 << SS_PROF_CONV_DX);
constexpr int IMG_DW_WGS = 256;       // workgroups the split of a split-K (weight-gradient) image GEMM aims at

// Image GEMM (gemm_img.hip) for a contraction whose two operands exist as images.  Returns 1 when it was launched, 0 when the
// contraction has to take round 2's kernels (no images, shape outside what the image kernel supports), < 0 on error.
// klass: profile class of the contraction (SS_PROF_*; -1: none)
int try_img_gemm(ss_engine* e, const GemmDesc& d, hipStream_t st, int klass) {
    if (!d.a_pre || !d.b_pre) return 0;
    const bool b16 = e->img16();                     // the images are plain bf16 tensors: single-piece form, every class that has both
    if (!b16) {
        if (!(d.flags & GEMM_F16X2) || (d.flags & GEMM_BF16)) return 0;
        if (klass >= 0 && !((IMG_CLASSES >> klass) & 1) && !d.queue) return 0;
        // conv trunk at B x T <= 2048 rows: the image kernel's smallest tile (128 x 128) gives a 512-channel layer 64 workgroups; round 2's kernel
        // on 64 x 64 tiles fills the chip (16 x 128: 3.22 -> 3.17 ms, 12 x 128: 3.08 -> 3.04; equal at 8 x 128 and from 32 x 128 on)
        if ((klass == SS_PROF_CONV_FWD || klass == SS_PROF_CONV_DX) && (long)e->curB * e->curT <= 2048) return 0;
    }
    ImgGemmDesc g{};
    g.bf16 = b16 ? 1 : 0;
    g.A = {d.a_pre, d.A.ld, d.A.bstride, d.A.seglen, d.A.segstride};
    g.B = {d.b_pre, d.B.ld, d.B.bstride, d.B.seglen, d.B.segstride};
    g.C = d.C;
    g.ldc = d.ldc;
    g.cstride = d.cstride;
    g.bias = d.bias;
    g.M = d.M;
    g.N = d.N;
    g.K = d.K;
    g.batch = d.batch;
    g.flags = d.flags & (GEMM_TA | GEMM_TB | GEMM_ACCUM);
    g.row_period = d.row_period;
    g.row_off = d.row_off;
    g.row_lo = d.row_lo;
    g.row_hi = d.row_hi;
    g.scale_a = b16 ? nullptr : d.a_pre_scale;
    g.scale_b = b16 ? nullptr : d.b_pre_scale;
    g.zeros = e->zeros;
    g.cfg = -1;
    g.ksplit = 1;
    g.diag = g_gemm_diag;
    // Per-utterance batches of T rows over haloed slabs (and their flatten_rows form) become ONE matrix over the B * T real rows: the
    // kernel maps logical rows to slab rows, so the 256-row tiles neither end at every utterance nor compute halo rows
    const int T = e->curT;
    const long TP = T + 2 * HALO;
    if (!(g.flags & GEMM_TA) && T >= 32 && g.B.bstride == 0) {
        if (g.batch > 1 && g.M == T && !g.row_period && g.A.bstride == TP * g.A.ld && g.cstride == TP * g.ldc) {
            g.M = g.batch * T;
            g.batch = 1;
            g.A.bstride = g.cstride = 0;
            g.rm_T = T;
            g.rm_TP = (int)TP;
        } else if (g.batch == 1 && g.row_period == TP && g.row_off == HALO && g.row_lo == HALO && g.row_hi == HALO + T && (g.M + 2 * HALO) % TP == 0) {
            g.M = (int)((g.M + 2 * HALO) / TP) * T;
            g.row_period = 0;
            g.rm_T = T;
            g.rm_TP = (int)TP;
        }
    }
    // tile and split: measured on the step's shapes (tools/img_bench.py) -- without split-K the largest tile that still gives every CU a
    // workgroup; reductions that are much longer than the result is large (weight gradients, d.ksplit > 1 on entry: C is zeroed or
    // live) are cut along K into partial slabs, on 256 x 128 tiles (128 x 128 for narrow results)
    auto wgs = [&](int bm, int bn) { return (long)cdiv(g.M, bm) * cdiv(g.N, bn) * g.batch; };
    if (d.ksplit > 1 && !g.row_period) {
        g.cfg = (g.M >= 256 && g.N >= 128) ? 2 : 1;
        // 16-bit mode: 128 x 128 tiles (64 KB of LDS, two workgroups per CU).  The 256 x 128 form is 147 KB: one workgroup per CU, so the trunk's
        // weight-gradient GEMMs on the dependent chain queue for CUs behind the decoder's on the side streams (real_timeline: 147 us for a 32-us
        // launch).  32 x 128: 2.96 -> 2.91 ms, 64 x 128: 3.75 -> 3.69; the work-queue form keeps one workgroup per CU by design
        if (b16 && !d.queue) g.cfg = 1;
        const long t = g.cfg == 2 ? wgs(256, 128) : wgs(128, 128);
        long ks = ((d.queue ? 2 * IMG_DW_WGS : IMG_DW_WGS) + t / 2) / (t > 0 ? t : 1);       // work-queue form: twice the tiles (finer hand-over when the recurrence beside it ends)
        if (ks > g.K / 512) ks = g.K / 512;
        if (ks > 16) ks = 16;
        if (ks < 1) ks = 1;
        const long need = ks > 1 ? ks * (long)g.M * g.N * g.batch : 0;
        if (need && g.N % 4 == 0 && e->part && e->part_off + need <= e->part_cap) {
            g.ksplit = (int)ks;
            g.part = e->part + e->part_off;
            e->part_off += (need + 63) & ~63L;
        } else if (need) ++e->scratch_fallbacks;      // the contraction runs unsplit
    } else {
        g.cfg = wgs(256, 256) >= 256 ? 0 : (wgs(256, 128) >= 224 ? 2 : 1);
    }
    if (d.queue && e->wq_pool && e->bwd.wq_next < ss_engine::WQ_SLOTS) {
        // work-queue form on every XCD that will give it a CU; one workgroup per CU (128 / 144 KB of LDS), so that none fits beside a
        // recurrence workgroup
        if (g.cfg == 1) g.cfg = 2;
        g.wq = e->wq_pool + 4 * e->bwd.wq_next++;
        g.xcc_allow = 0xFFu;
    }
    if (!gemm_img_supported(g)) return 0;
    HIPCHK(launch_gemm_img(g, st));
    return 1;
}

// scratch of one column-sum launch (kernels.h colsum_acc): float64 partials from the step's bump allocator, counters from the ring
// (self-resetting; a launch's counters are not handed out again before COLSUM_CTRS / 64 later launches); null pointers: none left, the launch
// runs with one workgroup per column block
struct ColScratch {
    double* part = nullptr;
    unsigned* ctr = nullptr;
};
ColScratch colsum_scratch(ss_engine* e, int cols) {
    const long need = 2 * colsum_scratch_doubles(cols);          // in floats
    const int nb = cdiv(cols, 64);
    if (!e->part || !e->colsum_ctr || nb > ss_engine::COLSUM_CTRS || e->part_off + need > e->part_cap) {
        ++e->scratch_fallbacks;
        return {};
    }
    ColScratch cs;
    cs.part = (double*)(e->part + e->part_off);                  // part_off is kept at multiples of 64 floats
    e->part_off += (need + 63) & ~63L;
    if (e->colsum_next + nb > ss_engine::COLSUM_CTRS) e->colsum_next = 0;
    cs.ctr = e->colsum_ctr + e->colsum_next;
    e->colsum_next += nb;
    return cs;
}

int prof_begin(ss_engine* e, int klass, hipStream_t st, double flops);
void prof_end(ss_engine* e, int i, hipStream_t st);
// ss_profile bracket round the launches of one scope: the start event where it is made, the end event where the scope ends (on every way out)
struct Prof {
    ss_engine* e;
    hipStream_t st;
    int i;
    Prof(ss_engine* e_, int klass, hipStream_t st_, double flops = 0.0) : e(e_), st(st_), i(prof_begin(e_, klass, st_, flops)) {}
    ~Prof() { prof_end(e, i, st); }
    Prof(const Prof&) = delete;
    Prof& operator=(const Prof&) = delete;
};
// gradient norm (ss_set_grad_clip / ss_grad_norm): the arena is summed as [0, split) and [split, status_off), split = ss_grad_split when
// that is a float4 boundary -- the same two ranges on every route, so the norm has the same bits on every route
long clip_split(const ss_engine* e) {
    const long k = ss_grad_split(e);
    return (k % 4 == 0 && k > 0 && k < e->status_off) ? k : 0;
}
int clip_wgs_lo(const ss_engine* e) { return clip_split(e) > 0 ? grad_sumsq_wgs(clip_split(e)) : 0; }
// what every optimiser step of this engine does beyond Adam (ss_set_weight_decay, ss_set_ema): !on() while both are off, and every
// route then enqueues exactly what it did before they existed
AdamExt opt_ext(const ss_engine* e) {
    AdamExt x;
    x.ext = e->ext;
    x.wd = e->wd > 0.0f;
    x.runs = (x.wd && e->wd_which == 1) ? &e->wd_runs : nullptr;
    x.ema = e->ema;
    return x;
}
// the schedule state for the step's prepare kernel (ss_set_lr_schedule): NULL while it is off, and every route then enqueues the
// arguments it did before the schedule existed
LrSchedState* lr_sched(const ss_engine* e) { return e->lr_kind != LR_OFF ? e->sch : nullptr; }

// launch the pending encoder-BLSTM weight-gradient tasks (one kernel for all of them) on `st`: everything they read must be complete in
// st's order.  Scratch: partial tiles from the step's bump allocator, arrival counters from the column sums' ring.
int wgrad_flush(ss_engine* e, Backward& bw, hipStream_t st) {
    WgradTable& w = bw.wg;
    if (w.n == 0) return 0;
    w.row_groups = 16;
    const long need = (long)w.tiles_total * w.row_groups * 4096;
    if (!e->part || !e->colsum_ctr || w.tiles_total > ss_engine::COLSUM_CTRS || e->part_off + need > e->part_cap)
        return fail("wgrad_flush: no scratch left for the fused encoder-BLSTM weight gradients");
    w.part = e->part + e->part_off;
    e->part_off += (need + 63) & ~63L;
    if (e->colsum_next + w.tiles_total > ss_engine::COLSUM_CTRS) e->colsum_next = 0;
    w.ctr = e->colsum_ctr + e->colsum_next;
    e->colsum_next += w.tiles_total;
    {
        Prof pr(e, SS_PROF_WGRAD, st);
        HIPCHK(lstm_small_wgrad(w, st));
    }
    w.n = 0;               // (an error above ends the backward, and the table with it)
    w.tiles_total = 0;
    return 0;
}

// every contraction of the engine honours its precision mode (ss_set_precision)
int gemm_on(ss_engine* e, GemmDesc& d, hipStream_t st, int klass) {
    if (e->precision == SS_PRECISION_BF16) d.flags |= GEMM_BF16;
    const int r = try_img_gemm(e, d, st, klass);
    if (r < 0) return r;
    if (r == 0) {
        if (e->img16()) d.a_pre = d.b_pre = nullptr;        // plain bf16 tensors: not the format-v2 images round 2's kernel can take
        if (e->bwd.dg32_skipped) {                              // a decoder layer's fp32 gradient slab was not written: nothing may read it as an operand
            const long R8 = (long)e->curB * (e->curT + 2 * HALO) * 8L * e->ld.H;
            for (int l = 0; l < e->ld.L && l < 3; ++l)
                if (((e->bwd.dg32_skipped >> l) & 1) && ((d.A.p >= e->ld.gates[l] && d.A.p < e->ld.gates[l] + R8) || (d.B.p >= e->ld.gates[l] && d.B.p < e->ld.gates[l] + R8)))
                    return fail("internal: a contraction fell back to the fp32 gradient slab of a decoder layer that was only written as bf16");
        }
        // split-K weight gradients: partial slabs + ordered reduce instead of fp32 atomics, scratch from the step's bump allocator
        // (not for the encoder BLSTMs' tiny matrices: a one-block reduce over 32 slices is 17 us of latency, their atomics are nothing)
        if (d.ksplit > 1 && (d.flags & GEMM_TA) && (d.flags & GEMM_TB) && (d.flags & GEMM_ACCUM) && !d.row_period && !d.bias && d.N % 4 == 0 &&
            ((long)d.M * d.N >= 65536 || g_deterministic) && e->part) {        // deterministic mode: every split reduction through ordered slabs (small ones too)
            int ks = d.ksplit;
            const long need = (long)ks * d.M * d.N * (d.batch < 1 ? 1 : d.batch);
            if (e->part_off + need <= e->part_cap) {
                d.part = e->part + e->part_off;
                e->part_off += (need + 63) & ~63L;
            } else ++e->scratch_fallbacks;            // atomics (or, deterministic mode, no split) instead of ordered slabs
        }
        HIPCHK(launch_gemm(d, st));
    }
    return 0;
}
// Data parallel: the gradient range [off, off + count) is final once everything enqueued on `producer` so far has run -- hand it to a
// collective on the communication stream right away.  No-op outside a data-parallel step.
int dp_bucket(ss_engine* e, long off, long count, hipStream_t producer);

// make `to` wait for everything enqueued on `from` so far
int fork_join(ss_engine* e, hipStream_t from, hipStream_t to) {
    hipEvent_t ev = e->ev[e->ev_next];
    e->ev_next = (e->ev_next + 1) & 15;
    HIPCHK(hipEventRecord(ev, from));
    HIPCHK(hipStreamWaitEvent(to, ev, 0));
    return 0;
}

// Host-side view of the engine status word: no synchronisation, so it reports what earlier steps left behind.
int sticky_check(ss_engine* e) {
    if (!e->sticky) return 0;
    const unsigned v = *(volatile unsigned*)e->sticky;
    if (!v) return 0;
    if (v & SS_STICKY_RANGE)
        return fail("a parameter is not finite or left the range (|p| < 2048) the fixed-scale fp16 x 2 products of the WEIGHTS are valid for: the step "
                    "was not applied.  Use ss_tune(\"fwd_f16x2\", 0) and ss_tune(\"bwd_f16x2\", 0) (bf16 x 3 products, no range limit), then ss_clear_abort()");
    return fail(v & SS_STICKY_ABORT ? "a persistent LSTM kernel gave up waiting for its group (bounded spin expired) in an earlier step: that step's "
                                      "results were discarded and the parameters left untouched; ss_clear_abort() to continue"
                                    : "another data-parallel rank reported an aborted step: the update was skipped on every rank; ss_clear_abort() to continue");
}

// What a step / forward / Adam entry point does about the status word.  One engine on its own refuses to enqueue (its caller learns
// of the failure at once).  In LOCKSTEP mode (data parallel: ss_comm_init with world > 1, or ss_set_lockstep) it enqueues regardless:
// the word is set asynchronously, so ranks would see it at DIFFERENT host iterations, one would return while the others have already
// enqueued collectives that never get a partner.  The weights are safe either way (the Adam kernel skips on the device); the status is
// reported by ss_check(), which every rank calls at the same iteration, and cleared there by every rank (ss_clear_abort).
int entry_check(ss_engine* e) { return e->lockstep ? 0 : sticky_check(e); }

// Scope of one C-ABI call: work goes to the engine's main stream, which first waits for everything the caller's stream holds;
// on exit the caller's stream waits for the call's work, so the stream-ordered contract of the ABI is unchanged.
struct Own {
    ss_engine* e;
    hipStream_t caller, s;
    bool on = false;
    Own(ss_engine* e_, void* stream) : e(e_), caller((hipStream_t)stream), s((hipStream_t)stream) {
        if (e && e->main_s && g_own_streams && caller != e->main_s &&
            hipEventRecord(e->ev_io[0], caller) == hipSuccess && hipStreamWaitEvent(e->main_s, e->ev_io[0], 0) == hipSuccess) {
            s = e->main_s;
            on = true;
        }
    }
    ~Own() {
        if (on && hipEventRecord(e->ev_io[1], s) == hipSuccess) (void)hipStreamWaitEvent(caller, e->ev_io[1], 0);
    }
    Own(const Own&) = delete;
    Own& operator=(const Own&) = delete;
};

// a training step begins: is it one of the bracketed ones (ss_profile_sample)?
void prof_tick(ss_engine* e) {
    e->prof_live = e->prof_every <= 1 || (e->prof_ctr % e->prof_every) == 0;
    ++e->prof_ctr;
}

// ss_profile: bracket one launch with hipEvents on the stream it is launched on
int prof_begin(ss_engine* e, int klass, hipStream_t st, double flops) {
    if (!((e->prof_mask >> klass) & 1u) || !e->prof_live || e->prof_n >= ss_engine::PROF_CAP) return -1;
    const int i = e->prof_n;
    while ((int)e->prof_ev.size() < 2 * (i + 1)) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return -1;
        e->prof_ev.push_back(ev);
    }
    if ((int)e->prof_rec.size() <= i) e->prof_rec.resize(i + 1);
    e->prof_rec[i] = {klass, flops, st == e->side ? 1 : (st == e->side2 ? 2 : (st == e->side3 ? 3 : 0))};
    if (hipEventRecord(e->prof_ev[2 * i], st) != hipSuccess) return -1;
    e->prof_n = i + 1;
    return i;
}
void prof_end(ss_engine* e, int i, hipStream_t st) {
    if (i >= 0) (void)hipEventRecord(e->prof_ev[2 * i + 1], st);
}
// ALGORITHMIC work of a contraction (ss_profile): halo rows are not work -- a reduction over all B * (T + 4) slab rows counts B * T of
// them, a flattened row-masked matrix its B * T stored rows (round-2 review: the weight gradients' count was 3 % high)
double gemm_flops_of(const ss_engine* e, const GemmDesc& d) {
    double M = (double)d.M * (d.batch > 0 ? d.batch : 1), K = (double)d.K;
    const long TP = e->curT + 2 * HALO, R = (long)e->curB * TP;
    if ((d.flags & GEMM_TA) && (d.flags & GEMM_TB) && d.K >= R - 2 * HALO && d.K <= R) K = (double)e->curB * e->curT;
    if (d.row_period == TP && d.batch <= 1) M = (double)((d.M + 2 * HALO) / TP) * e->curT;
    return 2.0 * M * d.N * K;
}
#define gemm_flops(d) gemm_flops_of(e, d)
// GEMM launch bracketed as profile class `k`
#define PGEMM_ON(k, d, st)                          \
    do {                                            \
        Prof _pr(e, k, st, gemm_flops(d));          \
        CHK(gemm_on(e, d, st, k));                  \
    } while (0)
// forward contraction: both operands are O(1) by construction
#define PGEMM_FWD_ON(k, d, st)                      \
    do {                                            \
        if (g_fwd_f16x2) (d).flags |= GEMM_F16X2;   \
        PGEMM_ON(k, d, st);                         \
    } while (0)

// A per-utterance batched contraction over haloed slabs (M = T rows per batch entry, A / C pointing at slab row HALO) rewritten as
// ONE matrix over all slab rows between the first and the last halo, halo rows masked in the epilogue.  Batched, every utterance
// starts a new row tile: T = 144 needs two 128-row tiles per utterance (78 % of the rows computed are padding), T = 192 wastes 25 %.
// Worth it whenever T is not a multiple of the 128-row tile.  The A operand's rows are addressed exactly as before (row m of the
// flat matrix is slab row m + HALO, taps reach into the neighbouring rows; rows computed for halo positions are never stored).
void flatten_rows(GemmDesc& d, int B, int T) {
    if (T % 128 == 0 || d.batch != B || B < 2) return;
    const int TP = T + 2 * HALO;
    d.M = B * TP - 2 * HALO;
    d.batch = 1;
    d.A.bstride = 0;
    d.cstride = 0;
    d.row_period = TP;
    d.row_off = HALO;
    d.row_lo = HALO;
    d.row_hi = HALO + T;
}

// ---- convolution block -------------------------------------------------------------------------------------
int conv_pack_all(ss_engine* e, ConvBlk& cb, hipStream_t s) {
    const bool img = cb.img_ok();
    HIPCHK(conv_pack(e->P + cb.w, cb.Co, cb.Ci, cb.Cp, cb.wf, cb.wb, img ? cb.wf_img : nullptr, img ? cb.wb_img : nullptr, s, e->img16()));
    return 0;
}

constexpr int CONV_WANT = 256;    // workgroup target of the conv GEMMs' tile choice (GemmDesc::want)

int zero_conv_grads(ss_engine* e, hipStream_t s) {
    HIPCHK(hipMemsetAsync(e->gp_all, 0, e->gp_bytes, s));
    return 0;
}

// where the image of a conv-output gradient slab view goes (the trunk's views share d_img, Encoder_t's has d_img_t); null: no image
float* grad_img_of(ss_engine* e, const float* p, long R) {
    auto in = [&](const float* b, long cols) { return b && p >= b && p < b + R * cols; };
    if (in(e->d_act, e->CE)) return e->ioff(e->d_img, p - e->d_act);
    for (int i = 0; i < 2; ++i)
        if (in(e->d_act_l[i], e->CE)) return e->ioff(e->d_img_l[i], p - e->d_act_l[i]);
    if (in(e->d_xf, e->CE)) return e->ioff(e->d_img, p - e->d_xf);
    if (in(e->d_act_t, e->hp.dim_enc_2)) return e->ioff(e->d_img_t, p - e->d_act_t);
    return nullptr;
}

// y = relu(GN(conv5(x)))   x: slab view (ld), y: slab view
struct ConvFwd {
    // gather (nullable): the resampling plan of the training forward -- GroupNorm + ReLU + gather in one kernel straight into gy / gy_img (the
    // resampled slab from the block's first column on, and its image at gy's position), behind gather_ready (nullable); y is then not written
    const InterpPlan* gather = nullptr;
    Rows gy;
    float* gy_img = nullptr;
    hipEvent_t gather_ready = nullptr;
    // lens (nullable; eval-mode forwards only): per-row lengths of a ragged batch, device i32[B] -- the GroupNorm takes its statistics over each
    // row's own frames and writes zeros behind them (the convolution itself is row-wise over a slab whose padded rows its producer zeroed)
    const int* lens = nullptr;
};
int conv_block_fwd(ss_engine* e, ConvBlk& cb, Slab x, Slab y, hipStream_t s, const ConvFwd& o = {}) {
    const int B = e->curB, T = e->curT;
    const long TP = T + 2 * HALO;
    GemmDesc d{};
    d.A = {x.p, x.ld, TP * x.ld, cb.Cp, x.ld};
    d.a_pre = x.img;
    d.a_pre_scale = x.scale;
    d.B = {cb.wf, 5L * cb.Cp, 0, 0, 0};
    d.b_pre = cb.img_ok() ? cb.wf_img : nullptr;
    d.C = cb.cout + HALO * cb.Co;
    d.ldc = cb.Co;
    d.cstride = TP * cb.Co;
    d.bias = e->P + cb.b;
    d.M = T;
    d.N = cb.Co;
    d.K = 5 * cb.Cp;
    d.batch = B;
    d.ksplit = 1;
    d.want = CONV_WANT;
    flatten_rows(d, B, T);
    PGEMM_FWD_ON(SS_PROF_CONV_FWD, d, s);
    if (o.gather) {
        if (o.gather_ready) HIPCHK(hipStreamWaitEvent(s, o.gather_ready, 0));
        Prof pr(e, SS_PROF_GN, s);
        HIPCHK(gn_relu_gather(CRows::slab(cb.cout, cb.Co, T), o.gy, e->P + cb.ga, e->P + cb.be, cb.stats, *o.gather, B, T, cb.Co, s,
                              {.y_img = o.gy_img, .img_scale = e->act_scale + cb.scale_i, .img_bf16 = e->img16()}));
        return 0;
    }
    // T > 256 (eval only): the chunked GroupNorm takes its float64 partials from the step's scratch (one region per block: blocks run
    // side by side on different streams)
    double* gn_scratch = nullptr;
    if (const long gb = gn_relu_fwd_scratch_bytes(B, T, cb.Co)) {
        const long need = (gb / 4 + 63) & ~63L;
        if (!e->part || e->part_off + need > e->part_cap) return fail("conv_block_fwd: no scratch left for the long-sequence GroupNorm");
        gn_scratch = (double*)(e->part + e->part_off);          // part_off is kept at multiples of 64 floats
        e->part_off += need;
    }
    Prof pr(e, SS_PROF_GN, s);
    HIPCHK(gn_relu_fwd(CRows::slab(cb.cout, cb.Co, T), y.rows(T), e->P + cb.ga, e->P + cb.be, cb.stats, B, T, cb.Co, s, gn_scratch, o.lens));
    return 0;
}

// dy: gradient of the block output (slab view, overwritten in place with the conv-output gradient);
// x: the block's forward input; dx: where to put the input gradient (p == nullptr: not needed)
// bw: collects the weight gradient's re-layout (unpack_later) and names the caller buffer of a layer-0 block's input gradient
struct ConvBwd {
    // scatter / src (nullable): the block's output was resampled in the forward (training): src is the gradient of the RESAMPLED output (from
    // this block's first column on); the gather's adjoint is taken inside the GroupNorm backward, which writes dy
    const InterpPlan* scatter = nullptr;
    CRows src;
    // dws (nullable): the weight-gradient GEMM goes to that stream behind an event, the chain on `s` does not wait for it -- the caller keeps dy
    // untouched until dws is joined
    hipStream_t dws = nullptr;
};
int conv_block_bwd(ss_engine* e, Backward& bw, ConvBlk& cb, Slab dy, Slab x, Slab dx, hipStream_t s, const ConvBwd& o = {}) {
    const int B = e->curB, T = e->curT;
    const long TP = T + 2 * HALO, R = (long)B * TP;
    float* am = (g_bwd_f16x2 && cb.amax_i >= 0) ? e->amax + cb.amax_i : nullptr;
    const bool i16 = e->img16();
    // 16-bit data path: the GroupNorm backward writes the gradient's bf16 image itself (the image's halo rows are zero since the geometry
    // was planned and nobody writes them); fp32 mode: a split_image pass with the scale gn_relu_bwd has just measured
    float* im16 = (i16 && cb.Co % 8 == 0 && dy.ld % 8 == 0) ? grad_img_of(e, dy.p, R) : nullptr;
    {
        Prof pr(e, SS_PROF_GN, s);
        HIPCHK(gn_relu_bwd(CRows::slab(cb.cout, cb.Co, T), dy.rows(T), e->P + cb.ga, e->P + cb.be, cb.stats, e->G + cb.ga, e->G + cb.be, e->G + cb.b, B, T, cb.Co, s,
                           {.amax = am, .part = cb.part, .scatter = o.scatter, .src = o.src, .dy_img = im16}));
    }
    // the conv-output gradient as an image for the image GEMM (scale: the power of two for the maximum gn_relu_bwd has just measured)
    const float* dimg = im16;
    const float* dsc = nullptr;
    if (!i16 && am && e->precision == SS_PRECISION_F32 && cb.Co % 8 == 0 && dy.ld % 8 == 0) {
        float* im = grad_img_of(e, dy.p, R);
        if (im) {
            HIPCHK(split_image(dy.p, dy.ld, R, cb.Co, am, 0.f, im, dy.ld, e->gscale + cb.amax_i, s));
            dimg = im;
            dsc = e->gscale + cb.amax_i;
        }
    }
    // weight gradient: one reduction over every slab row (halo rows of dy are zero); cb.gp was zeroed by zero_conv_grads
    GemmDesc d{};
    d.A = {dy.p + 2 * dy.ld, dy.ld, 0, 0, 0};
    if (dimg) {
        d.a_pre = e->ioff(dimg, 2 * dy.ld);
        d.a_pre_scale = dsc;
    }
    d.B = {x.p, x.ld, 0, cb.Cp, x.ld};
    d.b_pre = x.img;
    d.b_pre_scale = x.scale;
    d.C = cb.gp;
    d.ldc = 5L * cb.Cp;
    d.M = cb.Co;
    d.N = 5 * cb.Cp;
    d.K = (int)(R - 4);
    d.batch = 1;
    d.flags = GEMM_TA | GEMM_TB | GEMM_ACCUM | (am ? GEMM_F16X2 : 0);
    d.amax_a = am;                                  // gradient operand: measured scale; the block input is O(1)
    d.ksplit = pick_ksplit(d.M, d.N, d.K);
    hipStream_t dws = o.dws ? o.dws : s;
    if (dws != s) CHK(fork_join(e, s, dws));
    PGEMM_ON(SS_PROF_CONV_DW, d, dws);
    // packed [Co][5][Cp] -> the parameter's [Co][Ci][5]: nobody reads it before the optimiser (or, data parallel, the layer's bucket), so the
    // one-GPU step collects the blocks and unpacks them all in one launch at the end of the backward (backward_encoder) instead of seven
    // small launches on the trunk's dependent chain
    if (bw.unpack_later && bw.unpack.n < CONV_UNPACK_MAX) bw.unpack.t[bw.unpack.n++] = {cb.gp, e->G + cb.w, cb.Co, cb.Ci, cb.Cp};
    else HIPCHK(conv_unpack_grad(cb.gp, cb.Co, cb.Ci, cb.Cp, e->G + cb.w, dws, bw.accumulate));
    // input gradient: dy against the flipped taps, T rows per utterance, into rows of stride ldc (utterances cstride apart)
    auto dx_desc = [&](const float* taps, float* C, long ldc, long cstride) {
        GemmDesc g{};
        g.A = {dy.p, dy.ld, TP * dy.ld, cb.Co, dy.ld};
        g.B = {taps, 5L * cb.Co, 0, 0, 0};
        g.C = C;
        g.ldc = ldc;
        g.cstride = cstride;
        g.M = T;
        g.N = cb.Ci;
        g.K = 5 * cb.Co;
        g.batch = B;
        g.ksplit = 1;
        g.flags = am ? GEMM_F16X2 : 0;
        g.amax_a = am;
        g.want = CONV_WANT;
        return g;
    };
    if (dx.p) {
        GemmDesc g = dx_desc(cb.wb, dx.p + HALO * dx.ld, dx.ld, TP * dx.ld);
        if (dimg) {
            g.a_pre = dimg;
            g.a_pre_scale = dsc;
        }
        g.b_pre = cb.img_ok() ? cb.wb_img : nullptr;
        flatten_rows(g, B, T);
        PGEMM_ON(SS_PROF_CONV_DX, g, s);
    }
    if (const Backward::InputGrad* tg = bw.input_grad_of(cb)) {
        // the block's input is the network input (ss_g*_backward_inputs): the same contraction against taps packed for this call (the forward
        // packs none for layer 0), stored straight into the caller's dense [B][T] rows -- per-utterance batches of T rows, so no halo row is
        // ever computed or stored, and the halo rows of dy (zero) are what the taps past either end of an utterance read
        if (!cb.wb0) return fail("internal: input gradient asked of a conv block without its tap buffer");
        HIPCHK(conv_pack_dx(e->P + cb.w, cb.Co, cb.Ci, cb.wb0, s));
        GemmDesc g = dx_desc(cb.wb0, tg->p, tg->ld, (long)T * tg->ld);
        PGEMM_ON(SS_PROF_CONV_DX, g, s);
    }
    return 0;
}

// ---- BLSTM block -------------------------------------------------------------------------------------------
// Per-step re-layouts of one BLSTM block's weights: b_ih + b_hh per (layer, direction) and, for the decoder-size blocks,
// the fragment-major W_hh of the forward recurrence.  Independent of the activations, so the schedule runs it on a branch.
int lstm_prep(ss_engine* e, LstmBlk& lb, PrepTable& tb, hipStream_t s) {
    const int H = lb.H;
    const bool persist = lb.persist(e);
    for (int l = 0; l < lb.L; ++l) {
        for (int dir = 0; dir < 2; ++dir) {
            const LstmDir& pd = lb.pd[l * 2 + dir];
            const long n = 4L * H * lb.in_of(l);
            if (tb.n + 2 > PREP_MAX) return fail("lstm_prep: task table full");
            tb.t[tb.n++] = {e->P + pd.bih, e->P + pd.bhh, lb.bsum + ((long)l * 2 + dir) * 4 * H, 4L * H};       // summed biases
            tb.t[tb.n++] = {e->P + pd.wih, nullptr, lb.wcat[l] + dir * n, n, (lb.wcat_img[l] && lb.in_of(l) % 8 == 0) ? e->ioff(lb.wcat_img[l], dir * n) : nullptr};      // stacked W_ih (+ image: rows of whole groups of eight)
        }
        // fragment-major W_hh for the one-launch-per-step schedule (the persistent kernels read the parameters directly)
        if (lb.big() && !persist) HIPCHK(lstm_pack_w(e->P + lb.pd[l * 2].whh, e->P + lb.pd[l * 2 + 1].whh, lb.wfrag[l], H, 0, s));
    }
    if (lb.big() && persist) HIPCHK(hipMemsetAsync(lb.zf, 0, lb.zf_bytes, s));     // h(-1) = 0 and the group counters of every layer
    return 0;
}

// input projections of layer l over the slab xi: both directions in one GEMM against the stacked W_ih / summed biases of lstm_prep (N = 8H)
GemmDesc lstm_proj_desc(const ss_engine* e, const LstmBlk& lb, int l, Slab xi) {
    const int B = e->curB, T = e->curT, H = lb.H;
    const long TP = T + 2 * HALO;
    GemmDesc d{};
    d.A = {xi.p + HALO * xi.ld, xi.ld, TP * xi.ld, 0, 0};
    d.B = {lb.wcat[l], lb.in_of(l), 0, 0, 0};
    d.b_pre = lb.wimg(l);
    d.C = lb.gates[l] + HALO * 8L * H;
    d.ldc = 8L * H;
    d.cstride = TP * 8L * H;
    d.bias = lb.bsum + (long)l * 8 * H;
    d.M = T;
    d.N = 8 * H;
    d.K = lb.in_of(l);
    d.batch = B;
    d.ksplit = 1;
    flatten_rows(d, B, T);
    return d;
}

// Decoder-size BLSTM: one persistent launch per layer, or one launch per time step (persist = 0 / a batch the persistent kernels do not take).
int lstm_big_fwd(ss_engine* e, LstmBlk& lb, Slab x, hipStream_t s, const int* lens) {
    const int B = e->curB, T = e->curT, H = lb.H;
    const bool persist = lb.persist(e);
    // only fp16 x 2 GEMMs read the hidden states' pre-split images, and only the persistent recurrences write them
    lb.out_img_valid = persist && ((e->precision == SS_PRECISION_F32 && g_fwd_f16x2) || e->img16()) && !lb.out_img.empty() && lb.out_img[0];
    const long half = 2L * (((B + 15) / 16) * 16) * H;       // one of the two ping-pong h(t) tiles of the per-step schedule
    for (int l = 0; l < lb.L; ++l) {
        const int In = lb.in_of(l);
        Slab xi = l == 0 ? x : Slab{lb.out[l - 1], 2L * H};
        const bool compact = l == 0 && lb.xf && persist && x.p == lb.xc;       // the input repeats in blocks of xf frames: one projection row per block
        if (compact) {
            GemmDesc d{};
            d.A = {lb.xc, In, 0, 0, 0};
            d.B = {lb.wcat[l], In, 0, 0, 0};
            d.b_pre = lb.wimg(l);
            d.C = lb.xp0;
            d.ldc = 8L * H;
            d.bias = lb.bsum + (long)l * 8 * H;
            d.M = B * (T / lb.xf);
            d.N = 8 * H;
            d.K = In;
            d.batch = 1;
            d.ksplit = 1;
            PGEMM_FWD_ON(SS_PROF_DEC_PROJ0, d, s);
        } else {
            GemmDesc d = lstm_proj_desc(e, lb, l, xi);
            if (l > 0 && lb.out_img_valid) d.a_pre = e->ioff(lb.out_img[l - 1], HALO * xi.ld);       // written by the layer below's recurrence
            PGEMM_FWD_ON(l > 0 ? SS_PROF_DEC_PROJ : SS_PROF_DEC_PROJ0, d, s);
        }
        if (persist) {   // start state zeroed by lstm_prep
            // the input projections the GEMM has just written are read once more, in whole lines, beside the recurrence (lstm_seq.hip)
            // (worth it from ~48 utterances on: 64 x 128 -0.08 ms; at 32 and 16 the fork / join around the recurrence costs more than warm operands
            // gain: 32 x 128 bf16 3.00 vs 2.97 ms without, 16 x 128 3.28 vs 3.26)
            const bool pw = e->side3 && g_overlap && !compact && B > 32;
            if (pw) {
                CHK(fork_join(e, s, e->side3));
                HIPCHK(slab_prewarm(lb.gates[l], 8 * H, e->amax, B, T, e->side3, {.cn = 2 * H}));
            }
            {
                Prof pr(e, SS_PROF_REC_FWD, s, 2.0 * 2 * B * T * 4.0 * H * H);
                // 16-bit data path: bf16 images, products of the high fp16 pieces only
                HIPCHK(lstm_seq_fwd(lb.gates[l], e->P + lb.pd[l * 2].whh, e->P + lb.pd[l * 2 + 1].whh, lb.hf_l(l), lb.out[l], lb.csave[l], lb.sync_f(l), B, T, H, s,
                                    {.sticky = e->sticky, .xc = compact ? lb.xp0 : nullptr, .xf = compact ? lb.xf : 0,
                                     .out_img = lb.out_img_valid ? lb.out_img[l] : nullptr, .img_bf16 = e->img16(), .hi_only = e->img16(),
                                     .state_zeroed = true, .len = lens}));
            }
            if (pw) CHK(fork_join(e, e->side3, s));
            continue;
        }
        HIPCHK(hipMemsetAsync(lb.hf, 0, 2 * half * 4, s));
        for (int st = 0; st < T; ++st)
            HIPCHK(lstm_step_fwd(lb.gates[l], lb.wfrag[l], lb.hf + (st & 1) * half, lb.hf + ((st & 1) ^ 1) * half, lb.out[l], lb.csave[l], B, T, H, st, s, lens));
    }
    return 0;
}

// lens (nullable): per-row lengths of a ragged eval-mode batch; every recurrence of the block zeroes the state of rows behind their end
int lstm_fwd(ss_engine* e, LstmBlk& lb, Slab x, hipStream_t s, const int* lens = nullptr) {
    if (lb.big()) return lstm_big_fwd(e, lb, x, s, lens);
    const int B = e->curB, T = e->curT, H = lb.H;
    for (int l = 0; l < lb.L; ++l) {
        Slab xi = l == 0 ? x : Slab{lb.out[l - 1], lb.ow()};      // layer 1: K = 2H real columns of the (possibly padded) rows
        GemmDesc d = lstm_proj_desc(e, lb, l, xi);
        d.a_pre_scale = xi.scale;                  // conv-block output (layer 0); hidden states |h| < 1 take the fixed 16
        PGEMM_FWD_ON(SS_PROF_ENC_LSTM, d, s);
        Prof pr(e, SS_PROF_ENC_REC, s);
        HIPCHK(lstm_small_fwd(lb.gates[l], e->P + lb.pd[l * 2].whh, e->P + lb.pd[l * 2 + 1].whh, lb.out[l], lb.csave[l], B, T, H, s, lens));
    }
    return 0;
}

// d_top: gradient slab of the last layer's output [B,TP,2H]; x: forward input; dx: input-gradient view or null
// weight / bias gradients of one layer from its finished pre-activation gradient slab (full batch, flat over all rows)
// W_ih gradient of decoder layer l (both directions, one launch) as a work-queue image GEMM, in two calls: lstm_wih_split makes the image
// of the layer's pre-activation gradients (split_image; as soon as its recurrence is through), lstm_wih_gemm_queued contracts it against
// the layer input's image (the hidden states of layer l - 1, written by the forward recurrence).  `gate` (nullable): the sync words of the
// persistent recurrence the launch is meant to run beside -- the GEMM is dispatched once that grid is resident (seq_gate).
bool lstm_wih_queue_ok(ss_engine* e, LstmBlk& lb, int l, const float* am) {
    if (!am || &lb != &e->ld || l < 1 || l >= 3 || !e->dg_img[l] || e->precision != SS_PRECISION_F32 || !g_bwd_f16x2) return false;
    if (!lb.out_img_valid || !lb.out_img[l - 1] || !e->wq_pool || e->bwd.wq_next >= ss_engine::WQ_SLOTS) return false;
    return lb.pd[l * 2 + 1].wih > lb.pd[l * 2].wih;
}
int lstm_wih_split(ss_engine* e, LstmBlk& lb, int l, const float* am, hipStream_t ws) {
    const long TP = e->curT + 2 * HALO, R = (long)e->curB * TP;
    HIPCHK(split_image(lb.gates[l], 8L * lb.H, R, 8 * lb.H, am, 0.f, e->dg_img[l], 8L * lb.H, e->gscale + lb.amax0 + l, ws));
    return 0;
}
int lstm_wih_gemm_queued(ss_engine* e, LstmBlk& lb, int l, const float* am, const unsigned* gate, hipStream_t ws) {
    const int B = e->curB, T = e->curT, H = lb.H;
    const long TP = T + 2 * HALO, R = (long)B * TP;
    const int In = lb.in_of(l);
    const LstmDir &p0 = lb.pd[l * 2], &p1 = lb.pd[l * 2 + 1];
    if (gate) HIPCHK(seq_gate(gate, B, H, ws));
    GemmDesc a{};
    a.A = {lb.gates[l], 8L * H, 4L * H, 0, 0};
    a.B = {lb.out[l - 1], 2L * H, 0, 0, 0};
    a.a_pre = e->dg_img[l];
    a.a_pre_scale = e->gscale + lb.amax0 + l;
    a.b_pre = lb.out_img[l - 1];
    a.C = e->G + p0.wih;
    a.ldc = In;
    a.cstride = p1.wih - p0.wih;
    a.M = 4 * H;
    a.N = In;
    a.K = (int)R;
    a.batch = 2;
    a.flags = GEMM_TA | GEMM_TB | GEMM_ACCUM | GEMM_F16X2;
    a.amax_a = am;
    a.ksplit = 4;                   // > 1: the image path cuts the reduction into partial slabs
    a.queue = 1;
    int r;
    {
        Prof pr(e, SS_PROF_DEC_DW, ws, 2.0 * a.M * a.N * (double)B * T * a.batch);
        r = try_img_gemm(e, a, ws, SS_PROF_DEC_DW);
    }
    if (r < 0) return r;
    if (r == 0) return fail("lstm_wih_gemm_queued: the image GEMM refused a shape the engine planned for it");
    e->bwd.dec_ih_done |= 1 << l;
    return 0;
}

// Returns 1 when each direction of the layer has been handed to a data-parallel collective here (the caller's per-layer bucket then has
// nothing left to send), 0 when not, < 0 on error.
int lstm_weight_grads(ss_engine* e, Backward& bw, LstmBlk& lb, int l, Slab xi, const float* am, bool bias_done, hipStream_t ws, DwRoute route = {}) {
    const int B = e->curB, T = e->curT, H = lb.H;
    const long TP = T + 2 * HALO, R = (long)B * TP;
    const int In = lb.in_of(l);
    float* dG = lb.gates[l];
    const LstmDir &p0 = lb.pd[l * 2], &p1 = lb.pd[l * 2 + 1];
    if (!lb.big() && H <= 32 && !bias_done && e->part && e->colsum_ctr && bw.wg.n < WGRAD_MAX &&
        e->part_off + (long)(bw.wg.tiles_total + lstm_small_wgrad_tiles(H, In)) * 16 * 4096 <= e->part_cap) {
        // encoder BLSTMs: one fused fp32 kernel for the weight and bias gradients of every layer (lstm_wgrad.hip) instead of 12-14 tiny GEMMs + column sums
        WgradTask& t = bw.wg.t[bw.wg.n];
        t = WgradTask{dG, xi.p, xi.ld, lb.out[l], e->G + p0.wih, e->G + p1.wih, e->G + p0.whh, e->G + p1.whh, e->G + p0.bih, e->G + p0.bhh, e->G + p1.bih,
                      e->G + p1.bhh, H, In, R, bw.wg.tiles_total, (int)lb.ow()};
        bw.wg.tiles_total += lstm_small_wgrad_tiles(H, In);
        ++bw.wg.n;
        if (!bw.wg_defer) CHK(wgrad_flush(e, bw, ws));
        return 0;
    }
    const bool compact = l == 0 && lb.xf && xi.p == lb.xc;     // dW_ih from the block sums and one input row per block (K / xf)
    // the hidden-state slabs of a decoder-size block on the persistent kernels also exist as pre-split images (written by the forward)
    const bool img_ok = lb.out_img_valid && lb.out_img[l];
    // 16-bit data path: the decoder's pre-activation gradients as a bf16 image for the image GEMM, written by the backward recurrence's storing
    // wave.  (fp32 mode: the weight gradients are not in the image class set, IMG_CLASSES, and stay on round 2's kernel.)
    const float* dimg = nullptr;
    if (e->img16() && &lb == &e->ld && l < 3 && ((e->bwd.dg16_written >> l) & 1) && img_ok) dimg = e->dg_img[l];
    const int klass = lb.big() ? SS_PROF_DEC_DW : SS_PROF_ENC_LSTM;
    // Every contraction here is  dW[n][k] += sum_r dG[r][n] * X[r][k]  into the gradient arena at w_off: 4H rows, N columns (the row length
    // of W), reduced over K slab rows; batch = 2: both directions in one launch, their parameters one stride apart.  The gradient slab
    // carries its measured scale; the layer input is O(1).
    auto dw_desc = [&](Operand A, Operand X, long w_off, int N, long K, int batch) {
        GemmDesc d{};
        d.A = A;
        d.B = X;
        d.C = e->G + w_off;
        d.ldc = N;
        d.cstride = batch > 1 ? p1.wih - p0.wih : 0;
        d.M = 4 * H;
        d.N = N;
        d.K = (int)K;
        d.batch = batch;
        d.flags = GEMM_TA | GEMM_TB | GEMM_ACCUM | (am ? GEMM_F16X2 : 0);
        d.amax_a = am;
        d.ksplit = pick_ksplit(d.M, d.N, d.K);
        d.queue = (batch > 1 && route.queue) ? 1 : 0;
        return d;
    };
    // data parallel: one direction's parameters (W_ih, W_hh, b_ih, b_hh: contiguous in the arena) are final on its stream -- half a layer per
    // collective keeps the communication stream busy 140 us earlier than a bucket per layer (modelled N = 8: the last collective ends
    // closer to the backward's end)
    bool dir_buckets = false;
    auto dir_bucket = [&](const LstmDir& pd, hipStream_t st_ih, hipStream_t st) -> int {
        if (&lb != &e->ld || !e->dp_on || route.part != 0 || pd.bhh + 4L * H <= pd.wih) return 0;
        if (st_ih != st) return fail("internal: a direction's weight gradients on two streams under data parallelism");
        CHK(dp_bucket(e, pd.wih, pd.bhh + 4L * H - pd.wih, st));
        dir_buckets = true;
        return 0;
    };
    // Both directions in ONE launch each (batch = 2) when their parameters sit at one stride in the arena (PyTorch's order: they do).
    // dW_hh: h_prev is `out` one row earlier (forward) / later (reverse), so the forward direction reads dG one row later instead.
    // (With the image GEMM the decoder's launches are batched as well: 64 + 32 tile jobs per layer instead of 4 x (32 or 16) halve the
    // split-K factor, i.e. the partial-slab traffic and the number of reduce passes.)
    // The encoder BLSTMs always (36 -> 14 launches); the decoder only with images (without: measured step +0.18 ms).
    const bool img_batch = dimg != nullptr;
    if ((!compact || img_batch) && (!lb.big() || img_batch) && p1.wih - p0.wih == p1.whh - p0.whh && p1.wih > p0.wih) {
        if (!compact && route.part != 2) {
            GemmDesc a = dw_desc({dG, 8L * H, 4L * H, 0, 0}, {xi.p, xi.ld, 0, 0, 0}, p0.wih, In, R, 2);
            a.b_pre_scale = l == 0 ? xi.scale : nullptr;      // a conv block's output carries its own split scale (act_scales): right whichever product mode runs
            if (dimg && l > 0) {
                a.a_pre = dimg;
                a.b_pre = lb.out_img[l - 1];
            }
            PGEMM_ON(klass, a, ws);
        }
        GemmDesc h = dw_desc({dG + 8L * H, 8L * H, 4L * H - 8L * H, 0, 0},                    // forward: rows 1 .., reverse: rows 0 .. of its own columns
                             {lb.out[l], lb.ow(), lb.ow() + H, 0, 0}, p0.whh, H, R - 1, 2);    // forward: rows 0 .. of h_f, reverse: rows 1 .. of h_b
        if (dimg) {
            h.a_pre = e->ioff(dimg, 8L * H);
            h.b_pre = lb.out_img[l];
        }
        PGEMM_ON(klass, h, ws);
        if (!bias_done) {
            const ColScratch cs = colsum_scratch(e, 8 * H);
            HIPCHK(colsum_bias(dG, 8L * H, (int)R, 4 * H, e->G + p0.bih, e->G + p0.bhh, e->G + p1.bih, e->G + p1.bhh, cs.part, cs.ctr, ws));
        }
        if (!compact) return 0;
        // compact layer 0: dW_hh went out batched above, dW_ih comes from the block sums below, per direction
        for (int dir = 0; dir < 2; ++dir) {
            const LstmDir& pd = lb.pd[l * 2 + dir];
            GemmDesc c = dw_desc({lb.dgs + dir * 4L * H, 8L * H, 0, 0, 0}, {xi.p, xi.ld, 0, 0, 0}, pd.wih, In, B * (T / lb.xf), 1);
            PGEMM_ON(SS_PROF_DEC_DW, c, ws);
            CHK(dir_bucket(pd, ws, ws));
        }
        return dir_buckets ? 1 : 0;
    }
    for (int dir = 0; dir < 2; ++dir) {
        const LstmDir& pd = lb.pd[l * 2 + dir];
        const float* dGd = dG + dir * 4L * H;
        hipStream_t wa = (dir == 1 && route.over_ih) ? route.over_ih : ws, wh = (dir == 1 && route.over_hh) ? route.over_hh : ws;
        if (route.part != 2 || compact) {      // dW_ih[n][k] = sum_r dG[r][n] * X[r][k]
            GemmDesc a = dw_desc({compact ? lb.dgs + dir * 4L * H : dGd, 8L * H, 0, 0, 0}, {xi.p, xi.ld, 0, 0, 0}, pd.wih, In, compact ? B * (T / lb.xf) : R, 1);
            if (dimg && !compact) a.a_pre = e->ioff(dimg, a.A.p - dG);
            if (img_ok && l > 0) a.b_pre = lb.out_img[l - 1];
            PGEMM_ON(klass, a, wa);
        }
        // dW_hh[n][k] = sum_r dG[r][n] * h_prev[r][k];  h_prev = out one row earlier (fwd) / later (reverse)
        GemmDesc h = dw_desc({dir == 0 ? dGd + 8L * H : dGd, 8L * H, 0, 0, 0}, {dir == 0 ? lb.out[l] : lb.out[l] + lb.ow() + H, lb.ow(), 0, 0, 0}, pd.whh, H, R - 1, 1);
        if (dimg) h.a_pre = e->ioff(dimg, h.A.p - dG);
        if (img_ok) h.b_pre = dir == 0 ? lb.out_img[l] : e->ioff(lb.out_img[l], 2L * H + H);
        PGEMM_ON(klass, h, wh);
        if (!bias_done) {     // the persistent backward kernel accumulates both bias gradients itself
            const ColScratch cs = colsum_scratch(e, 4 * H);
            HIPCHK(colsum_acc(dGd, 8L * H, (int)R, 4 * H, e->G + pd.bih, cs.part, cs.ctr, ws));
            HIPCHK(hipMemcpyAsync(e->G + pd.bhh, e->G + pd.bih, 4L * H * 4, hipMemcpyDeviceToDevice, ws));
        }
        CHK(dir_bucket(pd, wa, wh));
    }
    return dir_buckets ? 1 : 0;
}

// input gradient of one layer for the slab rows [r0, r0 + nr):  dX = dG . W_ih  (both directions accumulate)
int lstm_input_grad(ss_engine* e, LstmBlk& lb, int l, Slab dxi, long r0, long nr, const float* am, hipStream_t st) {
    if (l == 0 && lb.xf && dxi.p == lb.d_xc) {
        // compact: d_xc[block] = (sum of dG over the block's frames) . W_ih, one row per block of repeated input frames
        const int H = lb.H, In = lb.in_of(0);
        const long R8 = (long)e->curB * (e->curT / lb.xf);
        GemmDesc g{};
        g.A = {lb.dgs, 8L * H, 0, 0, 0};
        g.B = {lb.wcat[0], In, 0, 0, 0};
        g.b_pre = lb.wimg(0);
        g.C = lb.d_xc;
        g.ldc = In;
        g.M = (int)R8;
        g.N = lb.xcols > 0 ? lb.xcols : In;        // the speaker columns (last in the row, model.py:308-309) are an input: nobody reads their gradient
        g.K = 8 * H;
        g.batch = 1;
        g.flags = GEMM_TB | GEMM_ACCUM | (am ? GEMM_F16X2 : 0);
        g.amax_a = am;                              // the block sums are at most xf times the slab's maximum: inside the scale's headroom (256x)
        g.ksplit = 8;
        HIPCHK(hipMemsetAsync(g.C, 0, R8 * In * 4, st));
        PGEMM_ON(SS_PROF_DEC_DX, g, st);
        return 0;
    }
    // dX[r][k] = sum over both directions' 8H gate units of dG[r][n] * W_ih[n][k]: ONE GEMM against the stacked weights
    // (lstm_prep).  A narrow input (the decoder's 164 columns) is cut along the reduction so the launch still fills the chip.
    const int H = lb.H, In = lb.in_of(l), T = e->curT;
    const long TPr = T + 2 * HALO;
    GemmDesc g{};
    g.A = {lb.gates[l] + r0 * 8L * H, 8L * H, 0, 0, 0};
    g.B = {lb.wcat[l], In, 0, 0, 0};
    // (round 2's kernel measured SLOWER with the weight image in format v2 on this transposing-read operand -- 573 us per step with it, 532
    // without -- so only the 16-bit data path, whose image GEMM reads it, passes that image)
    // The pipelined k-loop (ss_tune("gemm_pipe"), round 5) brings that image in by LDS-DMA and gains from it; the split it saves is the same
    // split (fixed scale 16), so the result keeps its bits.
    g.b_pre = (e->img16() || (g_gemm_pipe && lb.big())) ? lb.wimg(l) : nullptr;
    const bool dg16 = e->img16() && &lb == &e->ld && l < 3 && ((e->bwd.dg16_written >> l) & 1);      // the gradient slab's bf16 image (backward recurrence's storing wave)
    if (dg16) g.a_pre = e->ioff(e->dg_img[l], r0 * 8L * H);
    g.C = dxi.p + r0 * dxi.ld;
    g.ldc = dxi.ld;
    g.M = (int)nr;
    g.N = In;
    g.K = 8 * H;
    g.batch = 1;
    g.flags = GEMM_TB | (am ? GEMM_F16X2 : 0);
    g.amax_a = am;                                  // gradient slab: measured scale; the stacked weights are O(1)
    g.ksplit = 1;
    const long tiles = (long)cdiv(g.M, 128) * cdiv(g.N, 64);
    if (tiles < 512 && g.K >= 1024 && dxi.ld == In) {          // split-K needs a zeroed, dense C
        g.ksplit = tiles < 256 ? 4 : 2;
        g.flags |= GEMM_ACCUM;
        HIPCHK(hipMemsetAsync(g.C, 0, nr * dxi.ld * 4, st));
    } else if (g_dx_batched && nr % TPr == 0 && r0 % TPr == 0 && T % 64 == 0) {
        // whole utterances: leave the halo rows out (nobody reads them in a gradient slab) -- one batch entry per
        // utterance, T rows each (T a multiple of 64), which at T = 128 also makes the 128 x 128 tiling come out at exactly 2 workgroups per CU for B = 64
        g.A = {lb.gates[l] + (r0 + HALO) * 8L * H, 8L * H, TPr * 8L * H, 0, 0};
        if (dg16) g.a_pre = e->ioff(e->dg_img[l], (r0 + HALO) * 8L * H);
        g.C = dxi.p + (r0 + HALO) * dxi.ld;
        g.cstride = TPr * dxi.ld;
        g.M = T;
        g.batch = (int)(nr / TPr);
        g.want = g_dx_batched == 2 ? 512 : 0;
    }
    PGEMM_ON(lb.big() ? SS_PROF_DEC_DX : SS_PROF_ENC_LSTM, g, st);
    return 0;
}

// What the gradient launches of layer l agree on: lstm_bwd launches the recurrence, lstm_late_weights possibly much later the GEMMs behind it
struct LayerGrads {
    float* am;                // fp16 x 2 gradient GEMMs need the slab's maximum, which only the persistent kernel measures
    bool bias_in_kernel;      // b_ih and b_hh gradients sit back to back in the arena (registration order): the persistent kernel fills both
    bool compact0;            // layer 0's input gradient dx is the compact slab: the recurrence also writes the block sums it is taken from
};
LayerGrads layer_grads(const ss_engine* e, const LstmBlk& lb, int l, Slab dx = {}) {
    const bool persist = lb.persist(e);
    const LstmDir &p0 = lb.pd[l * 2], &p1 = lb.pd[l * 2 + 1];
    return {(persist && g_bwd_f16x2 && lb.amax0 >= 0) ? e->amax + lb.amax0 + l : nullptr,
            persist && !g_deterministic && p0.bhh == p0.bih + 4L * lb.H && p1.bhh == p1.bih + 4L * lb.H, l == 0 && lb.xf && dx.p == lb.d_xc};
}

// d_top: gradient slab of the last layer's output [B,TP,2H]; x: forward input; dx: input-gradient view or null
// dx_ready (nullable): recorded on `s` right behind the input-gradient GEMM of layer 0, i.e. BEFORE this block's weight-gradient
// launches go to their branch stream.  A consumer that waits for it is not held up by whatever else shares a hardware queue with
// `s`: an event recorded later would sit in that queue behind every packet enqueued in between (measured: the conv trunk's
// backward idled 0.88 ms behind ~36 tiny weight-gradient launches of a sibling stream, profiles/r02/step_timeline_before.txt).
int lstm_late_weights(ss_engine* e, Backward& bw, LstmBlk& lb, Slab x, hipStream_t ws, int l_hi = -1, int l_lo = 0, DwRoute route = {});

// late_w: enqueue the recurrence chain and the input gradients only; the caller enqueues the block's weight gradients later
// (lstm_late_weights) -- after the phase's critical path -- on a stream it has ordered behind this chain.
int lstm_bwd(ss_engine* e, Backward& bw, LstmBlk& lb, const float* d_top, Slab x, Slab dx, hipStream_t s, hipEvent_t dx_ready = nullptr, bool late_w = false) {
    const int B = e->curB, T = e->curT, H = lb.H;
    const long TP = T + 2 * HALO, R = (long)B * TP;
    const float* dcur = d_top;
    const bool persist = lb.persist(e);
    // Decoder on the persistent kernels: its weight-gradient GEMMs are held back until the whole recurrence chain
    // (layer L-1 .. 0 and the input gradients between them) is through.  Co-scheduled they do not fill idle cycles:
    // they stretch the latency-bound recurrence steps and halve the rate of the input-gradient GEMMs on the critical
    // path (measured: chain 2.95 ms with the GEMMs beside it against 1.93 ms alone + 0.78 ms of GEMMs), whereas the
    // encoder backward that follows is a string of small launches they can run beside.
    const bool defer = lb.defers_weights(e) || late_w;
    // see ss_engine::wq_pool: only with the weight gradients deferred (their usual schedule), on the decoder, where XCDs stay free
    const bool xcd = defer && persist && &lb == &e->ld && g_xcd_dw && e->side && g_overlap && !g_deterministic && lstm_seq_free_xcds(B, H) >= 2;
    bool xcd_split[4] = {false, false, false, false};
    // 16-bit data path: the recurrence writes the gradient image itself and every weight-gradient GEMM of a layer is one image launch per
    // operand pair, so the WHOLE layer above goes out beside this layer's recurrence (work-queue form: 144 KB workgroups, one per free CU)
    const bool early16 = defer && persist && &lb == &e->ld && g_early_dw && e->img16() && e->side && g_overlap &&
                         !g_deterministic && !e->dp_on && e->wq_pool && lstm_seq_free_xcds(B, H) >= 2 && lb.out_img_valid;
    bool early_ready[4] = {false, false, false, false};
    for (int l = lb.L - 1; l >= 0; --l) {
        Slab xi = l == 0 ? x : Slab{lb.out[l - 1], lb.ow()};
        Slab dxi = l == 0 ? dx : Slab{lb.dmid[l & 1], lb.ow()};
        float* dG = lb.gates[l];
        hipStream_t ws = s;
        const auto [am, bias_in_kernel, compact0] = layer_grads(e, lb, l, dx);
        if (lb.big()) {
            // persistent: start state zeroed by backward_decoder
            if (persist) {
                // (a streaming pre-read of the activated gates and cell states beside the recurrence, as the forward does for its input
                // projections, was measured: no gain in the step; neither one recurrence ahead: +0.08 ms)
                const bool dg16 = e->img16() && &lb == &e->ld && l < 3 && e->dg_img[l];
                // only as bf16 when every reader takes the image: weight gradients and input gradient on the image GEMM (layers >= 1: aligned
                // shapes, both images present; layer 0: compact form -- dW_ih and dX from the block sums, dW_hh from the image), bias sums in the
                // kernel (not the deterministic mode's column sum over the fp32 slab), weight gradients deferred or not: same readers
                const bool skip32 = dg16 && bias_in_kernel && lb.out_img_valid && lb.out_img[l] &&
                                    (l == 0 ? compact0 : (lb.wimg(l) != nullptr && lb.in_of(l) % 64 == 0)) && H % 64 == 0;
                {
                    Prof pr(e, SS_PROF_REC_BWD, s, 2.0 * 2 * B * T * 4.0 * H * H);
                    HIPCHK(lstm_seq_bwd(dG, e->P + lb.pd[l * 2].whh, e->P + lb.pd[l * 2 + 1].whh, lb.px_l(l), dcur, lb.csave[l], lb.sync_b(l), B, T, H, s,
                                        {.sticky = e->sticky, .amax = am, .gbias_f = bias_in_kernel ? e->G + lb.pd[l * 2].bih : nullptr,
                                         .gbias_b = bias_in_kernel ? e->G + lb.pd[l * 2 + 1].bih : nullptr, .dgs = compact0 ? lb.dgs : nullptr,
                                         .xf = compact0 ? lb.xf : 0, .dimg = dg16 ? e->dg_img[l] : nullptr, .img_only = skip32,
                                         .hi_only = e->img16(), .state_zeroed = true}));      // hi_only: the 16-bit data path
                }
                if (dg16) e->bwd.dg16_written |= 1 << l;
                if (skip32) e->bwd.dg32_skipped |= 1 << l;
                if (early16) {
                    if (l + 1 < lb.L && early_ready[l + 1]) {
                        HIPCHK(seq_gate(lb.sync_b(l), B, H, e->side));          // dispatched once this recurrence's grid is resident
                        if (const int r = lstm_weight_grads(e, bw, lb, l + 1, Slab{lb.out[l], 2L * H}, am ? e->amax + lb.amax0 + l + 1 : nullptr, true, e->side, {.queue = true}); r < 0) return r;
                        e->bwd.dec_w_done |= 1 << (l + 1);
                    }
                    if (l >= 1 && l < 3 && dg16 && bias_in_kernel && lb.out_img[l] && lb.out_img[l - 1] && e->bwd.wq_next + 2 <= ss_engine::WQ_SLOTS) {
                        CHK(fork_join(e, s, e->side));        // layer l's slab and image are complete behind this point
                        early_ready[l] = true;
                        e->side_used = true;
                    }
                }
                // XCD-aware weight gradients: this recurrence leaves XCDs free, the layer above is through -- its W_ih gradient runs beside it
                if (xcd) {
                    if (l + 1 < lb.L && xcd_split[l + 1]) {
                        const float* am1 = e->amax + lb.amax0 + l + 1;
                        CHK(lstm_wih_gemm_queued(e, lb, l + 1, am1, lb.sync_b(l), e->side));
                    }
                    if (l >= 1 && lstm_wih_queue_ok(e, lb, l, am)) {       // this layer's turn comes beside the next recurrence: its image as soon as it is through
                        CHK(fork_join(e, s, e->side));
                        CHK(lstm_wih_split(e, lb, l, am, e->side));
                        xcd_split[l] = true;
                        e->side_used = true;
                    }
                }
            } else {      // one launch per time step
                const long half = 2L * (((B + 15) / 16) * 16) * 4 * H;
                HIPCHK(hipMemsetAsync(lb.gf, 0, 2 * half * 4, s));
                for (int st = 0; st < T; ++st)
                    HIPCHK(lstm_step_bwd(dG, lb.wfrag[l], lb.gf + (st & 1) * half, lb.gf + ((st & 1) ^ 1) * half, dcur, lb.csave[l], lb.dc, B, T, H, st, s));
            }
        } else {
            Prof pr(e, SS_PROF_ENC_REC, s);
            HIPCHK(lstm_small_bwd(dG, e->P + lb.pd[l * 2].whh, e->P + lb.pd[l * 2 + 1].whh, dcur, lb.csave[l], B, T, H, s));
        }
        // the pre-activation gradients of this layer are complete behind this point
        if (!defer && e->side && g_overlap) {
            // decoder: the side stream.  Encoder BLSTMs (a string of ~36 tiny split-K launches): the third branch stream, so
            // that they do not queue behind the decoder's weight gradients, which drain on the side stream until late
            ws = (!lb.big() && e->side3) ? e->side3 : e->side;
            if (s != ws) CHK(fork_join(e, s, ws));
            if (ws == e->side) e->side_used = true;
        }
        // input gradient first (the next layer's recurrence needs it)
        if (dxi.p) CHK(lstm_input_grad(e, lb, l, dxi, 0, R, am, s));
        if (l == 0 && dx_ready) HIPCHK(hipEventRecord(dx_ready, s));
        if (!defer)
            if (const int r = lstm_weight_grads(e, bw, lb, l, xi, am, bias_in_kernel, ws); r < 0) return r;
        dcur = dxi.p;
    }
    if (lb.defers_weights(e) && !late_w) {
        CHK(fork_join(e, s, e->side));
        e->side_used = true;
        CHK(lstm_late_weights(e, bw, lb, x, e->side));
    }
    return 0;
}

// all layers' weight / bias gradients of a block whose chain ran with deferred weights (the decoder's deferred batch; every block under late_w)
int lstm_late_weights(ss_engine* e, Backward& bw, LstmBlk& lb, Slab x, hipStream_t ws, int l_hi, int l_lo, DwRoute route) {
    const int H = lb.H;
    for (int l = l_hi < 0 ? lb.L - 1 : l_hi; l >= l_lo; --l) {       // layers l_hi .. l_lo (default: all, last first)
        if (&lb == &e->ld && ((e->bwd.dec_w_done >> l) & 1)) continue;        // went out beside a recurrence (early_dw)
        Slab xi = l == 0 ? x : Slab{lb.out[l - 1], lb.ow()};
        const LayerGrads lg = layer_grads(e, lb, l);
        route.part = (&lb == &e->ld && ((e->bwd.dec_ih_done >> l) & 1)) ? 2 : 0;
        const int dir_buckets = lstm_weight_grads(e, bw, lb, l, xi, lg.am, lg.bias_in_kernel, ws, route);
        if (dir_buckets < 0) return dir_buckets;
        // this layer's gradients (both directions: W_ih, W_hh, b_ih, b_hh -- contiguous in the arena) are final (unless each direction has
        // already gone out on its own)
        if (&lb == &e->ld && !dir_buckets) CHK(dp_bucket(e, lb.pd[l * 2].wih, lb.pd[l * 2 + 1].bhh + 4L * H - lb.pd[l * 2].wih, ws));
    }
    return 0;
}

// every gradient enqueued on the side stream so far is complete on `s` after this
int join_side(ss_engine* e, hipStream_t s) {
    if (e->side_used) {
        CHK(fork_join(e, e->side, s));
        e->side_used = false;
    }
    return 0;
}

// Scale of the fp16 x 2 split of every conv block's output, from its GroupNorm affine (kernels.h act_scales): 16 for any sane
// parameters, smaller powers of two when a large gamma could push an activation past fp16's range -- the contractions that read the
// block's output (as an image or as fp32) take the scale from these words, so no parameter magnitude makes a forward product overflow.
int act_scales_all(ss_engine* e, hipStream_t s) {
    ActScaleTable tb{};
    for (ConvBlk* cb : conv_blocks(*e)) {
        const int i = cb->scale_i;
        if (i < 0 || i >= ACT_SCALE_MAX) return fail("act_scales_all: bad slot");
        tb.gamma[i] = cb->Co ? e->P + cb->ga : e->P;
        tb.beta[i] = cb->Co ? e->P + cb->be : e->P;
        tb.C[i] = cb->Co;                  // an absent block (Generator_6 has no convolutions_1) has C = 0: bound 0, scale 16
        if (i + 1 > tb.n) tb.n = i + 1;
    }
    HIPCHK(act_scales(tb, e->curT, e->act_scale, s));
    return 0;
}

// ---- whole-model schedules ---------------------------------------------------------------------------------
// The forward's branch-stream work that nobody needs before the trunk is through (see forward_core, which decides where it is enqueued)
// dec_prep: the decoder's weight re-layouts ride along (every forward; not ss_g*_encode, which runs nothing of the decoder)
int forward_branch_work(ss_engine* e, const FusedForward& fused, const int* lens, hipStream_t b2, bool dec_prep) {
    PrepTable tb;
    tb.n = 0;
    tb.img_bf16 = e->img16();
    if (e->kind == SS_GENERATOR_3) CHK(lstm_prep(e, e->l1, tb, b2));
    CHK(lstm_prep(e, e->l2, tb, b2));
    CHK(lstm_prep(e, e->lt, tb, b2));
    if (dec_prep) CHK(lstm_prep(e, e->ld, tb, b2));
    HIPCHK(prep_run(tb, b2));
    if (fused.prezero) {     // nothing touches the gradient arena before the decoder backward; b2 is joined long before
        if (!fused.keep_grads) HIPCHK(hipMemsetAsync(e->G, 0, e->arena * 4, b2));
        HIPCHK(hipMemsetAsync(e->amax, 0, 16 * 4, b2));      // (the gradient slabs' maxima are per backward, accumulating or not)
        e->fwd.grads_zeroed = true;
        // the backward recurrences' group words and exchange tiles (nothing in the forward touches them): zeroed here, the backward
        // needs no fork / memset / join between the head's gradient and its first recurrence (two event hops on the critical path)
        if (e->ld.persist(e)) {
            HIPCHK(hipMemsetAsync(e->ld.zb, 0, e->ld.zb_bytes, b2));
            if (e->wq_pool) HIPCHK(hipMemsetAsync(e->wq_pool, 0, ss_engine::WQ_SLOTS * 16, b2));
            e->fwd.bwd_sync_zeroed = true;
        }
    }
    // fp16 x 2 products scale WEIGHTS by a fixed 16 (forward and gradient contractions alike, and the persistent recurrences' W_hh):
    // fine up to |w| < 4094.  Activations carry their own scale (act_scales_all) and gradients their measured one, so the only thing
    // left to refuse is a parameter beyond 2048 in magnitude, or a non-finite one: the step is then marked invalid (status RANGE)
    // instead of silently overflowing to inf.
    if ((g_fwd_f16x2 || g_bwd_f16x2) && e->precision == SS_PRECISION_F32 && e->sticky) HIPCHK(param_guard(e->P, e->arena, 2048.0f, e->sticky, b2));
    // Encoder_t (model.py:74-89)
    CHK(conv_block_fwd(e, e->ct, Slab{e->org, e->hp.dim_freq}, enc_t_out(e), b2, {.lens = lens}));
    CHK(lstm_fwd(e, e->lt, enc_t_out(e), b2, lens));
    return 0;
}

// The encoder part: everything up to the encoder BLSTMs' outputs, joined on `s` (plus, on the branch stream, the decoder's weight prep).
// dec_prep = false: without the decoder's weight prep (ss_g3_encode / ss_g6_encode).
int forward_encoders(ss_engine* e, bool training, const float* scales, const int* len_seg, int draw0, hipStream_t s, const FusedForward& fused, const int* lens,
                     bool dec_prep = true) {
    const int B = e->curB, T = e->curT;
    e->part_off = 0;           // split-K scratch: every launch of a step gets its own region; the previous step is through (stream order) when this one's first kernel runs
    const int CE = e->CE;
    const bool g3 = e->kind == SS_GENERATOR_3;
    const int S7 = e->plan[0].S;
    const int off2 = g3 ? e->hp.dim_enc : 0;       // first channel of the f0 stream inside the fused slab
    // Branches.  `s` carries the conv trunk; `b2` the per-step weight re-layouts followed by Encoder_t (depends on x_org
    // only); after the trunk the two encoder BLSTMs run side by side (`s`, `b1`).  Everything joins at the decoder input.
    const bool par = e->side && e->side2 && g_overlap;
    hipStream_t b1 = par ? e->side : s, b2 = par ? e->side2 : s;
    e->fwd.grads_zeroed = false;               // set again below when this forward belongs to a fused training step
    e->fwd.bwd_sync_zeroed = false;
    {   // every conv block's per-step weight re-layout (and the images of the packed weights) in one launch
        ConvPackTable pt{};
        pt.img_bf16 = e->img16();
        for (ConvBlk* cb : conv_blocks(*e)) {
            if (!cb->Co) continue;
            const bool img = cb->img_ok();
            pt.t[pt.n++] = {e->P + cb->w, cb->wf, cb->wb, img ? cb->wf_img : nullptr, img ? cb->wb_img : nullptr, cb->Co, cb->Ci, cb->Cp};
        }
        Prof pr(e, SS_PROF_PREP, s);
        HIPCHK(conv_pack_many(pt, s));
    }
    CHK(act_scales_all(e, s));             // before every branch forks: the scale words of the conv blocks' outputs
    if (par) CHK(fork_join(e, s, b2));
    if (fused.late_org) {
        const ss_hparams& hh = e->hp;
        HIPCHK(copy_rows(CRows::dense(fused.late_org, hh.dim_freq, T), Rows::slab(e->org, hh.dim_freq, T), B, T, hh.dim_freq, b2));
        if (fused.late_emb) HIPCHK(hipMemcpyAsync(e->emb, fused.late_emb, (long)B * hh.dim_spk_emb * 4, hipMemcpyDeviceToDevice, b2));
    }
    // Encoder_7's content (512 ch) and pitch (256 ch) stacks only share the random-resampling PLAN of each layer (model.py:199-206: one
    // warp applied to the concatenation), and the plans depend on the draws alone.  With branch streams the plans are computed first thing
    // on the branch stream and the two stacks run as independent chains on `s` and `b1` -- conv, GroupNorm, gather of their OWN columns --
    // down to their BLSTMs, instead of meeting before every gather.
    const bool indep = g3 && par;
    e->fwd.xf_img_valid = indep && training && e->xf_img[0] && ((e->precision == SS_PRECISION_F32 && g_fwd_f16x2) || (e->img16() && g_gn_gather));     // only fp16 x 2 / 16-bit-path GEMMs read images
    hipEvent_t plans = nullptr;
    if (indep && training) {
        for (int i = 0; i < 3; ++i)
            HIPCHK(interp_plan(e->plan[draw0 + i], scales + (long)(draw0 + i) * B * S7, len_seg + (long)(draw0 + i) * B * S7, nullptr,
                               e->hp.max_len_pad, B, b2));
        plans = e->ev[e->ev_next];
        e->ev_next = (e->ev_next + 1) & 15;
        HIPCHK(hipEventRecord(plans, b2));
    }
    if (indep) CHK(fork_join(e, s, b1));
    // The branch stream's work that nobody needs before the trunk is through: bias sums / W_ih stackings, start state of the
    // persistent recurrences, the gradient-arena memset, the parameter guard, and Encoder_t (model.py:74-89).  With g_prio_order it
    // is ENQUEUED behind the trunk's three layers (it still runs beside them: the host is far ahead of the GPU), so that on a shared
    // hardware queue it can never sit in front of trunk launches.
    const bool prio_fwd = par && g_prio_order;
    for (int i = 0; i < 3; ++i) {
        float* y = training ? e->act : e->xf[i];
        // Issue order matters: a cross-stream wait on ROCm holds for everything the other stream had been handed when
        // the WAIT was issued, not only up to the recorded event (measured: the trunk stalled ~250 us behind the tiny
        // launches of b2's work).  So: first trunk layer, and only then the rest of b2's work.
        if (i == 1 && !prio_fwd) CHK(forward_branch_work(e, fused, lens, b2, dec_prep));
        if (indep) {
            const float* im = (e->fwd.xf_img_valid && i > 0) ? e->xf_img[i - 1] : nullptr;
            const Slab x1 = trunk_in(e, 1, i, im), x2 = trunk_in(e, 2, i, im);
            if (training && g_gn_gather) {       // conv -> [GroupNorm + ReLU + gather] per stack: the normalised slab is never written
                float* gi = (e->fwd.xf_img_valid && e->xf_img[i]) ? e->ioff(e->xf_img[i], HALO * CE) : nullptr;
                const InterpPlan* pl = &e->plan[draw0 + i];
                const Rows gy = Rows::slab(e->xf[i], CE, T);
                hipEvent_t ready = i == 0 ? plans : nullptr;
                CHK(conv_block_fwd(e, e->c2[i], x2, Slab{y + off2, CE}, b1,
                                   {.gather = pl, .gy = gy.col(off2), .gy_img = gi ? e->ioff(gi, off2) : nullptr, .gather_ready = ready}));
                CHK(conv_block_fwd(e, e->c1[i], x1, Slab{y, CE}, s, {.gather = pl, .gy = gy, .gy_img = gi, .gather_ready = ready}));
                continue;
            }
            CHK(conv_block_fwd(e, e->c2[i], x2, Slab{y + off2, CE}, b1, {.lens = lens}));
            CHK(conv_block_fwd(e, e->c1[i], x1, Slab{y, CE}, s, {.lens = lens}));
            if (training) {
                InterpPlan& pl = e->plan[draw0 + i];
                if (i == 0) {
                    HIPCHK(hipStreamWaitEvent(b1, plans, 0));
                    HIPCHK(hipStreamWaitEvent(s, plans, 0));
                }
                float* gi = (e->fwd.xf_img_valid && !e->img16() && e->xf_img[i]) ? e->xf_img[i] + HALO * CE : nullptr;      // (the separate gather writes format-v2 images only)
                const Rows a = Rows::slab(e->act, CE, T), xf = Rows::slab(e->xf[i], CE, T);
                HIPCHK(interp_gather(pl, a.col(off2), xf.col(off2), CE - off2, B, b1, gi ? gi + off2 : nullptr, e->act_scale + e->c2[i].scale_i));
                HIPCHK(interp_gather(pl, a, xf, off2, B, s, gi, e->act_scale + e->c1[i].scale_i));
            }
            continue;
        }
        // one chain on `s` (Generator_6's single stack; Generator_3 without branch streams)
        if (g3) CHK(conv_block_fwd(e, e->c1[i], trunk_in(e, 1, i), Slab{y, CE}, s, {.lens = lens}));
        CHK(conv_block_fwd(e, e->c2[i], trunk_in(e, 2, i), Slab{y + off2, CE}, s, {.lens = lens}));
        if (training) {
            // one warp for both streams (model.py:202-206), len_seq = max_len_pad for every utterance (:105,157,203)
            InterpPlan& pl = e->plan[draw0 + i];
            HIPCHK(interp_plan(pl, scales + (long)(draw0 + i) * B * S7, len_seg + (long)(draw0 + i) * B * S7, nullptr,
                               e->hp.max_len_pad, B, s));
            HIPCHK(interp_gather(pl, Rows::slab(e->act, CE, T), Rows::slab(e->xf[i], CE, T), CE, B, s));
        }
    }
    if (prio_fwd) CHK(forward_branch_work(e, fused, lens, b2, dec_prep));
    if (par) {
        CHK(fork_join(e, b2, s));                  // bias sums of every block are ready (and Encoder_t is done)
        if (indep) CHK(fork_join(e, b2, b1));      // the pitch chain does not wait for the content chain
        else CHK(fork_join(e, s, b1));
    }
    CHK(lstm_fwd(e, e->l2, trunk_in(e, 2, 3), b1, lens));
    if (g3) CHK(lstm_fwd(e, e->l1, trunk_in(e, 1, 3), s, lens));
    if (par) CHK(fork_join(e, b1, s));
    return 0;
}

// Codes and speaker rows a caller hands in (ss_g3_decode / ss_g6_decode) in place of the encoder slabs: dense fp32, [B, T / f_i, 2 H_i] in the
// column order of code_srcs, c_trg [B, dim_spk_emb] (Generator_3)
struct CallerCodes {
    const float* codes[3];
    const float* c_trg;
};

// The decoder part, on `s`: the decoder input (from the encoder slabs, or from `from`), the decoder BLSTM and the head.
int forward_decoder(ss_engine* e, hipStream_t s, const int* lens, const CallerCodes* from = nullptr) {
    const int B = e->curB, T = e->curT;
    const long TP = T + 2 * HALO;
    const bool g3 = e->kind == SS_GENERATOR_3;
    // decoder input (model.py:301-309 / 341-347)
    CodeSrc src[3];
    const int n = code_srcs(e, src);
    const ss_hparams& h = e->hp;
    const float* emb = g3 ? (from ? from->c_trg : e->emb) : nullptr;       // Generator_3: the speaker embedding fills the columns behind the three codes
    const int emb_dim = g3 ? h.dim_spk_emb : 0, emb_col = g3 ? 2 * h.dim_neck + 2 * h.dim_neck_2 + 2 * h.dim_neck_3 : e->dec_in_dim;
    if (from) {
        CodeIn in[3];
        for (int i = 0; i < n; ++i) in[i] = {from->codes[i], src[i].H, src[i].freq, src[i].col};
        if (dec_compact(e)) HIPCHK(dec_in_from_codes(in, n, emb, emb_dim, emb_col, e->ld.xc, e->dec_in_dim, B, T, e->ld.xf, s, lens));
        else HIPCHK(dec_in_from_codes(in, n, emb, emb_dim, emb_col, e->dec_in, e->dec_in_dim, B, T, 0, s, lens));
    } else if (dec_compact(e)) HIPCHK(build_dec_in_compact(src, n, emb, emb_dim, emb_col, e->ld.xc, e->dec_in_dim, B, T, e->ld.xf, s));
    else HIPCHK(build_dec_in(src, n, emb, emb_dim, emb_col, e->dec_in, e->dec_in_dim, B, T, s));
    CHK(lstm_fwd(e, e->ld, dec_x(e), s, lens));
    // LinearNorm head (model.py:253 / 277)
    const long HD = 2L * e->ld.H;
    GemmDesc d{};
    d.A = {e->ld.out[e->ld.L - 1] + HALO * HD, HD, TP * HD, 0, 0};
    if (e->ld.out_img_valid) d.a_pre = e->ioff(e->ld.out_img[e->ld.L - 1], HALO * HD);
    d.B = {e->P + e->head_w, HD, 0, 0, 0};
    d.C = e->out_slab + HALO * e->head_out;
    d.ldc = e->head_out;
    d.cstride = TP * e->head_out;
    d.bias = e->P + e->head_b;
    d.M = T;
    d.N = e->head_out;
    d.K = (int)HD;
    d.batch = B;
    d.ksplit = 1;
    flatten_rows(d, B, T);
    PGEMM_FWD_ON(SS_PROF_HEAD, d, s);
    return 0;
}

// Encoder_7 (G3) / Encoder_6 (G6) trunk + their LSTMs, Encoder_t, decoder, head.  Inputs already in in_mel/in_f0/org/emb.
// lens (nullable; eval mode only): per-row lengths of a ragged batch (device i32[B], caller-owned, read in stream order).  The staging
// of the inputs has zeroed the padded frames; here every GroupNorm and every recurrence takes the lengths, everything else is row-wise.
int forward_core(ss_engine* e, bool training, const float* scales, const int* len_seg, int draw0, hipStream_t s, const FusedForward& fused = {}, const int* lens = nullptr) {
    CHK(forward_encoders(e, training, scales, len_seg, draw0, s, fused, lens));
    CHK(forward_decoder(e, s, lens));
    e->fwd.training = training;
    e->fwd.enc_plan0 = draw0;
    e->fwd.ragged = lens != nullptr;
    e->fwd.decode = false;
    e->fwd.have = true;
    return 0;
}

// gradient of the loss w.r.t. the head output is in d_out_slab (halo rows zero)
// weight and bias gradient of the LinearNorm head from d_out_slab and the last decoder layer's output (both untouched by the backward chain)
int head_weight_grads(ss_engine* e, hipStream_t st) {
    const long TP = e->curT + 2 * HALO, R = (long)e->curB * TP;
    const long HD = 2L * e->ld.H;
    const float* h3 = e->ld.out[e->ld.L - 1];
    GemmDesc a{};
    a.A = {e->d_out_slab, e->head_out, 0, 0, 0};
    a.B = {h3, HD, 0, 0, 0};
    a.C = e->G + e->head_w;
    a.ldc = HD;
    a.M = e->head_out;
    a.N = (int)HD;
    a.K = (int)R;
    a.batch = 1;
    a.flags = GEMM_TA | GEMM_TB | GEMM_ACCUM;
    a.ksplit = pick_ksplit(a.M, a.N, a.K);
    PGEMM_ON(SS_PROF_HEAD, a, st);
    const ColScratch cs = colsum_scratch(e, e->head_out);
    HIPCHK(colsum_acc(e->d_out_slab, e->head_out, (int)R, e->head_out, e->G + e->head_b, cs.part, cs.ctr, st));
    CHK(dp_bucket(e, e->head_w, e->status_off - e->head_w, st));       // (the status slot behind it rides the step's last bucket)
    return 0;
}

// late: only the critical chain is enqueued here (head input gradient, recurrences, input gradients); the decoder's and the head's
// weight gradients are enqueued by backward_encoder behind ITS critical path, ordered after the chain through ev_join[1]
int backward_decoder(ss_engine* e, Backward& bw, hipStream_t s, bool late = false) {
    if (!e->fwd.have) return fail("backward without a preceding forward");
    const int B = e->curB, T = e->curT;
    const long TP = T + 2 * HALO, R = (long)B * TP;
    if (!e->fwd.grads_zeroed) {
        if (!bw.accumulate) HIPCHK(hipMemsetAsync(e->G, 0, e->arena * 4, s));
        HIPCHK(hipMemsetAsync(e->amax, 0, 16 * 4, s));
    }
    e->fwd.grads_zeroed = false;
    e->bwd_accumulate = bw.accumulate;
    e->accum_count = bw.accumulate ? e->accum_count + 1 : 1;
    // fragment-major W_hh^T of the decoder recurrences (overwrites the forward layout, no longer needed), beside the head
    const bool prezeroed = e->fwd.bwd_sync_zeroed && e->ld.persist(e);       // the fused step's forward has done it on its branch stream
    e->fwd.bwd_sync_zeroed = false;
    const bool par = e->side2 && g_overlap && !prezeroed;
    hipStream_t b2 = par ? e->side2 : s;
    if (par) CHK(fork_join(e, s, b2));
    e->bwd = {};
    if (e->ld.big() && !prezeroed) {
        if (e->ld.persist(e)) {
            // the group counters of every layer and their exchange tiles (tags start at 0)
            HIPCHK(hipMemsetAsync(e->ld.zb, 0, e->ld.zb_bytes, b2));
            if (e->wq_pool) HIPCHK(hipMemsetAsync(e->wq_pool, 0, ss_engine::WQ_SLOTS * 16, b2));
        } else {
            for (int l = 0; l < e->ld.L; ++l)
                HIPCHK(lstm_pack_w(e->P + e->ld.pd[l * 2].whh, e->P + e->ld.pd[l * 2 + 1].whh, e->ld.wfrag[l], e->ld.H, 1, b2));
        }
    }
    // head.  Only its input gradient is on the critical path; when the decoder's weight gradients are deferred to the side
    // stream (lstm_bwd), the head's weight / bias gradients go with them instead of running in front of the first recurrence.
    const long HD = 2L * e->ld.H;
    const bool defer_head = e->ld.defers_weights(e);
    late = late && defer_head;
    bw.dec_w_pending = late;
    if (!defer_head) CHK(head_weight_grads(e, s));
    GemmDesc g{};
    g.A = {e->d_out_slab, e->head_out, 0, 0, 0};
    g.B = {e->P + e->head_w, HD, 0, 0, 0};
    g.C = e->d_top;
    g.ldc = HD;
    g.M = (int)R;
    g.N = (int)HD;
    g.K = e->head_out;
    g.batch = 1;
    g.flags = GEMM_TB;
    g.ksplit = 1;
    PGEMM_ON(SS_PROF_HEAD, g, s);
    if (par) CHK(fork_join(e, b2, s));
    CHK(lstm_bwd(e, bw, e->ld, e->d_top, dec_x(e), dec_dx(e), s, nullptr, late));
    if (late) HIPCHK(hipEventRecord(e->ev_join[1], s));          // the chain is through: what the side stream's batch waits for
    else if (defer_head) CHK(head_weight_grads(e, e->side));      // behind the decoder's weight gradients, ordered after the chain by lstm_bwd's fork
                                                            // (measured: on the third branch stream instead 6.395 vs 6.365 ms)
    // every persistent recurrence of the step is behind this point: publish this rank's status into the gradient arena's
    // status slot (part of the decoder bucket, so a data-parallel all-reduce carries it to every rank's Adam kernel)
    if (e->sticky) HIPCHK(status_publish(e->sticky, e->G + e->status_off, s));
    return 0;
}

// The early range's optimiser work (Backward::adam_early: one GPU, Adam inside the step) on the side stream, right behind the last of
// the decoder's and the head's weight gradients
int early_update(ss_engine* e, Backward& bw) {
    if (!bw.adam_early || e->dp_on || !e->Mm || !e->Vv) return 0;
    // every persistent recurrence and the parameter guard ran before the event this stream waited for: the status word is final
    const long from = ss_grad_split(e);
    if (e->clip_max > 0.0f) {
        // clipping: no element may be updated before the norm of the whole arena is known -- this range's share of the sum
        // of squares takes the early update's place beside the encoder backward (adam_enqueue finalises)
        if (from == clip_split(e)) {
            Prof pr(e, SS_PROF_ADAM, e->side);
            HIPCHK(grad_sumsq(e->G, e->segs, from, e->status_off, e->clip_part + clip_wgs_lo(e), e->side));
            bw.clip_early_from = from;
        }
    } else if (from % 4 == 0 && from < e->arena) {
        const AdamExt x = opt_ext(e);
        if (x.on()) {         // decay and the average ride in the same launch; the step's ONE prepare sets their factors for both ranges
            HIPCHK(adam_prepare_ext(e->adam, x, e->sticky, nullptr, e->side, lr_sched(e)));
            Prof pr(e, SS_PROF_ADAM, e->side);
            HIPCHK(adam_range_ext(e->P, e->G, e->Mm, e->Vv, from, e->arena, e->adam, bw.adam_gs, nullptr, x, e->side));
        } else {
            HIPCHK(adam_prepare(e->adam, e->sticky, nullptr, e->side, lr_sched(e)));
            Prof pr(e, SS_PROF_ADAM, e->side);
            HIPCHK(adam_range(e->P + from, e->G + from, e->Mm + from, e->Vv + from, e->arena - from, e->adam, bw.adam_gs, e->side));
        }
        bw.adam_early_from = from;
    }
    return 0;
}

// backward_decoder(late) left the decoder's and the head's weight gradients to backward_encoder, which enqueues them in pieces
struct DecLate {
    int next = -1;                                   // next decoder layer whose weight gradients are still to be enqueued
    hipStream_t other[2] = {nullptr, nullptr};       // streams other than the side stream that carry some of them (tail split)
    bool main_used = false;                          // ... and the main stream, kept apart: the caller's stream may be the NULL stream
    hipStream_t main_s = nullptr;
};
// the decoder's layers dl.next .. l_lo and, with its layer 0, the head's weight gradients, behind the decoder chain (ev_join[1]): on ws
// (null: the side stream), the reverse direction's dW_ih / dW_hh on over_ih / over_hh where given (DwRoute).  on_main (nullable): on THAT
// stream instead of ws -- a pointer, because the main stream is the caller's and PyTorch's default stream is the null handle, which `ws`
// reads as "the side stream" (dec_tail_split = 3 silently ran as 0 for layer 0 and the head until tests/test_gpu_schedule_knobs.py looked)
int dec_late(ss_engine* e, Backward& bw, DecLate& dl, int l_lo, hipStream_t ws = nullptr, hipStream_t over_ih = nullptr, hipStream_t over_hh = nullptr,
             const hipStream_t* on_main = nullptr) {
    if (dl.next < l_lo) return 0;
    if (on_main) ws = *on_main;
    else if (!ws) ws = e->side;
    auto behind_chain = [&](hipStream_t o) -> int {      // a stream other than the side stream: noted for the join at the end
        if (dl.other[0] != o && dl.other[1] != o) dl.other[dl.other[0] ? 1 : 0] = o;
        HIPCHK(hipStreamWaitEvent(o, e->ev_join[1], 0));
        return 0;
    };
    for (hipStream_t o : {over_ih, over_hh})
        if (o && o != ws && o != e->side) CHK(behind_chain(o));
    if (dl.next == e->ld.L - 1) HIPCHK(hipStreamWaitEvent(e->side, e->ev_join[1], 0));
    if (on_main) {
        dl.main_used = true;
        dl.main_s = ws;
        HIPCHK(hipStreamWaitEvent(ws, e->ev_join[1], 0));
    } else if (ws != e->side) CHK(behind_chain(ws));
    CHK(lstm_late_weights(e, bw, e->ld, dec_x(e), ws, dl.next, l_lo, {.over_ih = over_ih, .over_hh = over_hh}));
    dl.next = l_lo - 1;
    if (l_lo == 0) {
        CHK(head_weight_grads(e, ws));
        bw.dec_w_pending = false;
        for (hipStream_t o : dl.other)
            if (o) CHK(fork_join(e, o, e->side));      // one join for the end of the step; the early optimiser update reads what they wrote
        if (dl.main_used) CHK(fork_join(e, dl.main_s, e->side));
        CHK(early_update(e, bw));
    }
    e->side_used = true;
    return 0;
}

// Tail split (g_dec_tail_split = m, one-GPU step): on the side stream alone the decoder's twelve weight-gradient GEMMs end ~450 us after every
// other stream -- its last layers and the head go behind streams that end early instead.  s: main, b2: pitch, b3: third; null: the side stream
struct TailSplit {
    hipStream_t l2_hh, l1, l1_ih, l1_hh, l0;      // layer 2's reverse dW_hh; layer 1, its reverse dW_ih and dW_hh; layer 0 + head
    bool l0_main;                                 // layer 0 + head on the main stream (whose handle may be null: not expressible in l0)
};
TailSplit dec_tail_split(int m, hipStream_t b2, hipStream_t b3) {
    TailSplit t{};
    //                        m:        1        2        3    4        5        6
    t.l1 = m == 4 || m == 5 ? b3 : (m == 6 ? b2 : nullptr);
    t.l0 = m == 1 || m == 5 ? b2 : (m == 2 || m == 6 || m >= 7 ? b3 : nullptr);
    t.l0_main = m == 3;
    // 7-9: as 2, and layer 1's reverse direction leaves the side stream as well: 7: dW_ih -> third, dW_hh -> pitch stream; 8: both -> third; 9: dW_hh -> third
    t.l1_ih = m == 7 || m == 8 ? b3 : nullptr;
    t.l1_hh = m == 7 ? b2 : (m == 8 || m == 9 || m == 10 ? b3 : nullptr);
    t.l2_hh = m == 10 ? b3 : nullptr;      // 10: as 9, and layer 2's reverse dW_hh -> third as well
    return t;
}

// everything below the decoder input: code gradients, encoder BLSTMs, conv trunks.  Touches only gradient-arena
// offsets below the decoder's, so a data-parallel caller can all-reduce the decoder range meanwhile.
int backward_encoder(ss_engine* e, Backward& bw, hipStream_t s) {
    bw.unpack_later = !e->dp_on;       // (data parallel: a trunk layer's bucket leaves right behind its block)
    const int B = e->curB, T = e->curT;
    const long TP = T + 2 * HALO, R = (long)B * TP;
    const int CE = e->CE;
    const bool g3 = e->kind == SS_GENERATOR_3;
    const bool training = e->fwd.training;
    const ss_hparams& h = e->hp;
    // ---- phase 1: code gradients and forks
    CodeSrc src[3];
    const int n = code_srcs(e, src);
    if (dec_compact(e)) HIPCHK(dec_in_grad_compact(src, n, e->ld.d_xc, e->dec_in_dim, B, T, e->ld.xf, s));
    else HIPCHK(dec_in_grad(src, n, e->d_dec_in, e->dec_in_dim, B, T, s));
    const int off2 = g3 ? h.dim_enc : 0;
    // Three independent branches below the decoder input: lstm_1 (on `s`), lstm_2 (`b2`; writes the other columns of d_xf)
    // and Encoder_t (`b3`; joins at the end).  Their weight-gradient GEMMs share the side stream.
    const bool par = e->side2 && e->side3 && g_overlap;
    hipStream_t b2 = par ? e->side2 : s, b3 = par ? e->side3 : s;
    // prio: critical path first (g_prio_order) -- lstm_2's and lstm_1's chains and the conv trunk are enqueued before anything that only
    // has to be done by the end of the step; the latter (decoder + head weight gradients, the encoder BLSTMs' weight gradients,
    // Encoder_t's whole backward) follow below, each ordered behind its producer by an event that was recorded when the producer
    // was enqueued.
    const bool prio = par && g_prio_order && !e->l2.big() && !e->l1.big() && !e->lt.big();
    bw.wg_defer = prio;        // the small blocks' weight gradients of this backward: collected, launched once on b3 below (prio schedule)
    if (par) {
        if (prio) HIPCHK(hipEventRecord(e->ev_join[2], s));                 // dec_in_grad done: what Encoder_t's backward needs
        CHK(fork_join(e, s, b2));
        if (!prio) CHK(fork_join(e, s, b3));
    }
    CHK(zero_conv_grads(e, b2));                   // long done when the first conv weight gradient starts (b2 joins s, b3 forks after)
    if (prio && b3 != b2) CHK(fork_join(e, b2, b3));      // Encoder_t's conv weight gradient accumulates into its zeroed image before b3 sees lstm_2's event
    if (par && !prio) CHK(fork_join(e, b2, b3));
    // ---- phase 2: encoder BLSTM chains -> gradient of the last fused slab
    const bool early = par && !e->l2.big();         // the join event of the lstm_2 branch is taken as soon as its last kernel is queued
    CHK(lstm_bwd(e, bw, e->l2, e->d_o2, trunk_in(e, 2, 3), Slab{e->d_xf + off2, CE}, b2, (early || prio) ? e->ev_join[0] : nullptr, prio));
    if (g3) {
        CHK(lstm_bwd(e, bw, e->l1, e->d_o1, trunk_in(e, 1, 3), Slab{e->d_xf, CE}, s, nullptr, prio));
        if (prio) HIPCHK(hipEventRecord(e->ev_join[3], s));                 // lstm_1's chain done: its weight gradients may start
    }
    if (!prio) {
        // Encoder_t
        CHK(lstm_bwd(e, bw, e->lt, e->d_ot, enc_t_out(e), Slab{e->d_act_t, h.dim_enc_2}, b3));
        CHK(conv_block_bwd(e, bw, e->ct, Slab{e->d_act_t, h.dim_enc_2}, Slab{e->org, h.dim_freq}, Slab{nullptr, 0}, b3));
    }
    if (early || prio) HIPCHK(hipStreamWaitEvent(s, e->ev_join[0], 0));
    else if (par) CHK(fork_join(e, b2, s));
    // ---- phase 3: conv trunk, last layer first (data parallel: the decoder's late weight gradients between its layers)
    DecLate dl{bw.dec_w_pending ? e->ld.L - 1 : -1};
    // Data parallel: the communication stream executes its collectives in the order they are ENQUEUED, so the buckets are enqueued in the
    // order they become final -- decoder layer L-1, trunk layer 2, decoder layer L-2, trunk layer 1, the rest of the decoder + head --
    // instead of every decoder bucket in front of (or behind) every trunk bucket.  (One GPU: the decoder's weight gradients stay behind
    // the trunk in enqueue order, see prio_order.)
    if (e->dp_on) CHK(dec_late(e, bw, dl, e->ld.L - 1));
    // Encoder_7's content (512 ch) and pitch (256 ch) stacks are independent chains in the backward as in the forward (forward_core):
    // each block's output gradient comes from its own BLSTM / its own upper block, its input gradient goes to its own lower block, and the two
    // write disjoint columns of the shared slabs.  The pitch chain never leaves the stream lstm_2's backward ran on (second branch stream), beside the
    // content stack on the main stream, through all three layers (round 3 did this for layer 0 only): 64 x 128 unchanged (that phase is
    // throughput-bound), 32 x 128 bf16 3.16 -> 3.02 ms, 16 x 128 fp32 3.44 -> 3.29.  (Measured and rejected beside it: each block's weight-gradient
    // GEMM on the side stream beside its input-gradient GEMM -- +8 % at B <= 32: the two cross-stream event hops per block cost more than the
    // overlap gains.)
    // Data parallel: that stream carries the collectives, so the pitch chain takes the third branch stream instead (behind the event of lstm_2's
    // input gradient; Encoder_t's backward and the fused weight gradients queue behind it there).
    const bool chain_par = training && g3 && par && g_gn_gather && (!e->dp_on || (prio && b3 != s && b3 != b2));
    hipStream_t cs = e->dp_on ? b3 : b2;
    if (chain_par && e->dp_on) HIPCHK(hipStreamWaitEvent(b3, e->ev_join[0], 0));      // d_xf's pitch columns (lstm_2's input gradient) and the zeroed conv images
    // weight gradients off the dependent chain (g_conv_dw_off): Generator_6's single chain, the second branch stream is idle behind lstm's backward
    const bool dw_off = g_conv_dw_off == 1 && training && !g3 && par && prio && !e->dp_on && g_gn_gather && bw.unpack_later && b2 != s && e->d_act_l[0] && e->d_act_l[1];
    hipStream_t dw_s = dw_off ? b2 : nullptr;
    for (int i = 2; i >= 0; --i) {
        float* dy = e->d_xf;
        // training: the adjoint of the layer's resampling, d_xf -> d_act; fused into each block's GroupNorm backward (g_gn_gather) or as a pass of its own
        const InterpPlan* sc = (training && g_gn_gather) ? &e->plan[e->fwd.enc_plan0 + i] : nullptr;
        const CRows sc_src = CRows::slab(e->d_xf, CE, T);
        if (training) {
            if (!sc) HIPCHK(interp_scatter(e->plan[e->fwd.enc_plan0 + i], sc_src, Rows::slab(e->d_act, CE, T), CE, B, s));
            dy = (dw_off && i > 0) ? e->d_act_l[i - 1] : e->d_act;
        }
        // input gradients of layer i become d_xf (the gradient of xf[i-1]); dy is consumed before it is overwritten
        // only when dy != d_xf, so in eval mode the input gradient goes through d_act instead.
        float* dxbuf = training ? e->d_xf : e->d_act;
        // the resampled activations also exist as pre-split images when the forward's gathers wrote them (training, independent trunk chains)
        const float* bim = (training && e->fwd.xf_img_valid && i > 0) ? e->xf_img[i - 1] : nullptr;
        if (!chain_par && i == 0 && g3 && par && !e->dp_on) CHK(fork_join(e, s, b2));      // tail_par below: the pitch block's stream forks BEFORE the content block is enqueued
        if (g3) CHK(conv_block_bwd(e, bw, e->c1[i], Slab{dy, CE}, trunk_in(e, 1, i, bim), i > 0 ? Slab{dxbuf, CE} : Slab{}, s, {.scatter = sc, .src = sc_src}));
        // Layer 0 is the step's tail: the decoder's weight gradients are through by then, and each of its two weight-gradient GEMMs alone
        // fills half the chip's workgroup slots -- the pitch block runs on the second branch stream beside the content block.  (Not under
        // data parallelism, where that stream carries the collectives.)
        const bool tail_par = chain_par || (i == 0 && g3 && par && !e->dp_on);
        hipStream_t s2 = tail_par ? (chain_par ? cs : b2) : s;
        CHK(conv_block_bwd(e, bw, e->c2[i], Slab{dy + off2, CE}, trunk_in(e, 2, i, bim), i > 0 ? Slab{dxbuf + off2, CE} : Slab{}, s2,
                           {.scatter = sc, .src = sc_src.col(off2), .dws = (dw_off && i > 0) ? dw_s : nullptr}));
        if (tail_par && (!chain_par || (i == 0 && !e->dp_on))) CHK(fork_join(e, b2, s));      // (chain_par: the two chains meet once, behind layer 0; data parallel: where the third branch stream joins below)
        if (i > 0) {           // the two wide layers' parameters (weight, bias, GroupNorm affine: contiguous) are final; layer 0 rides the last bucket
            if (g3) CHK(dp_bucket(e, e->c1[i].w, e->c1[i].be + e->c1[i].Co - e->c1[i].w, s));
            CHK(dp_bucket(e, e->c2[i].w, e->c2[i].be + e->c2[i].Co - e->c2[i].w, s2));
            if (e->dp_on) CHK(dec_late(e, bw, dl, i == 2 ? (e->ld.L >= 3 ? e->ld.L - 2 : 0) : 0));      // next decoder layer(s) behind this trunk layer's buckets
        }
        if (!training && i > 0) {
            // eval mode has no resampling between layers: the next (lower) layer reads its output gradient from d_xf
            HIPCHK(hipMemcpyAsync(e->d_xf, e->d_act, R * CE * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    // ---- phase 4: everything that only has to be finished by the end of the step
    if (!e->dp_on && prio && chain_par && bw.dec_w_pending && e->ld.L == 3 && g_dec_tail_split) {
        const TailSplit t = dec_tail_split(g_dec_tail_split, b2, b3);
        CHK(dec_late(e, bw, dl, 2, nullptr, nullptr, t.l2_hh));
        CHK(dec_late(e, bw, dl, 1, t.l1, t.l1_ih, t.l1_hh));
        CHK(dec_late(e, bw, dl, 0, t.l0, nullptr, nullptr, t.l0_main ? &s : nullptr));
        if (t.l1 == b2 || t.l0 == b2 || t.l1_hh == b2) CHK(fork_join(e, b2, s));
    }
    CHK(dec_late(e, bw, dl, 0));
    if (prio) {
        // Encoder_t's backward first: its input (d_ot from dec_in_grad) is the earliest thing this stream waits for, and it is a dependent chain of
        // five launches; the BLSTMs' weight gradients (all three blocks: ONE fused launch) only have to be done by the end of the step
        // (Generator_6 32 x 192 bf16 2.26 -> 2.23 ms, 16 x 128 3.20 -> 3.18 against the BLSTMs' weight gradients in front; headline unchanged)
        HIPCHK(hipStreamWaitEvent(b3, e->ev_join[2], 0));                   // d_ot from dec_in_grad
        CHK(lstm_bwd(e, bw, e->lt, e->d_ot, enc_t_out(e), Slab{e->d_act_t, h.dim_enc_2}, b3));
        CHK(conv_block_bwd(e, bw, e->ct, Slab{e->d_act_t, h.dim_enc_2}, Slab{e->org, h.dim_freq}, Slab{nullptr, 0}, b3));
        HIPCHK(hipStreamWaitEvent(b3, e->ev_join[0], 0));                   // lstm_2's pre-activation gradients (and the zeroed conv images)
        CHK(lstm_late_weights(e, bw, e->l2, trunk_in(e, 2, 3), b3));
        if (g3) {
            HIPCHK(hipStreamWaitEvent(b3, e->ev_join[3], 0));
            CHK(lstm_late_weights(e, bw, e->l1, trunk_in(e, 1, 3), b3));
        }
        CHK(wgrad_flush(e, bw, b3));               // Encoder_t's, lstm_2's and both layers of lstm_1's: one launch
    }
    // ---- phase 5: joins
    if (par) CHK(fork_join(e, b3, s));
    if (dw_off) CHK(fork_join(e, dw_s, s));
    CHK(join_side(e, s));
    if (bw.unpack.n) HIPCHK(conv_unpack_grads(bw.unpack, s, bw.accumulate));
    return 0;
}

int backward_core(ss_engine* e, Backward& bw, hipStream_t s) {
    CHK(backward_decoder(e, bw, s, g_prio_order));
    return backward_encoder(e, bw, s);
}

// Generator_3's speaker embedding enters decoder layer 0 as the last dim_spk_emb columns of every frame's input row (model.py:308-309):
// dc[b][j] = sum_t sum_g dG0[b][t][g] * W_ih0[g][xcols + j] over both directions' gate rows.  dG0 summed over time first -- from the
// block sums of the compact layer 0, or from the layer's full pre-activation gradient slab -- then contracted with the 82 columns.
int speaker_input_grad(ss_engine* e, float* dc, hipStream_t s) {
    LstmBlk& lb = e->ld;
    const int B = e->curB, T = e->curT, H = lb.H;
    const long TP = T + 2 * HALO;
    const bool compact = dec_compact(e);
    const float* dg = compact ? lb.dgs : lb.gates[0] + HALO * 8L * H;
    const long bs = compact ? (long)(T / lb.xf) * 8 * H : TP * 8L * H;
    const int rows = compact ? T / lb.xf : T;
    if (!compact && (e->bwd.dg32_skipped & 1)) return fail("internal: decoder layer 0's fp32 gradient slab was not written");
    HIPCHK(spk_grad(dg, 8L * H, bs, rows, e->P + lb.pd[0].wih, e->P + lb.pd[1].wih, lb.In, lb.xcols, 4 * H, e->hp.dim_spk_emb, dc, B, s));
    return 0;
}

}  // namespace

// ================================================================================================ C ABI
namespace {

// ---- the entry guard: what EVERY extern "C" call that takes an engine refuses, in this order, before its own argument checks:
// a null engine, the wrong kind of engine, an engine that is not bound as far as the call needs, a member of a data-parallel group.
// Then come the call's own checks, then the status word (entry_check) where the call consults it, and only then its stream scope (Own):
// a refused call records no event and enqueues nothing.  Every message starts with the call's name.
// Three places say one of their own refusals BEFORE the binding, because tests from before the guard pin that order on an unbound engine
// (the call then opens with guard(kind) and runs guard(kind | binding) behind that one check): a bad argument of the three clipping
// calls, training != 0 with a length array, and a backward with no forward -- whose text ("backward without a preceding forward") is
// pinned verbatim, without the call's name.
enum : unsigned {
    G3 = 1, G6 = 2, GEN = G3 | G6, ANY = GEN | 4,      // kind: that generator, either generator, an InterpLnr-only engine as well
    WS = 8, GRADS = WS | 16, ADAM = WS | 32,           // binding: the workspace; also the gradient arena; also both Adam arenas
    NO_DP = 64,                                        // not on a member of a data-parallel group
};
int refuse(const char* call, const char* why) { return fail(std::string(call) + why); }
int guard(const ss_engine* e, const char* call, unsigned need) {
    if (!e) return refuse(call, ": null engine");
    const unsigned kind = e->kind == SS_GENERATOR_3 ? G3 : e->kind == SS_GENERATOR_6 ? G6 : 4u;
    if (!(need & kind))      // the kind the call needs, then the kind the engine was created as (known, not guessed)
        return fail(std::string(call) + " on an engine that is not a " +
                    ((need & ANY) == G3 ? "Generator_3" : (need & ANY) == G6 ? "Generator_6" : "Generator_3 or a Generator_6") + ": it is " +
                    (kind == G3 ? "a Generator_3" : kind == G6 ? "a Generator_6" : "InterpLnr-only"));
    if (((need & WS) && !e->ws) || ((need & GRADS & ~WS) && !e->G)) return refuse(call, ": engine is not bound (call ss_bind first)");
    if ((need & ADAM & ~WS) && (!e->Mm || !e->Vv)) return refuse(call, ": Adam arenas are not bound (pass SS_STEP_NO_ADAM where the call takes flags)");
    if ((need & NO_DP) && e->dp_on) return refuse(call, ": not available on a member of a data-parallel group");
    return 0;
}
unsigned adam_unless(int flags) { return (flags & SS_STEP_NO_ADAM) ? 0u : ADAM; }

// B and T of a call that plans the workspace -- everything geometry() would refuse, said under the call's name before anything is enqueued.
// eval: an eval-mode forward (T up to SS_MAX_EVAL_FRAMES); everything that trains or differentiates keeps T <= max_frames.
// replan: the plan is about to change for another reason (max_len_pad), so the current shape says nothing about what fits.
int shape_check(const ss_engine* e, const char* call, int B, int T, bool eval, bool replan = false) {
    if (B < 1 || B > e->maxB) return refuse(call, ": batch outside 1 .. max_batch given to ss_create");
    if (eval && (T < 1 || T > SS_MAX_EVAL_FRAMES)) return refuse(call, ": T outside 1 .. SS_MAX_EVAL_FRAMES (8192)");
    if (!eval && (T < 1 || T > e->maxT))
        return refuse(call, ": T outside 1 .. max_frames (everything that trains or is differentiated keeps T <= max_frames <= 256, as every backward does; "
                        "longer sequences run in eval mode only)");
    if (e->kind != SS_INTERP_ONLY && (T % e->hp.freq || T % e->hp.freq_2 || T % e->hp.freq_3))
        return refuse(call, ": T must be a multiple of the code down-sampling factors (model.py:87,223-227)");
    if ((replan || B != e->curB || T != e->curT) && carve(*e, B, T) > e->ws_bytes)
        return refuse(call, ": workspace too small for this batch / frames: grow it to ss_plan_bytes(B, T) with ss_set_workspace");
    return 0;
}

// Everything that runs InterpLnr inside the model (train-mode forwards, the training steps) needs T == max_len_pad, within max_frames
int train_len(const ss_engine* e, const char* call, int T, int max_len_pad) {
    if (T > e->maxT) return refuse(call, ": training: T above max_frames; frames above max_frames (<= 256) run in eval mode only");
    if (T != max_len_pad)
        return refuse(call, ": training needs T == max_len_pad (InterpLnr pads to it, model.py:105,157,370); pass SS_STEP_BUCKET for a length-bucketed batch");
    return 0;
}
// The max_len_pad a training STEP at T frames runs with: the one the engine was created with, or T itself under SS_STEP_BUCKET (a step
// WITHOUT the flag runs with the created one again, whatever bucket came before: speechsplit_amd/solver.py mixes buckets with full-length
// batches).  Refuses a T that is not that length; nothing is changed here (set_max_len_pad, once the call can no longer be refused).
int step_len(const ss_engine* e, const char* call, int T, int flags, int* want) {
    *want = (flags & SS_STEP_BUCKET) ? T : e->bound_max_len_pad;      // the batch's length bucket
    if ((flags & SS_STEP_BUCKET) && (T < 8 || T % 8)) return refuse(call, ": SS_STEP_BUCKET: T must be a multiple of 8 within the engine's max_frames");
    return train_len(e, call, T, *want);
}
void set_max_len_pad(ss_engine* e, int want) {
    if (e->hp.max_len_pad == want) return;
    e->hp.max_len_pad = want;
    e->curB = e->curT = 0;         // InterpLnr plans are sized by max_len_pad: carve again
}

// ---- what differs between the two generators, as data (beside code_srcs, which does the same for the codes)
// One dense caller input: argument `arg` of the call ([B][T][row], its columns from `col` on) is staged in `slab` and read by the layer-0
// conv block `cb`, whose input gradient is therefore that argument's gradient.  In the order the staging copies are enqueued.
struct InputSrc {
    int arg;
    float* slab;
    int slab_ld, width, col, row;
    const ConvBlk* cb;
};
int input_srcs(const ss_engine* e, InputSrc in[3]) {
    const ss_hparams& h = e->hp;
    if (e->kind == SS_GENERATOR_3) {      // (x_f0, x_org): x_f0 = [mel 80 | f0 one-hot 257] splits into the mel and the (channel-padded) f0 slab (model.py:196-197)
        const int CI = h.dim_freq + h.dim_f0;
        in[0] = {0, e->in_mel, h.dim_freq, h.dim_freq, 0, CI, &e->c1[0]};
        in[1] = {0, e->in_f0, e->f0p, h.dim_f0, h.dim_freq, CI, &e->c2[0]};
        in[2] = {1, e->org, h.dim_freq, h.dim_freq, 0, h.dim_freq, &e->ct};
        return 3;
    }
    in[0] = {0, e->org, h.dim_freq, h.dim_freq, 0, h.dim_freq, &e->ct};      // (x_org, f0_trg): Encoder_t, Encoder_6's stack (model.py:123-140)
    in[1] = {1, e->in_f0, e->f0p, h.dim_f0, 0, h.dim_f0, &e->c2[0]};
    return 2;
}
bool has_speaker_row(const ss_engine* e) { return e->kind == SS_GENERATOR_3; }
// first arena offset of the decoder + head parameters (ss_grad_split)
long grad_split(const ss_engine* e) {
    for (const auto& p : e->params)
        if (p.name.rfind("decoder.", 0) == 0) return p.offset;
    return e->arena;
}

// x[arg] (NULL: that argument is not part of this call, ss_g3_rhythm) into the slabs, then the speaker rows if given
// lens (nullable): ragged batch -- frames t >= len[b] of the inputs are not read, the slabs get zeros there
int stage_inputs(ss_engine* e, const float* const x[2], const float* c_trg, int B, int T, hipStream_t s, const int* lens = nullptr) {
    InputSrc in[3];
    const int n = input_srcs(e, in);
    for (int i = 0; i < n; ++i)
        if (x[in[i].arg])
            HIPCHK(copy_rows(CRows::dense(x[in[i].arg], in[i].row, T).col(in[i].col), Rows::slab(in[i].slab, in[i].slab_ld, T), B, T, in[i].width, s, lens));
    if (c_trg) HIPCHK(hipMemcpyAsync(e->emb, c_trg, (long)B * e->hp.dim_spk_emb * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// one BLSTM block's per-call weight preparation on its own (forward_branch_work batches the blocks of a whole forward)
int prep_block(ss_engine* e, LstmBlk& lb, hipStream_t s) {
    PrepTable tb;
    tb.n = 0;
    tb.img_bf16 = e->img16();
    CHK(lstm_prep(e, lb, tb, s));
    HIPCHK(prep_run(tb, s));
    return 0;
}

// lens (nullable): ragged batch -- the head is row-wise and leaves its bias in the padded frames of the slab; the caller's tensor gets zeros
int export_out(ss_engine* e, float* out, int B, int T, hipStream_t s, const int* lens = nullptr) {
    const int C = e->head_out;
    HIPCHK(copy_rows(CRows::slab(e->out_slab, C, T), Rows::dense(out, C, T), B, T, C, s, lens));
    return 0;
}

int import_dout(ss_engine* e, const float* d_out, int B, int T, hipStream_t s) {
    const int C = e->head_out;
    HIPCHK(copy_rows(CRows::dense(d_out, C, T), Rows::slab(e->d_out_slab, C, T), B, T, C, s));
    return 0;
}

}  // namespace

extern "C" {

int ss_comm_destroy(ss_engine* e);
const char* ss_last_error(void) { return g_err.c_str(); }
int ss_abi_version(void) { return 2; }      // 2: ss_profile(mask) / ss_profile_read, status word, RCCL entry points, SS_STEP_BUCKET

ss_engine* ss_create(int kind, const ss_hparams* hp, int max_batch, int max_frames) {
    if (!hp || (kind != SS_GENERATOR_3 && kind != SS_GENERATOR_6 && kind != SS_INTERP_ONLY)) {
        fail("ss_create: kind must be SS_GENERATOR_3, SS_GENERATOR_6 or SS_INTERP_ONLY");
        return nullptr;
    }
    // Every field is either inside the set the header states for it or refused here, before anything is built ("Hyper-parameters", has
    // the kernel-by-kernel audit behind each bound)
    auto refuse = [](const char* msg) -> ss_engine* {
        fail(msg);
        return nullptr;
    };
    if (hp->chs_grp != 16) return refuse("ss_create: chs_grp must be 16 (the GroupNorm kernels work on 64-channel tiles of four 16-channel groups)");
    for (int c : {hp->dim_enc, hp->dim_enc_2, hp->dim_enc_3})
        if (c < 64 || c > 1024 || c % 64) return refuse("ss_create: conv widths (dim_enc, dim_enc_2, dim_enc_3) must be multiples of 64 in 64..1024");
    if (hp->max_len_pad < 1 || hp->max_len_pad > 512 || max_frames > 256 || max_frames < 8 || max_batch < 1)
        return refuse("ss_create: limits are 1 <= max_len_pad <= 512, 8 <= max_frames <= 256, max_batch >= 1");
    // InterpLnr (model.py:365, 389, 399-402): the plan kernel gives every candidate position of a segment one lane of a wavefront
    // (2 * max_len_seg <= 64), the segment count is max_len_seq / min_len_seg + 1 and the lengths are drawn from [min_len_seg, max_len_seg)
    if (hp->min_len_seg < 1 || hp->min_len_seg >= hp->max_len_seg || hp->max_len_seg > 32)
        return refuse("ss_create: segment lengths must satisfy 1 <= min_len_seg < max_len_seg <= 32");
    if (hp->max_len_seq < 1 || hp->max_len_seq > 512) return refuse("ss_create: max_len_seq must be in 1..512");
    for (int hdim : {hp->dim_neck, hp->dim_neck_2, hp->dim_neck_3}) {
        if (hdim < 1 || hdim > 32)      // the encoder BLSTMs' single-launch recurrences and fused weight gradients (H <= 32)
            return refuse("ss_create: bottleneck widths (dim_neck, dim_neck_2, dim_neck_3) must be in 1..32");
    }
    if (kind != SS_INTERP_ONLY) {
        // the mel slabs' rows are dim_freq floats apart and the k = 5 convolutions read align4(dim_freq) columns per tap: a width that is no
        // multiple of 4 would read past each row and, at the slab's last row, past the slab; K segments shorter than a k-tile (32) never ran
        if (hp->dim_freq < 32 || hp->dim_freq > 512 || hp->dim_freq % 4)
            return refuse("ss_create: dim_freq must be a multiple of 4 in 32..512");
        // one thread per speaker column in the speaker-gradient kernel's 1024-thread workgroup
        if (hp->dim_spk_emb < 1 || hp->dim_spk_emb > 1024) return refuse("ss_create: dim_spk_emb must be in 1..1024");
        // Generator_3 quantises the resampled F0 itself into 256 bins + unvoiced (utils.py:62-74); Generator_6 takes the one-hot as an input
        if (kind == SS_GENERATOR_3 && hp->dim_f0 != 257)
            return refuse("ss_create: dim_f0 must be 257 for Generator_3 (the F0 quantiser has 256 bins plus unvoiced)");
        if (kind == SS_GENERATOR_6 && (hp->dim_f0 < 32 || hp->dim_f0 > 512))
            return refuse("ss_create: dim_f0 must be in 32..512 for Generator_6");
    }
    ss_engine* e = new ss_engine();
    e->kind = kind;
    e->hp = *hp;
    e->bound_max_len_pad = hp->max_len_pad;
    e->maxB = max_batch;
    e->maxT = max_frames;
    build_table(e);
    return e;
}

void ss_destroy(ss_engine* e) {
    if (!e) return;
    if (e->comm) (void)ss_comm_destroy(e);
    if (e->sticky) {
        (void)hipDeviceSynchronize();
        (void)hipHostFree(e->sticky);
    }
    // every stream of the engine's own drains, then all events go, then the streams
    const hipStream_t streams[] = {e->side, e->side2, e->side3, e->main_s};
    for (hipStream_t st : streams)
        if (st) (void)hipStreamSynchronize(st);
    std::vector<hipEvent_t> events(e->prof_ev);
    events.insert(events.end(), e->dp_ev_pool.begin(), e->dp_ev_pool.end());
    events.insert(events.end(), {e->ev_comm, e->dp_bwd_end});
    events.insert(events.end(), std::begin(e->ev), std::end(e->ev));
    events.insert(events.end(), std::begin(e->ev_io), std::end(e->ev_io));
    events.insert(events.end(), std::begin(e->ev_dec), std::end(e->ev_dec));
    events.insert(events.end(), std::begin(e->ev_join), std::end(e->ev_join));
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t st : streams)
        if (st) (void)hipStreamDestroy(st);
    delete e;
}

int ss_num_params(const ss_engine* e) { return guard(e, "ss_num_params", ANY) ? -1 : (int)e->params.size(); }

int ss_param_info(const ss_engine* e, int i, char* name, int cap, long* offset, int* ndim, long shape[3]) {
    CHK(guard(e, "ss_param_info", ANY));
    if (i < 0 || i >= (int)e->params.size()) return fail("ss_param_info: index out of range");
    const ParamInfo& p = e->params[i];
    if (name && cap > 0) {
        std::strncpy(name, p.name.c_str(), cap - 1);
        name[cap - 1] = 0;
    }
    if (offset) *offset = p.offset;
    if (ndim) *ndim = p.ndim;
    if (shape)
        for (int k = 0; k < 3; ++k) shape[k] = p.shape[k];
    return 0;
}

long ss_arena_numel(const ss_engine* e) { return guard(e, "ss_arena_numel", ANY) ? -1 : e->arena; }

// split-K scratch of the image GEMM behind the planned workspace (never zeroed, independent of the geometry): partial slabs have the
// size of weight tensors, so 16 arenas' worth holds a step's launches at ksplit <= 8 with room to spare
static long part_floats(const ss_engine* e) { return e->kind == SS_INTERP_ONLY ? 0 : 16 * ((e->arena + 63) & ~63L) + (32L << 20); }      // + 32 M floats: the small generator's deterministic mode, column sums, fused encoder weight gradients
static long plan_bytes(const ss_engine* e) { return (carve(*e, e->maxB, e->maxT) + 255) & ~255L; }
static long workspace_bytes(const ss_engine* e) { return plan_bytes(e) + part_floats(e) * 4; }
long ss_workspace_bytes(const ss_engine* e) { return guard(e, "ss_workspace_bytes", ANY) ? -1 : workspace_bytes(e); }

long ss_plan_bytes(const ss_engine* e, int B, int T) {
    CHK(guard(e, "ss_plan_bytes", ANY));
    if (B < 1 || B > e->maxB) return fail("ss_plan_bytes: batch outside 1 .. max_batch");
    if (T < 8 || T > SS_MAX_EVAL_FRAMES) return fail("ss_plan_bytes: frames outside 8 .. SS_MAX_EVAL_FRAMES");
    if (e->kind != SS_INTERP_ONLY && (T % e->hp.freq || T % e->hp.freq_2 || T % e->hp.freq_3))
        return fail("ss_plan_bytes: T must be a multiple of the code down-sampling factors (model.py:87,223-227)");
    return ((carve(*e, B, T) + 255) & ~255L) + part_floats(e) * 4;
}

static_assert(sizeof(AdamState) <= 256, "the Adam state is the workspace's first 256 bytes");
static_assert(sizeof(AdamState) <= CLIP_STATE_BYTE && CLIP_STATE_BYTE + sizeof(ClipState) <= 256 && CLIP_STATE_BYTE % 16 == 0,
              "the clip state shares those 256 bytes (ss_set_adam rewrites sizeof(AdamState) of them, no more)");
static_assert(OPT_EXT_STATE_BYTE >= CLIP_STATE_BYTE + (long)sizeof(ClipState) && OPT_EXT_STATE_BYTE + sizeof(OptExtState) <= 256 &&
                  OPT_EXT_STATE_BYTE % 16 == 0 && offsetof(OptExtState, stats) == 0,
              "the weight-decay / EMA state shares those 256 bytes too (its four stats words are handed out as one float4)");
static_assert(LR_SCHED_STATE_BYTE >= OPT_EXT_STATE_BYTE + (long)sizeof(OptExtState) && LR_SCHED_STATE_BYTE + sizeof(LrSchedState) <= 256 &&
                  LR_SCHED_STATE_BYTE % 16 == 0 && offsetof(LrSchedState, stats) == 0,
              "and so does the learning-rate schedule, behind them");
int ss_set_workspace(ss_engine* e, void* ws_dev, long bytes, void* stream) {
    CHK(guard(e, "ss_set_workspace", ANY | WS));
    if (!ws_dev || ((uintptr_t)ws_dev & 255)) return fail("ss_set_workspace: the workspace must be 256-byte aligned");
    if (bytes < workspace_bytes(e)) return fail("ss_set_workspace: workspace smaller than ss_workspace_bytes()");
    // nothing may still run on the old workspace once the caller frees it: every stream the engine enqueues on drains first
    HIPCHK(hipStreamSynchronize(S(stream)));
    for (hipStream_t st : {e->main_s, e->side, e->side2, e->side3, e->comm_s})
        if (st) HIPCHK(hipStreamSynchronize(st));
    char* old = e->ws;
    e->ws = (char*)ws_dev;
    e->ws_bytes = ((bytes - part_floats(e) * 4) & ~255L);
    e->part = (float*)(e->ws + e->ws_bytes);
    e->part_cap = part_floats(e);
    e->part_off = 0;
    e->curB = e->curT = 0;          // the next call plans (and zeroes) its geometry in the new workspace
    e->fwd = {};
    // the head of the workspace (the Adam state at offset 0, 256 bytes) survives, as across geometry changes; the rest starts zero
    HIPCHK(hipMemcpyAsync(e->ws, old, 256, hipMemcpyDeviceToDevice, S(stream)));
    HIPCHK(hipMemsetAsync(e->ws + 256, 0, e->ws_bytes - 256, S(stream)));
    carve(*e, e->maxB, e->maxT);
    HIPCHK(hipStreamSynchronize(S(stream)));
    return 0;
}

int ss_bind(ss_engine* e, float* params, float* grads, float* m, float* v, void* workspace, long ws_bytes, void* stream) {
    CHK(guard(e, "ss_bind", ANY));
    if (!workspace || (e->kind != SS_INTERP_ONLY && (!params || !grads))) return fail("ss_bind: null arena");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v | (uintptr_t)workspace) & 255)
        return fail("ss_bind: arenas must be 256-byte aligned");
    const long need = workspace_bytes(e);
    if (ws_bytes < need) return fail("ss_bind: workspace smaller than ss_workspace_bytes()");
    e->P = params;
    e->G = grads;
    e->accum_count = 0;
    e->bwd_accumulate = false;
    e->Mm = m;
    e->Vv = v;
    e->ws = (char*)workspace;
    e->ws_bytes = plan_bytes(e);
    e->part = (float*)(e->ws + e->ws_bytes);
    e->part_cap = part_floats(e);
    e->part_off = 0;
    e->curB = e->curT = 0;
    e->fwd = {};
    HIPCHK(hipMemsetAsync(e->ws, 0, e->ws_bytes, S(stream)));
    carve(*e, e->maxB, e->maxT);
    if (!e->sticky) {       // host-coherent pinned word: kernels OR into it (system scope), the host reads it without a sync
        void* p = nullptr;
        HIPCHK(hipHostMalloc(&p, 64, hipHostMallocDefault));
        std::memset(p, 0, 64);
        e->sticky = (unsigned*)p;
    }
    if (!e->side && e->kind != SS_INTERP_ONLY) {
        // main + three branch streams, created back to back: HIP deals a process's streams onto its hardware queues in creation
        // order, so these four get one queue each no matter how many streams (PyTorch's, RCCL's) existed before
        if (g_own_streams) HIPCHK(hipStreamCreateWithFlags(&e->main_s, hipStreamNonBlocking));
        if (g_probe_queues) {
            // branch streams chosen by MEASURING which candidates share a hardware queue with the stream the step will be issued on
            hipStream_t branch[3];
            CHK(pick_streams((g_own_streams && e->main_s) ? e->main_s : S(stream), branch, e->stream_report));
            e->side = branch[0];
            e->side2 = branch[1];
            e->side3 = branch[2];
        } else {
            // (the side stream at the lowest priority: measured 2.3x SLOWER, 35 ms vs 14.8 ms per step -- the low-priority queue starves
            // behind 768 tiny step launches)
            HIPCHK(hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, 0));
            HIPCHK(hipStreamCreateWithFlags(&e->side2, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&e->side3, hipStreamNonBlocking));
            e->stream_report = "branch streams as created (probe off)";
        }
        for (auto& ev : e->ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (auto& ev : e->ev_io) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (auto& ev : e->ev_dec) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (auto& ev : e->ev_join) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    e->clip_max = 0.0f;       // the workspace (clip state included) starts zero: clipping is off until ss_set_grad_clip
    e->wd = 0.0f;             // ... and so are weight decay and the parameter average (their device state is zero as well)
    e->wd_which = 0;
    e->ema = nullptr;
    e->lr_kind = LR_OFF;      // ... and the learning-rate schedule
    AdamState st{};
    st.lr = 1e-4;
    st.beta1 = 0.9;
    st.beta2 = 0.999;
    st.eps = 1e-8;
    st.step = 0;
    HIPCHK(hipMemcpyAsync(e->adam, &st, sizeof(st), hipMemcpyHostToDevice, S(stream)));
    HIPCHK(hipStreamSynchronize(S(stream)));
    return 0;
}

int ss_set_adam(ss_engine* e, double lr, double b1, double b2, double eps, long step, void* stream) {
    CHK(guard(e, "ss_set_adam", ANY | WS));
    AdamState st{};
    st.lr = lr;
    st.beta1 = b1;
    st.beta2 = b2;
    st.eps = eps;
    st.step = step;
    HIPCHK(hipMemcpyAsync(e->adam, &st, sizeof(st), hipMemcpyHostToDevice, S(stream)));
    HIPCHK(hipStreamSynchronize(S(stream)));
    return 0;
}

// partial sums of the squared gradients the norm still needs on stream s ([split, status_off) unless have_hi says they are there), SS_PROF_ADAM;
// returns the number of partials through *n
static int grad_norm_partials(ss_engine* e, bool have_hi, hipStream_t s, int* n) {
    if (!e->segs_ok) return fail("gradient norm: the parameter table has more runs than GRAD_SEG_MAX");
    const long k = clip_split(e);
    const int nlo = clip_wgs_lo(e);
    {
        Prof pr(e, SS_PROF_ADAM, s);
        if (k > 0) HIPCHK(grad_sumsq(e->G, e->segs, 0, k, e->clip_part, s));
        if (!have_hi) HIPCHK(grad_sumsq(e->G, e->segs, k, e->status_off, e->clip_part + nlo, s));
    }
    *n = nlo + grad_sumsq_wgs(e->status_off - k);
    return 0;
}

// enqueue only: the host-side status check belongs to the ABI entry points, never to the middle of a step being enqueued
// (the device-side guard in adam_prepare_kernel is what protects the parameters)
// bw: the backward this update follows, for what it has already sent to the side stream (a fresh one: nothing, the whole arena here)
static int adam_enqueue(ss_engine* e, const Backward& bw, float grad_scale, hipStream_t s) {
    if (!e->ws || !e->Mm || !e->Vv) return fail("ss_adam_step: Adam arenas are not bound");
    const AdamExt x = opt_ext(e);
    if (x.on()) {             // weight decay and / or the parameter average: the same three schedules, the extended launches
        if (e->clip_max > 0.0f) {
            const bool have_hi = bw.clip_early_from >= 0 && bw.clip_early_from == clip_split(e);
            int n = 0;
            CHK(grad_norm_partials(e, have_hi, s, &n));
            Prof pr(e, SS_PROF_ADAM, s);
            HIPCHK(adam_prepare_clip_ext(e->adam, e->clip, x, e->sticky, e->G + e->status_off, e->clip_part, n, grad_scale, e->clip_max, s, lr_sched(e)));
            HIPCHK(adam_range_ext(e->P, e->G, e->Mm, e->Vv, 0, e->arena, e->adam, grad_scale, &e->clip->coef, x, s));
            return 0;
        }
        Prof pr(e, SS_PROF_ADAM, s);
        if (bw.adam_early_from >= 0) {     // early_update prepared the step and updated [adam_early_from, arena): the rest under the same state
            HIPCHK(adam_range_ext(e->P, e->G, e->Mm, e->Vv, 0, bw.adam_early_from, e->adam, grad_scale, nullptr, x, s));
            return 0;
        }
        HIPCHK(adam_prepare_ext(e->adam, x, e->sticky, e->G + e->status_off, s, lr_sched(e)));
        HIPCHK(adam_range_ext(e->P, e->G, e->Mm, e->Vv, 0, e->arena, e->adam, grad_scale, nullptr, x, s));
        return 0;
    }
    if (e->clip_max > 0.0f) {              // global norm over the whole (all-reduced) arena, then ONE update launch with the coefficient
        const bool have_hi = bw.clip_early_from >= 0 && bw.clip_early_from == clip_split(e);
        int n = 0;
        CHK(grad_norm_partials(e, have_hi, s, &n));
        {
            Prof pr(e, SS_PROF_ADAM, s);
            HIPCHK(adam_prepare_clip(e->adam, e->clip, e->sticky, e->G + e->status_off, e->clip_part, n, grad_scale, e->clip_max, s, lr_sched(e)));
            HIPCHK(adam_range_clip(e->P, e->G, e->Mm, e->Vv, e->arena, e->adam, grad_scale, &e->clip->coef, s));
        }
        return 0;
    }
    if (bw.adam_early_from >= 0) {         // the decoder + head range went out beside the encoder backward (backward_encoder): the rest, same step state
        Prof pr(e, SS_PROF_ADAM, s);
        HIPCHK(adam_range(e->P, e->G, e->Mm, e->Vv, bw.adam_early_from, e->adam, grad_scale, s));
        return 0;
    }
    Prof pr(e, SS_PROF_ADAM, s);
    HIPCHK(adam_step(e->P, e->G, e->Mm, e->Vv, e->arena, e->adam, grad_scale, e->sticky, e->G + e->status_off, s, lr_sched(e)));
    return 0;
}

int ss_adam_step(ss_engine* e, float grad_scale, void* stream) {
    CHK(guard(e, "ss_adam_step", GEN | GRADS | ADAM));
    CHK(entry_check(e));
    Own own(e, stream);
    return adam_enqueue(e, Backward{}, grad_scale, own.s);      // a stand-alone optimiser step always covers the whole arena
}

int ss_set_grad_clip(ss_engine* e, float max_norm, void* stream) {
    // (the three clip calls say a bad argument before a missing binding: tests/test_capi_grad_clip.py pins that order)
    CHK(guard(e, "ss_set_grad_clip", GEN));      // (an InterpLnr-only engine has no gradient arena)
    if (!(max_norm >= 0.0f)) return fail("ss_set_grad_clip: max_norm must be 0 (off), positive or +inf; negative and NaN are refused");
    CHK(guard(e, "ss_set_grad_clip", GEN | GRADS));
    if (!e->segs_ok) return fail("ss_set_grad_clip: the parameter table has more runs than GRAD_SEG_MAX");
    Own own(e, stream);
    HIPCHK(hipMemsetAsync(e->clip, 0, sizeof(ClipState), own.s));      // norm, coefficient and both counters start again
    e->clip_max = max_norm;
    return 0;
}

int ss_grad_norm(ss_engine* e, float grad_scale, float* norm_dev, void* stream) {
    CHK(guard(e, "ss_grad_norm", GEN));
    if (!norm_dev) return fail("ss_grad_norm: null pointer");
    CHK(guard(e, "ss_grad_norm", GEN | GRADS));
    if (!e->segs_ok) return fail("ss_grad_norm: the parameter table has more runs than GRAD_SEG_MAX");
    Own own(e, stream);
    int n = 0;
    CHK(grad_norm_partials(e, false, own.s, &n));
    {
        Prof pr(e, SS_PROF_ADAM, own.s);
        HIPCHK(grad_norm_finish(e->clip_part, n, grad_scale, norm_dev, own.s));
    }
    return 0;
}

int ss_grad_clip_stats(ss_engine* e, float* out4_dev, void* stream) {
    CHK(guard(e, "ss_grad_clip_stats", GEN));
    if (!out4_dev) return fail("ss_grad_clip_stats: null pointer");
    CHK(guard(e, "ss_grad_clip_stats", GEN | WS));
    Own own(e, stream);
    HIPCHK(hipMemcpyAsync(out4_dev, e->clip, sizeof(ClipState), hipMemcpyDeviceToDevice, own.s));
    return 0;
}

int ss_set_weight_decay(ss_engine* e, float weight_decay, int which, void* stream) {
    CHK(guard(e, "ss_set_weight_decay", GEN | GRADS | ADAM));
    if (!(weight_decay >= 0.0f) || !(weight_decay <= 3.402823466e+38f))
        return fail("ss_set_weight_decay: weight_decay must be 0 (off) or positive and finite; negative, NaN and inf are refused");
    if (which != 0 && which != 1) return fail("ss_set_weight_decay: which must be 0 (every parameter) or 1 (tensors with ndim >= 2 only)");
    if (which == 1 && !e->wd_runs_ok) return fail("ss_set_weight_decay: the parameter table has more runs than WD_RUN_MAX");
    Own own(e, stream);
    // the device keeps the value the prepare kernels form the factor from (the host copy is pageable: the call returns once it is there)
    HIPCHK(hipMemcpyAsync(&e->ext->wd, &weight_decay, sizeof(float), hipMemcpyHostToDevice, own.s));
    HIPCHK(hipStreamSynchronize(own.s));
    e->wd = weight_decay;
    e->wd_which = which;
    return 0;
}

int ss_op_wd_runs(int kind, const ss_hparams* hp, long* start, int* len, int* decayed, int cap) {
    if (!start || !len || !decayed || cap < 0) return fail("ss_op_wd_runs: null pointer or negative cap");
    ss_engine* e = ss_create(kind, hp, 1, 64);      // host side only: the parameter table and what build_table derives from it
    if (!e) return -1;
    const bool ok = e->kind != SS_INTERP_ONLY && e->wd_runs_ok;
    const int n = ok ? e->wd_runs.n : 0;
    for (int k = 0; k < n && k < cap; ++k) {
        start[k] = e->wd_runs.start[k];
        len[k] = e->wd_runs.len[k];
        decayed[k] = e->wd_runs.decayed[k];
    }
    ss_destroy(e);
    return ok ? n : fail("ss_op_wd_runs: an InterpLnr-only engine has no parameters, or the table has more runs than WD_RUN_MAX");
}

int ss_set_ema(ss_engine* e, float* ema_dev, double decay, int warmup, long updates, void* stream) {
    CHK(guard(e, "ss_set_ema", GEN | GRADS | ADAM));
    if (ema_dev && !(decay >= 0.0 && decay < 1.0)) return fail("ss_set_ema: decay must lie in [0, 1)");
    if (ema_dev && ((uintptr_t)ema_dev & 15)) return fail("ss_set_ema: the EMA arena must be 16-byte aligned");
    if (ema_dev && (ema_dev == e->P || ema_dev == e->G || ema_dev == e->Mm || ema_dev == e->Vv))
        return fail("ss_set_ema: the EMA arena must be an arena of its own");
    Own own(e, stream);
    OptExtState st{};         // everything but wd starts again: the counter, the factors, the stats
    st.ema_decay = ema_dev ? decay : 0.0;
    st.n = ema_dev && updates > 0 ? updates : 0;
    st.wd = e->wd;
    st.flags = ema_dev ? (OPT_EXT_EMA | (warmup ? OPT_EXT_WARMUP : 0u)) : 0u;
    st.stats[0] = (float)st.n;
    if (ema_dev && updates < 0) HIPCHK(hipMemcpyAsync(ema_dev, e->P, e->arena * 4, hipMemcpyDeviceToDevice, own.s));
    HIPCHK(hipMemcpyAsync(e->ext, &st, sizeof(st), hipMemcpyHostToDevice, own.s));
    HIPCHK(hipStreamSynchronize(own.s));
    e->ema = ema_dev;
    return 0;
}

int ss_ema_swap(ss_engine* e, void* stream) {
    CHK(guard(e, "ss_ema_swap", GEN | GRADS | ADAM));
    if (!e->ema) return fail("ss_ema_swap: no EMA arena (call ss_set_ema first)");
    Own own(e, stream);
    HIPCHK(arena_swap(e->P, e->ema, e->arena, own.s));
    return 0;
}

int ss_ema_stats(ss_engine* e, float* out4_dev, void* stream) {
    CHK(guard(e, "ss_ema_stats", GEN | GRADS | ADAM));
    if (!out4_dev) return fail("ss_ema_stats: null pointer");
    Own own(e, stream);
    HIPCHK(hipMemcpyAsync(out4_dev, e->ext->stats, 4 * sizeof(float), hipMemcpyDeviceToDevice, own.s));
    return 0;
}

int ss_set_lr_schedule(ss_engine* e, int kind, int warmup_steps, double warmup_start, int total_steps, double gamma, int period, double min_lr,
                       void* stream) {
    CHK(guard(e, "ss_set_lr_schedule", GEN | GRADS | ADAM));
    if (const char* why = lr_schedule_refusal(kind, warmup_steps, warmup_start, total_steps, gamma, period, min_lr))
        return fail(std::string("ss_set_lr_schedule: ") + why);
    Own own(e, stream);
    LrSchedState st{};        // the stats words start again: no step has been applied under this schedule
    st.kind = kind;
    if (kind != LR_OFF) {
        st.W = warmup_steps;
        st.sf = warmup_start;
        st.N = total_steps > 0 ? total_steps : 1;
        st.gamma = gamma;
        st.P = period > 0 ? period : 1;
        st.min_lr = min_lr;
        st.stats[3] = (float)kind;
    }
    HIPCHK(hipMemcpyAsync(e->sch, &st, sizeof(st), hipMemcpyHostToDevice, own.s));
    HIPCHK(hipStreamSynchronize(own.s));
    e->lr_kind = kind;
    return 0;
}

int ss_lr_stats(ss_engine* e, float* out4_dev, void* stream) {
    CHK(guard(e, "ss_lr_stats", GEN | GRADS | ADAM));
    if (!out4_dev) return fail("ss_lr_stats: null pointer");
    Own own(e, stream);
    HIPCHK(hipMemcpyAsync(out4_dev, e->sch->stats, 4 * sizeof(float), hipMemcpyDeviceToDevice, own.s));
    return 0;
}

int ss_zero_grads(ss_engine* e, void* stream) {
    CHK(guard(e, "ss_zero_grads", GEN | GRADS));
    Own own(e, stream);
    HIPCHK(hipMemsetAsync(e->G, 0, e->arena * 4, own.s));
    e->accum_count = 0;
    return 0;
}

long ss_grad_accum_count(const ss_engine* e) { return e ? e->accum_count : 0; }

// every backward: whether the forward that is there (the caller has looked at fwd.have) can be differentiated by this call
static int backward_check(const ss_engine* e, const char* call) {
    if (e->fwd.decode)
        return refuse(call, ": the last forward was a decode (ss_*_decode_train), which ran no encoder: only ss_*_decode_backward can follow it");
    if (e->curT > e->maxT)
        return refuse(call, ": the last forward ran T above max_frames, which is eval-only (GroupNorm backward, training and input "
                        "gradients keep T <= max_frames <= 256)");
    if (e->fwd.ragged)
        return refuse(call, ": the last forward ran over per-row lengths (a ragged batch), which is eval-only (no gradient exists for it)");
    return 0;
}

// ---- one body per ss_g3_* / ss_g6_* pair: the public functions pack their pointers in the order of input_srcs' `arg` and name themselves
// the forward on stream s, behind every refusal (the Generator_6 training step runs it too)
static int forward_on(ss_engine* e, const float* const x[2], const float* c_trg, const float* scales, const int* len_seg, const int* lens, int B, int T,
                      bool training, float* out, hipStream_t s) {
    CHK(geometry(e, B, T, s, !training));
    CHK(stage_inputs(e, x, c_trg, B, T, s, lens));
    CHK(forward_core(e, training, scales, len_seg, 0, s, {}, lens));
    if (out) CHK(export_out(e, out, B, T, s, lens));
    return 0;
}
// behind the guard a forward refuses: training != 0 with lengths, without the draws or at a T that is not max_len_pad
static int forward_call(ss_engine* e, const char* call, unsigned kind, const float* const x[2], const float* c_trg, const float* scales,
                        const int* len_seg, const int* lens, int B, int T, int training, float* out, void* stream) {
    CHK(guard(e, call, kind));
    if (training && lens) return refuse(call, ": ragged batches are eval-only (training != 0 with a length array)");
    CHK(guard(e, call, kind | WS));
    if (!x[0] || !x[1] || (has_speaker_row(e) && !c_trg)) return refuse(call, ": null pointer (every input is required)");
    if (training) CHK(train_len(e, call, T, e->hp.max_len_pad));
    if (training && (!scales || !len_seg)) return refuse(call, ": train-mode forward needs the InterpLnr draws");
    CHK(shape_check(e, call, B, T, !training));
    CHK(entry_check(e));
    Own own(e, stream);
    return forward_on(e, x, c_trg, scales, len_seg, lens, B, T, training != 0, out, own.s);
}

// d_x (nullable as a whole: the plain backward; each entry nullable): the caller's input-gradient buffers, one per forward argument
static int backward_call(ss_engine* e, const char* call, unsigned kind, const float* d_out, float* const* d_x, float* dc_trg, void* stream) {
    CHK(guard(e, call, kind));
    if (!e->fwd.have) return fail("backward without a preceding forward");
    CHK(guard(e, call, kind | GRADS));
    CHK(backward_check(e, call));
    if (!d_out) return refuse(call, ": null pointer (d_out is required)");
    Own own(e, stream);
    hipStream_t s = own.s;
    Backward bw;
    InputSrc in[3];
    const int n = d_x ? input_srcs(e, in) : 0;
    for (int i = 0; i < n; ++i) bw.in_grad[i] = {in[i].cb, d_x[in[i].arg] ? d_x[in[i].arg] + in[i].col : nullptr, in[i].row};
    CHK(import_dout(e, d_out, e->curB, e->curT, s));
    CHK(backward_core(e, bw, s));
    if (dc_trg) CHK(speaker_input_grad(e, dc_trg, s));
    return 0;
}

int ss_g3_forward(ss_engine* e, const float* x_f0, const float* x_org, const float* c_trg, const float* scales,
                  const int* len_seg, int B, int T, int training, float* out, void* stream) {
    const float* const x[2] = {x_f0, x_org};
    return forward_call(e, "ss_g3_forward", G3, x, c_trg, scales, len_seg, nullptr, B, T, training, out, stream);
}

int ss_g3_forward_ragged(ss_engine* e, const float* x_f0, const float* x_org, const float* c_trg, const int* len_dev, int B, int T, int training,
                         float* out, void* stream) {
    const float* const x[2] = {x_f0, x_org};
    return forward_call(e, "ss_g3_forward_ragged", G3, x, c_trg, nullptr, nullptr, len_dev, B, T, training, out, stream);
}

int ss_g6_forward(ss_engine* e, const float* x_org, const float* f0_trg, const float* scales, const int* len_seg, int B,
                  int T, int training, float* out, void* stream) {
    const float* const x[2] = {x_org, f0_trg};
    return forward_call(e, "ss_g6_forward", G6, x, nullptr, scales, len_seg, nullptr, B, T, training, out, stream);
}

int ss_g6_forward_ragged(ss_engine* e, const float* x_org, const float* f0_trg, const int* len_dev, int B, int T, int training, float* out,
                         void* stream) {
    const float* const x[2] = {x_org, f0_trg};
    return forward_call(e, "ss_g6_forward_ragged", G6, x, nullptr, nullptr, nullptr, len_dev, B, T, training, out, stream);
}

int ss_g3_backward(ss_engine* e, const float* d_out, void* stream) { return backward_call(e, "ss_g3_backward", G3, d_out, nullptr, nullptr, stream); }
int ss_g6_backward(ss_engine* e, const float* d_out, void* stream) { return backward_call(e, "ss_g6_backward", G6, d_out, nullptr, nullptr, stream); }

int ss_g3_backward_inputs(ss_engine* e, const float* d_out, float* dx_f0, float* dx_org, float* dc_trg, void* stream) {
    float* const d_x[2] = {dx_f0, dx_org};
    return backward_call(e, "ss_g3_backward_inputs", G3, d_out, d_x, dc_trg, stream);
}

int ss_g6_backward_inputs(ss_engine* e, const float* d_out, float* dx_org, float* df0_trg, void* stream) {
    float* const d_x[2] = {dx_org, df0_trg};
    return backward_call(e, "ss_g6_backward_inputs", G6, d_out, d_x, nullptr, stream);
}

static int rhythm_call(ss_engine* e, const char* call, const float* x_org, const int* lens, int B, int T, float* codes, void* stream) {
    CHK(guard(e, call, G3 | WS));
    if (!x_org || !codes) return refuse(call, ": null pointer (x_org and codes are required)");
    CHK(shape_check(e, call, B, T, true));
    Own own(e, stream);
    hipStream_t s = own.s;
    CHK(geometry(e, B, T, s, true));
    e->part_off = 0;           // step scratch (long-sequence GroupNorm): as at the start of forward_core
    const ss_hparams& h = e->hp;
    const float* const x[2] = {nullptr, x_org};           // Encoder_t's input alone
    CHK(stage_inputs(e, x, nullptr, B, T, s, lens));
    CHK(conv_pack_all(e, e->ct, s));
    CHK(prep_block(e, e->lt, s));
    CHK(act_scales_all(e, s));
    CHK(conv_block_fwd(e, e->ct, Slab{e->org, h.dim_freq}, enc_t_out(e), s, {.lens = lens}));
    CHK(lstm_fwd(e, e->lt, enc_t_out(e), s, lens));
    // (ragged: the recurrence left zeros behind every row's end, so the codes of the padded blocks come out as zeros without a predicate)
    // codes = cat(fwd[:, 7::8], bwd[:, ::8]) (model.py:84-87): reuse the decoder-input assembler on a 2H-wide row (in d_ot's own geometry:
    // padding columns written zero, halo rows untouched) and pick t % freq == 0
    const int W = 2 * h.dim_neck_2;
    const long OW = e->lt.ow();
    CodeSrc tab[3];
    code_srcs(e, tab);
    CodeSrc src = tab[1];           // Encoder_t's row of the table (Generator_3), here alone at column 0 and without a gradient slab
    src.d_o = nullptr;
    src.col = 0;
    HIPCHK(build_dec_in(&src, 1, nullptr, 0, W, e->d_ot, (int)OW, B, T, s));
    CRows every = CRows::slab(e->d_ot, OW, T);
    every.ld *= h.freq_2;           // every freq_2-th frame
    HIPCHK(copy_rows(every, Rows::dense(codes, W, T / h.freq_2), B, T / h.freq_2, W, s));
    e->fwd.have = false;
    return 0;
}

int ss_g3_rhythm(ss_engine* e, const float* x_org, int B, int T, float* codes, void* stream) {
    return rhythm_call(e, "ss_g3_rhythm", x_org, nullptr, B, T, codes, stream);
}

int ss_g3_rhythm_ragged(ss_engine* e, const float* x_org, const int* len_dev, int B, int T, float* codes, void* stream) {
    return rhythm_call(e, "ss_g3_rhythm_ragged", x_org, len_dev, B, T, codes, stream);
}


// ---- codes: the encoders alone, and the decoder on codes the caller supplies (see the header's "codes" section) ----

// after the encoder part: every requested code (NULL: not wanted) in one launch, in the column order of code_srcs
static int export_requested_codes(ss_engine* e, float* const* codes, int B, int T, hipStream_t s, const int* lens) {
    CodeSrc src[3];
    const int n = code_srcs(e, src);
    CodeOut out[3];
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (codes[i]) out[m++] = {src[i].o, codes[i], src[i].H, src[i].freq, src[i].ld, 0};
    HIPCHK(export_codes(out, m, B, T, s, lens));
    return 0;
}

static int encode_call(ss_engine* e, const char* call, unsigned kind, const float* const x[2], const int* lens, int B, int T, float* const codes[3],
                       void* stream) {
    CHK(guard(e, call, kind | WS));
    if (!x[0] || !x[1] || !(codes[0] || codes[1] || codes[2]))
        return refuse(call, ": null pointer (every input is required, and at least one output)");
    CHK(shape_check(e, call, B, T, true));
    CHK(entry_check(e));
    Own own(e, stream);
    hipStream_t s = own.s;
    CHK(geometry(e, B, T, s, true));
    e->fwd.have = false;
    CHK(stage_inputs(e, x, nullptr, B, T, s, lens));          // without the speaker rows
    CHK(forward_encoders(e, false, nullptr, nullptr, 0, s, {}, lens, false));
    return export_requested_codes(e, codes, B, T, s, lens);
}

// the decoder's own weight preparation and the parameter guard, as forward_branch_work runs them inside a whole forward
static int decoder_prep(ss_engine* e, hipStream_t s) {
    CHK(prep_block(e, e->ld, s));
    if ((g_fwd_f16x2 || g_bwd_f16x2) && e->precision == SS_PRECISION_F32 && e->sticky) HIPCHK(param_guard(e->P, e->arena, 2048.0f, e->sticky, s));
    return 0;
}

// The decoder on the caller's codes, on stream s.  train: a dense batch within max_frames, recorded for a backward that stops at the codes
// (ss_*_decode_backward); otherwise eval mode, nothing left to differentiate.  Either way the decoder's slabs are overwritten: whatever
// forward ran before has no backward any more.
static int decode_on(ss_engine* e, const CallerCodes& cc, const int* lens, int B, int T, bool train, hipStream_t s) {
    CHK(geometry(e, B, T, s, !train));
    e->part_off = 0;
    if (train) e->fwd = {};
    else e->fwd.have = false;
    CHK(decoder_prep(e, s));
    CHK(forward_decoder(e, s, lens, &cc));
    if (train) e->fwd.decode = e->fwd.have = true;
    return 0;
}

// ss_*_decode (train = false) and the differentiable ss_*_decode_train (see the header's "differentiable decode" section)
static int decode_call(ss_engine* e, const char* call, unsigned kind, const CallerCodes& cc, const int* lens, int B, int T, bool train, float* out,
                       void* stream) {
    CHK(guard(e, call, kind | WS));
    if (!cc.codes[0] || !cc.codes[1] || (kind == G3 && (!cc.codes[2] || !cc.c_trg)) || !out)
        return refuse(call, ": null pointer (every input and the output are required)");
    CHK(shape_check(e, call, B, T, !train));
    CHK(entry_check(e));
    Own own(e, stream);
    CHK(decode_on(e, cc, lens, B, T, train, own.s));
    return export_out(e, out, B, T, own.s, lens);
}

// The decoder's backward alone, behind d_out_slab: parameter gradients of [ss_grad_split, arena) and the status slot, then whatever of the
// code gradients (in code_srcs order; NULL: not wanted) and the speaker-row gradient is asked for; the side stream's weight gradients joined
static int decode_backward_body(ss_engine* e, float* const* d_codes, float* dc_trg, bool accumulate, hipStream_t s) {
    Backward bw;
    bw.accumulate = accumulate;
    CHK(backward_decoder(e, bw, s));
    CodeSrc src[3];
    const int n = code_srcs(e, src);
    CodeGrad cg[3];
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (d_codes[i]) cg[m++] = {d_codes[i], src[i].H, src[i].freq, src[i].col};
    if (m) HIPCHK(dec_in_codes_grad(cg, m, dec_dx(e).p, e->dec_in_dim, e->curB, e->curT, dec_compact(e) ? e->ld.xf : 0, s));
    if (dc_trg) CHK(speaker_input_grad(e, dc_trg, s));
    return join_side(e, s);
}

// Adam on [ss_grad_split, arena) alone: the early range's update of the fused step (early_update), with the whole arena's norm when clipping
static int adam_decoder_enqueue(ss_engine* e, float grad_scale, hipStream_t s) {
    if (!e->ws || !e->Mm || !e->Vv) return fail("ss_adam_step_decoder: Adam arenas are not bound");
    const long from = grad_split(e);
    if (from % 4 || from >= e->arena) return fail("ss_adam_step_decoder: internal: the decoder range does not start on a multiple of 4 floats");
    const AdamExt x = opt_ext(e);
    if (x.on()) {             // decay inside the range only; the average over the WHOLE arena once: fused behind the update in the range,
                              // a plain pass over the encoder range, whose parameters did not move but whose average still approaches them
        const bool clip = e->clip_max > 0.0f;
        int n = 0;
        if (clip) CHK(grad_norm_partials(e, false, s, &n));
        Prof pr(e, SS_PROF_ADAM, s);
        if (clip) HIPCHK(adam_prepare_clip_ext(e->adam, e->clip, x, e->sticky, e->G + e->status_off, e->clip_part, n, grad_scale, e->clip_max, s, lr_sched(e)));
        else HIPCHK(adam_prepare_ext(e->adam, x, e->sticky, e->G + e->status_off, s, lr_sched(e)));
        HIPCHK(adam_range_ext(e->P, e->G, e->Mm, e->Vv, from, e->arena, e->adam, grad_scale, clip ? &e->clip->coef : nullptr, x, s));
        if (x.ema) HIPCHK(ema_range(x.ema, e->P, from, e->adam, e->ext, s));
        return 0;
    }
    if (e->clip_max > 0.0f) {
        int n = 0;
        CHK(grad_norm_partials(e, false, s, &n));
        Prof pr(e, SS_PROF_ADAM, s);
        HIPCHK(adam_prepare_clip(e->adam, e->clip, e->sticky, e->G + e->status_off, e->clip_part, n, grad_scale, e->clip_max, s, lr_sched(e)));
        HIPCHK(adam_range_clip(e->P + from, e->G + from, e->Mm + from, e->Vv + from, e->arena - from, e->adam, grad_scale, &e->clip->coef, s));
        return 0;
    }
    Prof pr(e, SS_PROF_ADAM, s);
    HIPCHK(adam_prepare(e->adam, e->sticky, e->G + e->status_off, s, lr_sched(e)));
    HIPCHK(adam_range(e->P + from, e->G + from, e->Mm + from, e->Vv + from, e->arena - from, e->adam, grad_scale, s));
    return 0;
}

// what ss_*_decode_backward refuses before anything is enqueued, then the backward behind the caller's d_out
static int decode_backward_call(ss_engine* e, const char* call, unsigned kind, const float* d_out, float* const d_codes[3], float* dc_trg, int flags,
                                void* stream) {
    CHK(guard(e, call, kind | GRADS | NO_DP));
    if (!d_out) return refuse(call, ": null pointer (d_out is required)");
    if (flags & ~SS_STEP_ACCUMULATE) return refuse(call, ": flags other than SS_STEP_ACCUMULATE");
    if (!e->fwd.have) return refuse(call, " without a preceding ss_*_decode_train (a plain ss_*_decode leaves nothing to differentiate)");
    if (!e->fwd.decode) return refuse(call, ": the last forward was a full forward, not a decode: ss_*_backward* differentiates it");
    Own own(e, stream);
    CHK(import_dout(e, d_out, e->curB, e->curT, own.s));
    return decode_backward_body(e, d_codes, dc_trg, (flags & SS_STEP_ACCUMULATE) != 0, own.s);
}

int ss_g3_encode(ss_engine* e, const float* x_f0, const float* x_org, const int* len_dev, int B, int T, float* codes_x, float* codes_r,
                 float* codes_f0, void* stream) {
    const float* const x[2] = {x_f0, x_org};
    float* const codes[3] = {codes_x, codes_r, codes_f0};
    return encode_call(e, "ss_g3_encode", G3, x, len_dev, B, T, codes, stream);
}

int ss_g6_encode(ss_engine* e, const float* x_org, const float* f0_trg, const int* len_dev, int B, int T, float* codes_r, float* codes_f0,
                 void* stream) {
    const float* const x[2] = {x_org, f0_trg};
    float* const codes[3] = {codes_r, codes_f0, nullptr};
    return encode_call(e, "ss_g6_encode", G6, x, len_dev, B, T, codes, stream);
}

int ss_g3_decode(ss_engine* e, const float* codes_x, const float* codes_r, const float* codes_f0, const float* c_trg, const int* len_dev, int B,
                 int T, float* out, void* stream) {
    return decode_call(e, "ss_g3_decode", G3, CallerCodes{{codes_x, codes_r, codes_f0}, c_trg}, len_dev, B, T, false, out, stream);
}

int ss_g6_decode(ss_engine* e, const float* codes_r, const float* codes_f0, const int* len_dev, int B, int T, float* out, void* stream) {
    return decode_call(e, "ss_g6_decode", G6, CallerCodes{{codes_r, codes_f0, nullptr}, nullptr}, len_dev, B, T, false, out, stream);
}

int ss_g3_decode_train(ss_engine* e, const float* codes_x, const float* codes_r, const float* codes_f0, const float* c_trg, int B, int T, float* out,
                       void* stream) {
    return decode_call(e, "ss_g3_decode_train", G3, CallerCodes{{codes_x, codes_r, codes_f0}, c_trg}, nullptr, B, T, true, out, stream);
}

int ss_g6_decode_train(ss_engine* e, const float* codes_r, const float* codes_f0, int B, int T, float* out, void* stream) {
    return decode_call(e, "ss_g6_decode_train", G6, CallerCodes{{codes_r, codes_f0, nullptr}, nullptr}, nullptr, B, T, true, out, stream);
}

int ss_g3_decode_backward(ss_engine* e, const float* d_out, float* d_codes_x, float* d_codes_r, float* d_codes_f0, float* dc_trg, int flags,
                          void* stream) {
    float* const d_codes[3] = {d_codes_x, d_codes_r, d_codes_f0};
    return decode_backward_call(e, "ss_g3_decode_backward", G3, d_out, d_codes, dc_trg, flags, stream);
}

int ss_g6_decode_backward(ss_engine* e, const float* d_out, float* d_codes_r, float* d_codes_f0, int flags, void* stream) {
    float* const d_codes[3] = {d_codes_r, d_codes_f0, nullptr};
    return decode_backward_call(e, "ss_g6_decode_backward", G6, d_out, d_codes, nullptr, flags, stream);
}

int ss_adam_step_decoder(ss_engine* e, float grad_scale, void* stream) {
    CHK(guard(e, "ss_adam_step_decoder", GEN | GRADS | ADAM));
    CHK(entry_check(e));
    Own own(e, stream);
    return adam_decoder_enqueue(e, grad_scale, own.s);
}

int ss_g3_decode_train_step(ss_engine* e, const float* codes_x, const float* codes_r, const float* codes_f0, const float* c_trg,
                            const float* target_mel, int B, int T, float grad_scale, int flags, float* loss, float* dc_trg, void* stream) {
    const char* call = "ss_g3_decode_train_step";
    CHK(guard(e, call, G3 | GRADS | adam_unless(flags) | NO_DP));
    if (!codes_x || !codes_r || !codes_f0 || !c_trg || !target_mel || !loss)
        return fail("ss_g3_decode_train_step: null pointer (every input and loss are required)");
    if (flags & ~(SS_STEP_NO_ADAM | SS_STEP_ACCUMULATE)) return fail("ss_g3_decode_train_step: flags other than SS_STEP_NO_ADAM and SS_STEP_ACCUMULATE");
    CHK(shape_check(e, call, B, T, false));
    CHK(entry_check(e));
    Own own(e, stream);
    hipStream_t s = own.s;
    prof_tick(e);
    CHK(decode_on(e, CallerCodes{{codes_x, codes_r, codes_f0}, c_trg}, nullptr, B, T, true, s));
    const int C = e->head_out;
    HIPCHK(mse_loss(CRows::slab(e->out_slab, C, T), CRows::dense(target_mel, C, T), Rows::slab(e->d_out_slab, C, T), B, T, C, 1.0f, e->loss_part, loss, s));
    float* const d_codes[3] = {nullptr, nullptr, nullptr};
    CHK(decode_backward_body(e, d_codes, dc_trg, (flags & SS_STEP_ACCUMULATE) != 0, s));
    if (!(flags & SS_STEP_NO_ADAM)) CHK(adam_decoder_enqueue(e, grad_scale, s));
    return 0;
}


// ---- the training steps.  The four entry points (one GPU / data parallel, per generator) share everything that can refuse, the prologue
// behind it and the tail (backward + Adam); the two cores between them really differ.
struct Step {
    const float *mel, *f0;            // [B,T,80]; Generator_3: f0 [B,T,1], Generator_6: its one-hot [B,T,257]
    const float* emb;                 // Generator_3: speaker rows
    const int* len_org;               // Generator_3: utterance lengths
    const int* target_idx;            // Generator_6: cross-entropy targets
    const float* scales;
    const int* len_seg;
    int B, T;
    float grad_scale;
    int flags;
    float* loss;
};
constexpr int STEP_FLAGS = SS_STEP_NO_ADAM | SS_STEP_SPLIT_BACKWARD | SS_STEP_SPLIT_NO_JOIN | SS_STEP_ACCUMULATE | SS_STEP_BUCKET;

// a step's own argument checks and the status word, behind the guard; *want: the max_len_pad it runs with
static int step_check(ss_engine* e, const char* call, const Step& a, int* want) {
    const bool g3 = e->kind == SS_GENERATOR_3;
    if (!a.mel || !a.f0 || !a.scales || !a.len_seg || !a.loss || (g3 ? !a.emb || !a.len_org : !a.target_idx))
        return refuse(call, ": null pointer (every input, the draws and loss are required)");
    if (a.flags & ~STEP_FLAGS) return refuse(call, ": flags outside the SS_STEP_* set");
    CHK(step_len(e, call, a.T, a.flags, want));
    const int old = e->hp.max_len_pad;
    e->hp.max_len_pad = *want;          // the plan is sized by it: ask about the one the step would run with
    const int rc = shape_check(e, call, a.B, a.T, false, *want != old);
    e->hp.max_len_pad = old;
    CHK(rc);
    return entry_check(e);
}

// behind the last refusal: the step's max_len_pad, its plan, and whether its launches are bracketed (ss_profile_sample)
static int step_begin(ss_engine* e, const Step& a, int want, hipStream_t s) {
    set_max_len_pad(e, want);
    CHK(geometry(e, a.B, a.T, s));
    prof_tick(e);
    return 0;
}

// the whole backward, then Adam unless SS_STEP_NO_ADAM
static int step_tail(ss_engine* e, Backward& bw, float grad_scale, int flags, hipStream_t s) {
    bw.adam_early = !(flags & SS_STEP_NO_ADAM);   // Adam follows inside this call: its decoder + head range may go out early
    bw.adam_gs = grad_scale;
    CHK(backward_core(e, bw, s));                                                           // solver.py:170-171
    if (!(flags & SS_STEP_NO_ADAM)) CHK(adam_enqueue(e, bw, grad_scale, s));                // solver.py:172
    return 0;
}

static int g3_step_core(ss_engine* e, const Step& a, float grad_scale, int flags, hipStream_t s) {
    const ss_hparams& h = e->hp;
    const int B = a.B, T = a.T;
    // solver.py:160-163: resample [mel | f0] with the utterance lengths, re-quantise the f0 channel
    HIPCHK(interp_plan(e->plan[0], a.scales, a.len_seg, a.len_org, 0, B, s));
    HIPCHK(interp_quant(e->plan[0], a.mel, a.f0, h.dim_freq, Rows::slab(e->in_mel, h.dim_freq, T), Rows::slab(e->in_f0, e->f0p, T), h.dim_f0, e->qidx, B, s));
    // x_org and the speaker embedding are first read by Encoder_t / the decoder input: their copies ride on the branch stream
    const bool accumulate = (flags & SS_STEP_ACCUMULATE) != 0;
    CHK(forward_core(e, true, a.scales, a.len_seg, 1, s, FusedForward{a.mel, a.emb, true, accumulate}));        // solver.py:165
    const int C = e->head_out;
    HIPCHK(mse_loss(CRows::slab(e->out_slab, C, T), CRows::slab(e->org, C, T), Rows::slab(e->d_out_slab, C, T), B, T, C, 1.0f, e->loss_part, a.loss,
                    s));                                                                    // solver.py:166
    Backward bw;
    bw.accumulate = accumulate;
    if (flags & SS_STEP_SPLIT_BACKWARD) {         // data parallel: stop once the decoder + head gradients are complete
        CHK(backward_decoder(e, bw, s));          // (not late: nothing of it is left pending for ss_train_finish's backward_encoder)
        if (!(flags & SS_STEP_SPLIT_NO_JOIN)) return join_side(e, s);
        // the weight-gradient GEMMs stay on the side stream (joined by backward_encoder, as in the one-call step);
        // ss_wait_decoder_grads() orders the consumer of the decoder range behind both parts
        HIPCHK(hipEventRecord(e->ev_dec[0], s));
        e->dec_pending = 1;
        if (e->side_used) {
            HIPCHK(hipEventRecord(e->ev_dec[1], e->side));
            e->dec_pending = 2;
        }
        return 0;
    }
    return step_tail(e, bw, grad_scale, flags, s);
}

// Generator_6 has no fused staging: the train-mode forward as ss_g6_forward runs it, then cross-entropy
static int g6_step_core(ss_engine* e, const Step& a, float grad_scale, int flags, hipStream_t s) {
    const float* const x[2] = {a.mel, a.f0};
    CHK(forward_on(e, x, nullptr, a.scales, a.len_seg, nullptr, a.B, a.T, true, nullptr, s));
    const int C = e->head_out;
    HIPCHK(ce_loss(CRows::slab(e->out_slab, C, a.T), a.target_idx, Rows::slab(e->d_out_slab, C, a.T), a.B, a.T, C, 1.0f, e->loss_part, a.loss, s));
    Backward bw;
    bw.accumulate = (flags & SS_STEP_ACCUMULATE) != 0;
    return step_tail(e, bw, grad_scale, flags, s);
}

static int step_core(ss_engine* e, const Step& a, float grad_scale, int flags, hipStream_t s) {
    return e->kind == SS_GENERATOR_3 ? g3_step_core(e, a, grad_scale, flags, s) : g6_step_core(e, a, grad_scale, flags, s);
}

static int train_step_call(ss_engine* e, const char* call, unsigned kind, const Step& a, void* stream) {
    CHK(guard(e, call, kind | GRADS | adam_unless(a.flags)));
    int want = 0;
    CHK(step_check(e, call, a, &want));
    Own own(e, stream);
    CHK(step_begin(e, a, want, own.s));
    return step_core(e, a, a.grad_scale, a.flags & ~SS_STEP_BUCKET, own.s);
}

int ss_g3_train_step(ss_engine* e, const float* mel, const float* f0, const float* emb, const int* len_org,
                     const float* scales, const int* len_seg, int B, int T, float grad_scale, int flags, float* loss,
                     void* stream) {
    return train_step_call(e, "ss_g3_train_step", G3, Step{mel, f0, emb, len_org, nullptr, scales, len_seg, B, T, grad_scale, flags, loss}, stream);
}

int ss_g6_train_step(ss_engine* e, const float* mel, const float* f0_onehot, const int* target_idx, const float* scales,
                     const int* len_seg, int B, int T, float grad_scale, int flags, float* loss, void* stream) {
    return train_step_call(e, "ss_g6_train_step", G6, Step{mel, f0_onehot, nullptr, nullptr, target_idx, scales, len_seg, B, T, grad_scale, flags, loss},
                           stream);
}

int ss_train_finish(ss_engine* e, float grad_scale, int flags, void* stream) {
    CHK(guard(e, "ss_train_finish", GEN | GRADS | adam_unless(flags)));
    if (!e->fwd.have) return fail("ss_train_finish without a preceding ss_*_train_step(SS_STEP_SPLIT_BACKWARD)");
    CHK(backward_check(e, "ss_train_finish"));
    Own own(e, stream);
    hipStream_t s = own.s;
    Backward bw;               // a backward of its own: the decoder half (an earlier call) left nothing pending, and nothing goes out early
    bw.accumulate = e->bwd_accumulate;      // ... but the step's choice between adding to the arena and overwriting it holds for both halves
    CHK(backward_encoder(e, bw, s));
    if (!(flags & SS_STEP_NO_ADAM)) CHK(adam_enqueue(e, bw, grad_scale, s));
    return 0;
}

int ss_wait_decoder_grads(ss_engine* e, void* consumer_stream) {
    CHK(guard(e, "ss_wait_decoder_grads", GEN | WS));
    if (!e->dec_pending) return fail("ss_wait_decoder_grads without a preceding SS_STEP_SPLIT_BACKWARD | SS_STEP_SPLIT_NO_JOIN step");
    hipStream_t c = S(consumer_stream);
    HIPCHK(hipStreamWaitEvent(c, e->ev_dec[0], 0));
    if (e->dec_pending == 2) HIPCHK(hipStreamWaitEvent(c, e->ev_dec[1], 0));
    e->dec_pending = 0;
    return 0;
}

void* ss_side_stream(ss_engine* e) { return guard(e, "ss_side_stream", ANY) ? nullptr : (void*)e->side; }

long ss_grad_split(const ss_engine* e) { return guard(e, "ss_grad_split", ANY) ? -1 : grad_split(e); }

int ss_interp_forward(ss_engine* e, const float* x, const int* len_seq, const float* scales, const int* len_seg, int B, int T,
                      int C, float* y, int* i0, float* lam, int* counts, void* stream) {
    CHK(guard(e, "ss_interp_forward", ANY | WS));
    if (!x || !len_seq || !scales || !len_seg || !y) return fail("ss_interp_forward: null pointer (x, len_seq, the draws and y are required)");
    if (B > e->maxB || T > e->maxT) return fail("ss_interp_forward: batch / frames exceed the engine limits (InterpLnr keeps T <= max_frames)");
    if (!e->curB) CHK(shape_check(e, "ss_interp_forward", e->maxB, e->maxT, false));      // a first call plans the engine's largest shape
    if ((long)B * (T + 1) > (e->curB ? (long)e->curB * (e->curT + 1) : (long)e->maxB * (e->maxT + 1))) return fail("ss_interp_forward: plan storage too small");
    Own own(e, stream);
    hipStream_t s = own.s;
    if (!e->curB) CHK(geometry(e, e->maxB, e->maxT, s));
    InterpPlan pl = e->plan[3];     // standalone calls use the last plan slot with their own T
    pl.T = T;
    const int P = pl.P;
    HIPCHK(interp_plan(pl, scales, len_seg, len_seq, 0, B, s));
    HIPCHK(interp_gather(pl, CRows::dense(x, C, T), Rows::dense(y, C, P), C, B, s));
    if (i0) HIPCHK(hipMemcpyAsync(i0, pl.i0, (long)B * P * 4, hipMemcpyDeviceToDevice, s));
    if (lam) HIPCHK(hipMemcpyAsync(lam, pl.lam, (long)B * P * 4, hipMemcpyDeviceToDevice, s));
    if (counts) HIPCHK(hipMemcpyAsync(counts, pl.counts, (long)B * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int ss_interp_backward(ss_engine* e, const float* dy, int B, int T, int C, float* dx, void* stream) {
    CHK(guard(e, "ss_interp_backward", ANY | WS));
    if (!e->curB) return fail("ss_interp_backward without ss_interp_forward");
    if (!dy || !dx) return fail("ss_interp_backward: null pointer (dy and dx are required)");
    if (B > e->maxB || T > e->maxT) return fail("ss_interp_backward: batch / frames exceed the engine limits (InterpLnr keeps T <= max_frames)");
    Own own(e, stream);
    InterpPlan pl = e->plan[3];
    pl.T = T;
    const int P = pl.P;
    HIPCHK(interp_scatter(pl, CRows::dense(dy, C, P), Rows::dense(dx, C, T), C, B, own.s));
    return 0;
}

int ss_set_precision(ss_engine* e, int precision) {
    CHK(guard(e, "ss_set_precision", ANY));
    if (precision != SS_PRECISION_F32 && precision != SS_PRECISION_BF16) return fail("ss_set_precision: unknown precision");
    if (precision != e->precision) e->fwd = {};      // a forward of the other precision cannot be differentiated: its backward is refused
    e->precision = precision;
    return 0;
}

int ss_profile(ss_engine* e, unsigned class_mask) {
    CHK(guard(e, "ss_profile", ANY));
    if (class_mask) e->prof_n = 0;
    e->prof_mask = class_mask;
    e->prof_ctr = 0;
    e->prof_live = true;
    return 0;
}

int ss_profile_sample(ss_engine* e, int every_nth_step) {
    CHK(guard(e, "ss_profile_sample", ANY));
    if (every_nth_step < 1) return fail("ss_profile_sample: needs n >= 1");
    e->prof_every = every_nth_step;
    e->prof_ctr = 0;
    e->prof_live = true;
    return 0;
}

int ss_profile_read(ss_engine* e, int klass, int* launches, double* total_us, double* total_flops) {
    CHK(guard(e, "ss_profile_read", ANY));
    int n = 0;
    double us = 0, fl = 0;
    for (int i = 0; i < e->prof_n; ++i) {
        if (e->prof_rec[i].klass != klass) continue;
        if (hipEventSynchronize(e->prof_ev[2 * i + 1]) != hipSuccess) return fail("ss_profile_read: event sync failed");
        float ms = 0;
        if (hipEventElapsedTime(&ms, e->prof_ev[2 * i], e->prof_ev[2 * i + 1]) != hipSuccess)
            return fail("ss_profile_read: elapsed time failed");
        us += ms * 1e3;
        fl += e->prof_rec[i].flops;
        ++n;
    }
    if (launches) *launches = n;
    if (total_us) *total_us = us;
    if (total_flops) *total_flops = fl;
    return 0;
}

// The brackets of ss_profile as a timeline: per record (class, start, end) in microseconds relative to the first record's start event --
// timestamps from the real run (no tracing tool slowing the host down), across the engine's streams.  3 doubles per record, enqueue order.
int ss_profile_timeline(ss_engine* e, double* out, int cap) {
    CHK(guard(e, "ss_profile_timeline", ANY));
    if (!out || cap < 0) return fail("ss_profile_timeline: null argument");
    const int n = e->prof_n < cap ? e->prof_n : cap;
    for (int i = 0; i < n; ++i) {
        if (hipEventSynchronize(e->prof_ev[2 * i + 1]) != hipSuccess) return fail("ss_profile_timeline: event sync failed");
        float a = 0, b = 0;
        if (hipEventElapsedTime(&a, e->prof_ev[0], e->prof_ev[2 * i]) != hipSuccess || hipEventElapsedTime(&b, e->prof_ev[0], e->prof_ev[2 * i + 1]) != hipSuccess)
            return fail("ss_profile_timeline: elapsed time failed");
        out[3 * i] = e->prof_rec[i].klass + 100 * e->prof_rec[i].stream;      // class + 100 x stream (0 main, 1 side, 2 / 3 branch streams)
        out[3 * i + 1] = a * 1e3;
        out[3 * i + 2] = b * 1e3;
    }
    return n;
}

int ss_check(ss_engine* e, void* stream) {
    CHK(guard(e, "ss_check", ANY));
    HIPCHK(hipStreamSynchronize(S(stream)));
    HIPCHK(hipGetLastError());
    for (LstmBlk* lb : {&e->ld, &e->l1, &e->l2, &e->lt}) {
        if (!lb->zf) continue;
        for (int l = 0; l < 2 * lb->L; ++l) {
            unsigned flag = 0;
            HIPCHK(hipMemcpy(&flag, l < lb->L ? lb->sync_f(l) : lb->sync_b(l - lb->L), 4, hipMemcpyDeviceToHost));
            if (flag) return fail("persistent LSTM kernel gave up waiting for its group (bounded spin expired): results are invalid");
        }
    }
    return sticky_check(e);       // an abort in ANY earlier step (the per-launch words above are re-zeroed every step)
}

int ss_clear_abort(ss_engine* e, void* stream) {
    CHK(guard(e, "ss_clear_abort", ANY));
    HIPCHK(hipStreamSynchronize(S(stream)));
    if (e->sticky) *(volatile unsigned*)e->sticky = 0u;
    return 0;
}

unsigned ss_status(const ss_engine* e) { return e && e->sticky ? *(volatile unsigned*)e->sticky : 0u; }

int ss_debug_buffer(ss_engine* e, const char* name, float** ptr, long* rows, long* cols) {
    CHK(guard(e, "ss_debug_buffer", ANY));
    if (!name || !ptr || !rows || !cols) return fail("ss_debug_buffer: null argument");
    auto it = e->dbg.find(name);
    if (it == e->dbg.end()) return fail(std::string("ss_debug_buffer: no such buffer: ") + name);
    *ptr = it->second.first;
    *rows = (long)e->curB * (e->curT + 2 * HALO);
    *cols = it->second.second;
    return 0;
}

int ss_debug_relu_mask(ss_engine* e, const char* block, float* mask, void* stream) {
    CHK(guard(e, "ss_debug_relu_mask", GEN | WS));
    if (!block || !mask) return fail("ss_debug_relu_mask: null argument");
    if (!e->curB) return fail("ss_debug_relu_mask: no forward has run");
    auto it = e->dbg.find(std::string(block) + ".conv");
    if (it == e->dbg.end()) return fail(std::string("ss_debug_relu_mask: no such conv block: ") + block);
    for (ConvBlk* cb : conv_blocks(*e))
        if (cb->Co && cb->cout == it->second.first) {
            HIPCHK(gn_relu_mask(CRows::slab(cb->cout, cb->Co, e->curT), e->P + cb->ga, e->P + cb->be, cb->stats, mask, e->curB, e->curT, cb->Co, S(stream)));
            return 0;
        }
    return fail("ss_debug_relu_mask: block has no storage");
}

long ss_op_conv_block_scratch(int B, int T, int Ci, int Co) {
    const long Cp = align4(Ci), R = (long)B * (T + 2 * HALO);
    const long np = align4((long)Co * Ci * 5) + 3L * Co;
    const long gn = T > 256 ? ((gn_relu_fwd_scratch_bytes(B, T, Co) / 4 + 63) & ~63L) + 4 : 0;       // long-sequence GroupNorm partials (forward only)
    return 2 * np + 2L * Co * 5 * Cp + (long)Ci * 5 * Co + R * (2 * Cp + 3L * Co) + 2L * B * (Co / 16) + 64 + gn;
}

static int op_conv_block(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, const float* dy,
                         float* y, float* dx, float* gw, float* gb, float* ggamma, float* gbeta, float* scratch, long scratch_floats,
                         const int* len, int B, int T, int Ci, int Co, void* stream) {
    hipStream_t s = S(stream);
    if (!x || !w || !bias || !gamma || !beta || !y || !scratch) return fail("ss_op_conv_block: null pointer");
    if (Co % 64 || T < 1 || B < 1) return fail("ss_op_conv_block: needs Co % 64 == 0, B >= 1 and T >= 1");
    if (T > 256 && (dy || T > SS_MAX_EVAL_FRAMES))
        return fail("ss_op_conv_block: T > 256 runs the forward only (dy == nullptr), up to SS_MAX_EVAL_FRAMES");
    if (scratch_floats < ss_op_conv_block_scratch(B, T, Ci, Co)) return fail("ss_op_conv_block: scratch too small");
    // a stack engine that holds nothing but this block: the product's own conv_block_fwd / conv_block_bwd do the work
    ss_engine e{};
    e.kind = SS_GENERATOR_3;
    e.curB = B;
    e.curT = T;
    const long TP = T + 2 * HALO, R = (long)B * TP;
    ConvBlk cb;
    cb.Ci = Ci;
    cb.Co = Co;
    cb.Cp = (int)align4(Ci);
    cb.w = 0;
    cb.b = align4((long)Co * Ci * 5);
    cb.ga = cb.b + Co;
    cb.be = cb.ga + Co;
    cb.need_dx = dx != nullptr;
    const long np = cb.be + Co;
    HIPCHK(hipMemsetAsync(scratch, 0, ss_op_conv_block_scratch(B, T, Ci, Co) * 4, s));
    float* p = scratch;
    auto take = [&](long n) {
        float* q = p;
        p += align4(n);
        return q;
    };
    e.P = take(np);
    e.G = take(np);
    cb.wf = take((long)Co * 5 * cb.Cp);
    cb.wb = take((long)Ci * 5 * Co);
    cb.gp = take((long)Co * 5 * cb.Cp);
    float* xs = take(R * cb.Cp);
    float* dxs = take(R * cb.Cp);
    cb.cout = take(R * Co);
    float* ys = take(R * Co);
    float* dys = take(R * Co);
    cb.stats = take(2L * B * (Co / 16));
    e.amax = take(16);
    if (const long gn = (gn_relu_fwd_scratch_bytes(B, T, Co) / 4 + 63) & ~63L) {     // conv_block_fwd takes the GroupNorm's partials from the step scratch
        e.part = take(gn);
        e.part_cap = gn;
    }
    cb.amax_i = 0;
    HIPCHK(hipMemcpyAsync(e.P + cb.w, w, (long)Co * Ci * 5 * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(e.P + cb.b, bias, Co * 4L, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(e.P + cb.ga, gamma, Co * 4L, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(e.P + cb.be, beta, Co * 4L, hipMemcpyDeviceToDevice, s));
    HIPCHK(copy_rows(CRows::dense(x, Ci, T), Rows::slab(xs, cb.Cp, T), B, T, Ci, s, len));
    CHK(conv_pack_all(&e, cb, s));
    CHK(conv_block_fwd(&e, cb, Slab{xs, cb.Cp}, Slab{ys, Co}, s, {.lens = len}));
    HIPCHK(copy_rows(CRows::slab(ys, Co, T), Rows::dense(y, Co, T), B, T, Co, s));
    if (dy) {
        if (!gw || !gb || !ggamma || !gbeta) return fail("ss_op_conv_block: backward needs the gradient outputs");
        HIPCHK(copy_rows(CRows::dense(dy, Co, T), Rows::slab(dys, Co, T), B, T, Co, s));
        Backward bw;
        CHK(conv_block_bwd(&e, bw, cb, Slab{dys, Co}, Slab{xs, cb.Cp}, dx ? Slab{dxs, cb.Cp} : Slab{nullptr, 0}, s));
        HIPCHK(hipMemcpyAsync(gw, e.G + cb.w, (long)Co * Ci * 5 * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(gb, e.G + cb.b, Co * 4L, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ggamma, e.G + cb.ga, Co * 4L, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(gbeta, e.G + cb.be, Co * 4L, hipMemcpyDeviceToDevice, s));
        if (dx) HIPCHK(copy_rows(CRows::slab(dxs, cb.Cp, T), Rows::dense(dx, Ci, T), B, T, Ci, s));
    }
    return 0;
}

int ss_op_conv_block(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, const float* dy,
                     float* y, float* dx, float* gw, float* gb, float* ggamma, float* gbeta, float* scratch, long scratch_floats,
                     int B, int T, int Ci, int Co, void* stream) {
    return op_conv_block(x, w, bias, gamma, beta, dy, y, dx, gw, gb, ggamma, gbeta, scratch, scratch_floats, nullptr, B, T, Ci, Co, stream);
}

int ss_op_conv_block_ragged(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, const int* len_dev,
                            float* y, float* scratch, long scratch_floats, int B, int T, int Ci, int Co, void* stream) {
    return op_conv_block(x, w, bias, gamma, beta, nullptr, y, nullptr, nullptr, nullptr, nullptr, nullptr, scratch, scratch_floats, len_dev, B, T,
                         Ci, Co, stream);
}

const char* ss_stream_report(const ss_engine* e) { return guard(e, "ss_stream_report", ANY) ? nullptr : e->stream_report.c_str(); }

int ss_debug_names(ss_engine* e, char* buf, int cap) {
    CHK(guard(e, "ss_debug_names", ANY));
    std::string all;
    for (auto& kv : e->dbg) all += kv.first + "\n";
    if (buf && cap > 0) {
        std::strncpy(buf, all.c_str(), cap - 1);
        buf[cap - 1] = 0;
    }
    return (int)all.size();
}

}  // extern "C"

// ================================================================================================ RCCL (data parallel)
// The reference is single-device (solver.py:38); this is the exchange step of SURVEY.md section 8(e).  RCCL is reached through
// dlopen: no link-time dependency, and inside a PyTorch process the copy PyTorch already loaded is reused (two RCCL copies in
// one process would each bring their own bootstrap state).
namespace {

struct NcclId {
    char internal[128];
};
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(NcclId*) = nullptr;
    int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;

int rccl_load() {
    if (g_rccl.h) return 0;
    void* h = nullptr;
    for (const char* n : {"librccl.so", "librccl.so.1"})
        if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);                     // already in the process (PyTorch's)?
    for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(std::string("RCCL not found: ") + dlerror());
    Rccl r;
    r.h = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce))dlsym(h, "ncclAllReduce");
    r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.GetErrorString || !r.GroupStart || !r.GroupEnd) return fail("RCCL: missing symbols");
    g_rccl = r;
    return 0;
}
#define NCCLCHK(x)                                                                          \
    do {                                                                                    \
        int _r = (x);                                                                       \
        if (_r != 0) return fail(std::string(#x) + ": " + g_rccl.GetErrorString(_r));       \
    } while (0)

// Stand-in for a collective when a data-parallel run is MODELLED on one GPU (ss_tune("dp_model", ranks)): 32 workgroups (RCCL's
// channels) stream the range once -- read and write it back, the memory traffic of a reduction -- and then hold their place until the
// modelled duration has passed.  Model (the conservative one): ring all-reduce, 2 (R - 1) / R of the bytes through
// one xGMI link of 153 GB/s, plus 25 us of launch / protocol latency.
__global__ __launch_bounds__(256) void dp_model_kernel(float* __restrict__ p, long n4, long long ticks) {
    const long long t0 = wall_clock64();                         // constant 100 MHz
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 v = reinterpret_cast<const f32x4*>(p)[i];
        asm volatile("" : "+v"(v));
        reinterpret_cast<f32x4*>(p)[i] = v;
    }
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
// ss_tune("dp_emulate", 1) with dp_model = N: the stand-in MULTIPLIES its range by N -- the sum N identical ranks would produce.  With the
// 1 / N of the Adam step behind it every element must come out as in the one-GPU step: an element reduced twice, or never, shows in the
// first moment (tests/test_gpu_buckets_dp.py).  At world 1 a real all-reduce is the identity, so nothing else on one GPU checks that the
// bucket schedule covers the arena exactly once.
__global__ __launch_bounds__(256) void dp_scale_kernel(float* __restrict__ p, long n, float mul) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] *= mul;
}
double dp_model_us(long bytes, int ranks) { return 25.0 + 2.0 * (ranks - 1) / ranks * (double)bytes / 153e9 * 1e6; }

int allreduce_range(ss_engine* e, long off, long count, hipStream_t st) {
    if (off < 0 || count < 0 || off + count > e->arena) return fail("ss_allreduce_grads: range outside the gradient arena");
    if (count == 0) return 0;
    if (g_dp_model > 1 && (!e->comm || e->comm_world == 1)) {
        if (g_dp_emulate) {
            hipLaunchKernelGGL(dp_scale_kernel, dim3(256), dim3(256), 0, st, e->G + off, count, (float)g_dp_model);
            HIPCHK(hipGetLastError());
            return 0;
        }
        const long a = (off + 3) & ~3L, b = (off + count) & ~3L;       // whole float4s inside the range
        hipLaunchKernelGGL(dp_model_kernel, dim3(32), dim3(256), 0, st, e->G + a, b > a ? (b - a) / 4 : 0, (long long)(dp_model_us(count * 4, g_dp_model) * 100.0));
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (!e->comm) return fail("no communicator: call ss_comm_init first");
    NCCLCHK(g_rccl.AllReduce(e->G + off, e->G + off, (size_t)count, /*ncclFloat*/ 7, /*ncclSum*/ 0, e->comm, st));
    return 0;
}

// ss_dp_profile bracket: a timing event from the pool (null when profiling is off or an event could not be created)
hipEvent_t dp_prof_event(ss_engine* e) {
    if (!e->dp_prof) return nullptr;
    if (e->dp_ev_used == (int)e->dp_ev_pool.size()) {
        hipEvent_t ev = nullptr;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        e->dp_ev_pool.push_back(ev);
    }
    return e->dp_ev_pool[e->dp_ev_used++];
}

// see the declaration above fork_join
int dp_bucket(ss_engine* e, long off, long count, hipStream_t producer) {
    if (!e->dp_on || !g_dp_buckets || count <= 0) return 0;
    if (off < 0 || off + count > e->arena) return fail("dp_bucket: range outside the gradient arena");
    for (auto& r : e->dp_done)          // a range reduced twice would be summed twice: at world 1 nobody would notice, so it is checked here
        if (off < r.second && r.first < off + count) return fail("dp_bucket: gradient range handed to a collective twice");
    HIPCHK(hipEventRecord(e->ev_comm, producer));
    HIPCHK(hipStreamWaitEvent(e->comm_s, e->ev_comm, 0));
    hipEvent_t pa = dp_prof_event(e), pb = pa ? dp_prof_event(e) : nullptr;
    if (pb) HIPCHK(hipEventRecord(pa, e->comm_s));
    CHK(allreduce_range(e, off, count, e->comm_s));
    if (pb) {
        HIPCHK(hipEventRecord(pb, e->comm_s));
        e->dp_rec.push_back({off, count, pa, pb});
    }
    e->dp_done.push_back({off, off + count});
    return 0;
}

// end of a data-parallel backward: everything not yet handed to a collective (layer-0 convolutions, the encoder BLSTMs, Encoder_t, the
// status slot -- a few MB, final only now), then the main stream waits for the communication stream
int dp_finish(ss_engine* e, hipStream_t s) {
    std::sort(e->dp_done.begin(), e->dp_done.end());
    std::vector<std::pair<long, long>> rest;
    long at = 0;
    for (auto& r : e->dp_done) {
        if (r.first > at) rest.push_back({at, r.first});
        if (r.second > at) at = r.second;
    }
    if (at < e->arena) rest.push_back({at, e->arena});
    // ONE launch for all of them (ncclGroupStart / End); modelled: one stand-in over their total size
    HIPCHK(hipEventRecord(e->ev_comm, s));
    HIPCHK(hipStreamWaitEvent(e->comm_s, e->ev_comm, 0));
    hipEvent_t pa = nullptr, pb = nullptr;
    if (e->dp_prof) {
        if (!e->dp_bwd_end) HIPCHK(hipEventCreate(&e->dp_bwd_end));
        HIPCHK(hipEventRecord(e->dp_bwd_end, s));           // the backward's last kernel on the main stream: time zero of the record
        pa = dp_prof_event(e);
        pb = pa ? dp_prof_event(e) : nullptr;
        if (pb) HIPCHK(hipEventRecord(pa, e->comm_s));
    }
    const bool model = g_dp_model > 1 && (!e->comm || e->comm_world == 1);
    if (model && g_dp_emulate) {
        for (auto& r : rest) CHK(allreduce_range(e, r.first, r.second - r.first, e->comm_s));
    } else if (model) {
        long tot = 0;
        for (auto& r : rest) tot += r.second - r.first;
        hipLaunchKernelGGL(dp_model_kernel, dim3(32), dim3(256), 0, e->comm_s, e->G, 0L, (long long)(dp_model_us(tot * 4, g_dp_model) * 100.0));
        HIPCHK(hipGetLastError());
    } else {
        // an open group must be closed whatever happens inside it: a failing member would otherwise leave every later RCCL call of the
        // process queued in a group that never ends
        const bool grouped = rest.size() > 1;
        if (grouped) NCCLCHK(g_rccl.GroupStart());
        int rc = 0;
        for (auto& r : rest)
            if ((rc = allreduce_range(e, r.first, r.second - r.first, e->comm_s)) != 0) break;
        if (grouped) {
            const std::string first_err = rc ? g_err : std::string();
            const int ge = g_rccl.GroupEnd();
            if (rc) return fail(first_err);
            NCCLCHK(ge);
        } else if (rc) return rc;
    }
    if (pb) {
        long tot = 0;
        for (auto& r : rest) tot += r.second - r.first;
        HIPCHK(hipEventRecord(pb, e->comm_s));
        e->dp_rec.push_back({-1, tot, pa, pb});             // offset -1: the grouped rest
    }
    e->dp_done.clear();
    HIPCHK(hipEventRecord(e->ev_comm, e->comm_s));
    HIPCHK(hipStreamWaitEvent(s, e->ev_comm, 0));
    return 0;
}
// The communication stream is the engine's SECOND BRANCH stream, not a fifth stream: HIP serves a process's streams from four hardware
// queues, so a fifth one shares a queue with one of the four the engine already runs on -- measured with modelled collectives
// (gpurun_out/r03/dp: it landed on the MAIN stream's queue, every collective sat in front of the encoder backward's launches and the
// backward took 1.16 ms longer).  The second branch stream has its own queue (pick_streams) and is idle from the first tenth of the
// encoder-backward phase on (it carries the pitch BLSTM's backward); whatever it still holds is simply in front of the first bucket.
int dp_streams(ss_engine* e) {
    e->comm_s = e->side2;
    if (!e->ev_comm) HIPCHK(hipEventCreateWithFlags(&e->ev_comm, hipEventDisableTiming));
    return 0;
}

}  // namespace

extern "C" {

int ss_comm_unique_id(char* id128) {
    if (!id128) return fail("ss_comm_unique_id: null pointer");
    CHK(rccl_load());
    NcclId id;
    NCCLCHK(g_rccl.GetUniqueId(&id));
    std::memcpy(id128, id.internal, 128);
    return 0;
}

int ss_comm_init(ss_engine* e, const char* id128, int rank, int world) {
    CHK(guard(e, "ss_comm_init", GEN | GRADS));
    if (!id128 || world < 1 || rank < 0 || rank >= world) return fail("ss_comm_init: bad arguments");
    if (e->comm) return fail("ss_comm_init: the engine already has a communicator");
    CHK(rccl_load());
    NcclId id;
    std::memcpy(id.internal, id128, 128);
    void* c = nullptr;
    NCCLCHK(g_rccl.CommInitRank(&c, world, id, rank));
    e->comm = c;
    e->comm_rank = rank;
    e->comm_world = world;
    if (world > 1) e->lockstep = true;
    return 0;
}

int ss_set_lockstep(ss_engine* e, int on) {
    CHK(guard(e, "ss_set_lockstep", ANY));
    e->lockstep = on != 0;
    return 0;
}

int ss_comm_destroy(ss_engine* e) {
    CHK(guard(e, "ss_comm_destroy", ANY));
    if (e->comm) {
        (void)hipDeviceSynchronize();
        NCCLCHK(g_rccl.CommDestroy(e->comm));
        e->comm = nullptr;
        e->comm_world = 1;
    }
    return 0;
}

int ss_allreduce_grads(ss_engine* e, long offset, long count, void* stream) {
    CHK(guard(e, "ss_allreduce_grads", GEN | GRADS));
    if (offset < 0 || count < 0 || offset + count > e->arena) return fail("ss_allreduce_grads: range outside the gradient arena");
    if (count && !e->comm && g_dp_model < 2) return fail("ss_allreduce_grads: no communicator: call ss_comm_init first");
    Own own(e, stream);
    return allreduce_range(e, offset, count, own.s);
}

// common part of the data-parallel steps: the step's forward + loss + whole backward (no Adam) with the gradient arena reduced
// in per-layer buckets on the communication stream while the backward is still running (dp_bucket: each of the decoder's layers as
// its four weight-gradient GEMMs retire, the head, the two wide trunk layers, the rest), Adam with the 1 / world mean folded in
static int dp_step(ss_engine* e, const Step& a, hipStream_t s) {
    const int flags = SS_STEP_NO_ADAM | (a.flags & SS_STEP_ACCUMULATE);
    const int world = (g_dp_model > 1 && (!e->comm || e->comm_world == 1)) ? g_dp_model : e->comm_world;
    // the mean over the ranks and over the micro-batches each of them summed into its arena (SS_STEP_ACCUMULATE; 1 without): the count
    // includes the backward the step is about to enqueue, so it is read behind it
    auto mean_scale = [&]() { return 1.0f / (float)((long)world * (e->accum_count > 0 ? e->accum_count : 1)); };
    CHK(dp_streams(e));
    if (!e->side || !e->side2 || !g_overlap || !g_dp_buckets) {        // no branch streams (or round 2's plan asked for): the plain step, then the arena
        CHK(step_core(e, a, 1.0f, flags, s));
        if (g_dp_buckets) CHK(allreduce_range(e, 0, e->arena, s));
        else {
            const long k = grad_split(e);
            CHK(allreduce_range(e, k, e->arena - k, s));
            CHK(allreduce_range(e, 0, k, s));
        }
        return adam_enqueue(e, Backward{}, mean_scale(), s);
    }
    e->dp_done.clear();
    e->dp_rec.clear();              // ss_dp_profile keeps the LAST step's record
    e->dp_ev_used = 0;
    e->dp_on = true;
    const int rc = step_core(e, a, 1.0f, flags, s);
    e->dp_on = false;
    CHK(rc);
    CHK(dp_finish(e, s));
    return adam_enqueue(e, Backward{}, mean_scale(), s);    // the whole arena; the mean is folded into the Adam kernel
}

static int dp_step_call(ss_engine* e, const char* call, unsigned kind, const Step& a, void* stream) {
    CHK(guard(e, call, kind | GRADS | ADAM));
    if (!e->comm && g_dp_model < 2) return refuse(call, ": call ss_comm_init first");
    int want = 0;
    CHK(step_check(e, call, a, &want));      // every rank runs the same bucket (speechsplit_amd/buckets.py)
    Own own(e, stream);
    CHK(step_begin(e, a, want, own.s));
    return dp_step(e, a, own.s);
}

int ss_g3_dp_train_step(ss_engine* e, const float* mel, const float* f0, const float* emb, const int* len_org, const float* scales,
                        const int* len_seg, int B, int T, int flags, float* loss, void* stream) {
    return dp_step_call(e, "ss_g3_dp_train_step", G3, Step{mel, f0, emb, len_org, nullptr, scales, len_seg, B, T, 1.0f, flags, loss}, stream);
}

int ss_g6_dp_train_step(ss_engine* e, const float* mel, const float* f0_onehot, const int* target_idx, const float* scales, const int* len_seg,
                        int B, int T, int flags, float* loss, void* stream) {
    return dp_step_call(e, "ss_g6_dp_train_step", G6, Step{mel, f0_onehot, nullptr, nullptr, target_idx, scales, len_seg, B, T, 1.0f, flags, loss},
                        stream);
}

long ss_scratch_fallbacks(const ss_engine* e) { return e ? e->scratch_fallbacks : -1; }

int ss_dp_profile(ss_engine* e, int on) {
    CHK(guard(e, "ss_dp_profile", ANY));
    e->dp_prof = on != 0;
    e->dp_rec.clear();
    e->dp_ev_used = 0;
    return 0;
}

int ss_dp_profile_read(ss_engine* e, double* out, int cap) {
    CHK(guard(e, "ss_dp_profile_read", ANY));
    const int n = (int)e->dp_rec.size();
    if (!out) return n;
    if (n && !e->dp_bwd_end) return fail("ss_dp_profile_read: no data-parallel step has run with the profile on");
    for (int i = 0; i < n && i < cap; ++i) {
        const auto& r = e->dp_rec[i];
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventSynchronize(e->dp_bwd_end) != hipSuccess) return fail("ss_dp_profile_read: event sync failed");
        float ta = 0, tb = 0;
        if (hipEventElapsedTime(&ta, e->dp_bwd_end, r.a) != hipSuccess || hipEventElapsedTime(&tb, e->dp_bwd_end, r.b) != hipSuccess)
            return fail("ss_dp_profile_read: elapsed time failed");
        out[4 * i + 0] = (double)r.off;
        out[4 * i + 1] = (double)r.count;
        out[4 * i + 2] = ta * 1e3;
        out[4 * i + 3] = tb * 1e3;
    }
    return n < cap ? n : cap;
}


}  // extern "C"
