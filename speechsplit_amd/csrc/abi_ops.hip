// Engine-free kernel hooks of the C ABI (include/speechsplit_amd.h): single GEMM / image / LSTM launches for the tests and tools/, the
// placement probes and ss_tune.  None of them takes an engine.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "abi.h"
#include "knobs.h"
#include "kernels.h"
#include "../../include/speechsplit_amd.h"

using namespace ss;

namespace ss {
int g_op_time_major = 0;   // experiment: ss_op_lstm_fwd / _bwd take time-major slabs [T+4, B, C] (persistent kernels only)
static unsigned* g_img_wq = nullptr;      // queue words (+ placement log) of the test hook's work-queue launches
constexpr long IMG_WQ_BYTES = 16 + 16 * 1024;
// see common.h: the last instance per kind, and every distinct one since ss_debug_last_variant("reset") (at most 64 per kind, first come)
static char g_last_variant[VARIANT_KINDS][64] = {"", "", ""};
static std::vector<std::string> g_seen_variants[VARIANT_KINDS];
void note_variant(int kind, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_variant[kind], sizeof g_last_variant[kind], fmt, ap);
    va_end(ap);
    std::vector<std::string>& seen = g_seen_variants[kind];
    for (const std::string& v : seen)
        if (v == g_last_variant[kind]) return;
    if (seen.size() < 64) seen.push_back(g_last_variant[kind]);
}
int g_img_xcc = 0;      // ss_op_gemm_img (test hook): run the image GEMM in its work-queue form on the XCDs of this mask
}

extern "C" {

int ss_op_gemm(const float* a, long lda, const float* b, long ldb, float* c, long ldc, const float* bias, int M, int N, int K,
               int flags, int ksplit, void* stream) {
    GemmDesc d{};
    d.A = {a, lda, 0, 0, 0};
    d.B = {b, ldb, 0, 0, 0};
    d.C = c;
    d.ldc = ldc;
    d.bias = bias;
    d.M = M;
    d.N = N;
    d.K = K;
    d.batch = 1;
    d.ksplit = ksplit < 1 ? 1 : ksplit;
    d.flags = (flags & 1 ? GEMM_TA : 0) | (flags & 2 ? GEMM_TB : 0) | (flags & 8 ? GEMM_BF16 : 0) | (flags & 16 ? GEMM_F16X2 : 0) | (d.ksplit > 1 ? GEMM_ACCUM : 0);
    HIPCHK(launch_gemm(d, S(stream)));
    return 0;
}

int ss_op_gemm_pre(const float* a, long lda, const float* a_img, const float* b, long ldb, const float* b_img, float* c, long ldc, float* part, int M,
                   int N, int K, int flags, int ksplit, void* stream) {
    if (!a || !b || !c) return fail("ss_op_gemm_pre: null pointer");
    GemmDesc d{};
    d.A = {a, lda, 0, 0, 0};
    d.B = {b, ldb, 0, 0, 0};
    d.a_pre = a_img;
    d.b_pre = b_img;
    d.C = c;
    d.ldc = ldc;
    d.M = M;
    d.N = N;
    d.K = K;
    d.batch = 1;
    d.ksplit = ksplit < 1 ? 1 : ksplit;
    d.part = part;
    d.want = 1;           // the largest tile the shape admits, whatever the number of workgroups: the form under test
    d.flags = (flags & 1 ? GEMM_TA : 0) | (flags & 2 ? GEMM_TB : 0) | GEMM_F16X2 | (d.ksplit > 1 ? GEMM_ACCUM : 0);
    HIPCHK(launch_gemm(d, S(stream)));
    return 0;
}

int ss_op_split_image(const float* src, long ld, long rows, int cols, float scale, float* img, long ldi, void* stream) {
    if (!src || !img) return fail("ss_op_split_image: null pointer");
    HIPCHK(split_image(src, ld, rows, cols, nullptr, scale, img, ldi, nullptr, S(stream)));
    return 0;
}

int ss_op_gemm_img(const float* a_img, long lda, const float* b_img, long ldb, float* c, long ldc, const float* bias, int M, int N, int K, int flags,
                   int ksplit, int cfg, float scale_a, float scale_b, int a_seglen, long a_segstride, float* part, const void* zeros, void* stream) {
    static float* sc = nullptr;           // the two scales as device words (test hook: one call at a time)
    if (!sc) HIPCHK(hipMalloc((void**)&sc, 256));
    const float h[2] = {scale_a, scale_b};
    HIPCHK(hipMemcpyAsync(sc, h, sizeof(h), hipMemcpyHostToDevice, S(stream)));
    ImgGemmDesc d{};
    d.A = {a_img, lda, 0, a_seglen, a_segstride};
    d.B = {b_img, ldb, 0, 0, 0};
    d.C = c;
    d.ldc = ldc;
    d.bias = bias;
    d.M = M;
    d.N = N;
    d.K = K;
    d.batch = 1;
    d.ksplit = ksplit < 1 ? 1 : ksplit;
    d.flags = (flags & 1 ? GEMM_TA : 0) | (flags & 2 ? GEMM_TB : 0) | (flags & 4 ? GEMM_ACCUM : 0);
    d.bf16 = (flags & 8) ? 1 : 0;           // single-piece form: the operands are plain bf16 matrices, ld in elements
    d.part = part;
    d.scale_a = d.bf16 ? nullptr : sc;
    d.scale_b = d.bf16 ? nullptr : sc + 1;
    d.zeros = zeros;
    d.cfg = cfg;
    d.diag = g_gemm_diag;
    if (g_img_xcc) {                      // test hook for the work-queue form: ss_tune("img_xcc", mask of allowed XCDs; 255 = queue without a filter)
        if (!g_img_wq) HIPCHK(hipMalloc((void**)&g_img_wq, IMG_WQ_BYTES));
        HIPCHK(hipMemsetAsync(g_img_wq, 0, (g_img_xcc & 0x100) ? IMG_WQ_BYTES : 8, S(stream)));
        d.wq = g_img_wq;
        d.xcc_allow = (unsigned)g_img_xcc;
    }
    if (!gemm_img_supported(d)) return fail("ss_op_gemm_img: shape / alignment not supported by the image GEMM");
    HIPCHK(launch_gemm_img(d, S(stream)));
    return 0;
}

// Descriptor-level test hooks: every field a product launch sets, handed to the launcher unchanged.  Every refusal is made before anything
// is enqueued.
int ss_op_gemm_desc(const ss_gemm_desc* g, void* stream) {
    if (!g) return fail("ss_op_gemm_desc: null descriptor");
    if (!g->a || !g->b || !g->c) return fail("ss_op_gemm_desc: null pointer (a, b and c are required)");
    if (g->M < 0 || g->N < 0 || g->K < 0 || g->batch < 0 || g->ksplit < 0 || g->want < 0 || g->a_seglen < 0 || g->b_seglen < 0)
        return fail("ss_op_gemm_desc: negative size");
    if (g->flags & ~(GEMM_TA | GEMM_TB | GEMM_ACCUM | GEMM_BF16 | GEMM_F16X2)) return fail("ss_op_gemm_desc: unknown flag");
    if (g->ksplit > 1 && !(g->flags & GEMM_ACCUM)) return fail("ss_op_gemm_desc: ksplit > 1 needs the accumulate flag (C zeroed or live)");
    if (g->row_period < 0 || (g->row_period > 0 && (g->row_off < 0 || g->row_lo < 0 || g->row_hi > g->row_period || g->row_lo > g->row_hi)))
        return fail("ss_op_gemm_desc: bad row mask");
    GemmDesc d{};
    d.A = {g->a, g->lda, g->a_bstride, g->a_seglen, g->a_segstride};
    d.B = {g->b, g->ldb, g->b_bstride, g->b_seglen, g->b_segstride};
    d.C = g->c;
    d.ldc = g->ldc;
    d.cstride = g->cstride;
    d.bias = g->bias;
    d.M = g->M;
    d.N = g->N;
    d.K = g->K;
    d.batch = g->batch;
    d.flags = g->flags;
    d.want = g->want;
    d.row_period = g->row_period;
    d.row_off = g->row_off;
    d.row_lo = g->row_lo;
    d.row_hi = g->row_hi;
    d.ksplit = g->ksplit < 1 ? 1 : g->ksplit;
    d.amax_a = g->amax_a;
    d.amax_b = g->amax_b;
    d.a_pre = g->a_pre;
    d.b_pre = g->b_pre;
    d.a_pre_scale = g->a_pre_scale;
    d.b_pre_scale = g->b_pre_scale;
    d.part = g->part;
    HIPCHK(launch_gemm(d, S(stream)));
    return 0;
}

int ss_op_gemm_img_desc(const ss_gemm_img_desc* g, void* stream) {
    if (!g) return fail("ss_op_gemm_img_desc: null descriptor");
    if (!g->a || !g->b || !g->c) return fail("ss_op_gemm_img_desc: null pointer (a, b and c are required)");
    if (g->M < 0 || g->N < 0 || g->K < 0 || g->batch < 0 || g->ksplit < 0 || g->a_seglen < 0 || g->b_seglen < 0 || g->rm_T < 0 || g->rm_TP < 0)
        return fail("ss_op_gemm_img_desc: negative size");
    if (g->flags & ~(GEMM_TA | GEMM_TB | GEMM_ACCUM)) return fail("ss_op_gemm_img_desc: unknown flag");
    if (g->ksplit > 1 && !g->part) return fail("ss_op_gemm_img_desc: ksplit > 1 needs part_dev");
    if (g->row_period < 0 || (g->row_period > 0 && (g->row_off < 0 || g->row_lo < 0 || g->row_hi > g->row_period || g->row_lo > g->row_hi)))
        return fail("ss_op_gemm_img_desc: bad row mask");
    if (g->rm_T > 0 && g->rm_TP < g->rm_T) return fail("ss_op_gemm_img_desc: rm_TP < rm_T");
    if (g->cfg < -1 || g->cfg > 3) return fail("ss_op_gemm_img_desc: cfg outside -1 .. 3");
    ImgGemmDesc d{};
    d.A = {g->a, g->lda, g->a_bstride, g->a_seglen, g->a_segstride};
    d.B = {g->b, g->ldb, g->b_bstride, g->b_seglen, g->b_segstride};
    d.C = g->c;
    d.ldc = g->ldc;
    d.cstride = g->cstride;
    d.bias = g->bias;
    d.M = g->M;
    d.N = g->N;
    d.K = g->K;
    d.batch = g->batch < 1 ? 1 : g->batch;
    d.ksplit = g->ksplit < 1 ? 1 : g->ksplit;
    d.flags = g->flags;
    d.row_period = g->row_period;
    d.row_off = g->row_off;
    d.row_lo = g->row_lo;
    d.row_hi = g->row_hi;
    d.rm_T = g->rm_T;
    d.rm_TP = g->rm_TP;
    d.part = g->part;
    d.bf16 = g->bf16 ? 1 : 0;
    d.scale_a = d.bf16 ? nullptr : g->scale_a;
    d.scale_b = d.bf16 ? nullptr : g->scale_b;
    d.zeros = g->zeros;
    d.cfg = g->cfg;
    if (!gemm_img_supported(d)) return fail("ss_op_gemm_img_desc: shape / alignment / option not supported by the image GEMM");
    HIPCHK(launch_gemm_img(d, S(stream)));
    return 0;
}

// Where do the workgroups of a launch go?  n_wg workgroups of `threads` threads and lds_bytes of LDS each record (XCC_ID register, HW_ID
// register) in launch order; each then idles `hold_ticks` (100 MHz) so that the whole grid has to be resident at once.
__global__ void xcc_map_kernel(unsigned* out, long long hold_ticks) {
    extern __shared__ unsigned char xcc_map_lds[];
    if (threadIdx.x == 0) {
        unsigned x, h;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(h));
        out[2 * blockIdx.x] = x;
        out[2 * blockIdx.x + 1] = h;
        xcc_map_lds[0] = (unsigned char)x;
    }
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < hold_ticks) __builtin_amdgcn_s_sleep(8);
}
int ss_debug_xcc_map(int n_wg, int threads, int lds_bytes, int hold_us, unsigned* out_dev, void* stream) {
    if (!out_dev || n_wg < 1 || threads < 64 || threads > 1024 || lds_bytes < 0 || lds_bytes > 160 * 1024 || hold_us < 0 || hold_us > 2000)
        return fail("ss_debug_xcc_map: bad arguments");
    if (lds_bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)xcc_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    hipLaunchKernelGGL(xcc_map_kernel, dim3(n_wg), dim3(threads), lds_bytes, S(stream), out_dev, (long long)hold_us * 100);
    HIPCHK(hipGetLastError());
    return 0;
}

int ss_debug_img_wq(unsigned* out_host, int words) {
    if (!out_host || words < 1 || words * 4L > IMG_WQ_BYTES || !g_img_wq) return fail("ss_debug_img_wq: nothing logged / bad size");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_host, g_img_wq, words * 4L, hipMemcpyDeviceToHost));
    return 0;
}

int ss_debug_gemm_phases(unsigned long long* out24, int reset) {
    if (!out24) return fail("ss_debug_gemm_phases: null pointer");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(gemm_phase_probe(out24, reset != 0));
    return 0;
}

int ss_debug_last_variant(const char* what, char* buf, int n) {
    static const char* const kinds[VARIANT_KINDS] = {"gemm", "lstm_step_fwd", "lstm_step_bwd"};
    const std::string w = what ? what : "";
    if (w == "reset") {      // forget everything: a text read after this was written by a launch made after it
        for (int k = 0; k < VARIANT_KINDS; ++k) {
            g_last_variant[k][0] = 0;
            g_seen_variants[k].clear();
        }
        return 0;
    }
    for (int k = 0; k < VARIANT_KINDS; ++k) {
        std::string text;
        if (w == kinds[k]) text = g_last_variant[k];
        else if (w == std::string(kinds[k]) + "_seen")
            for (const std::string& v : g_seen_variants[k]) text += v + "\n";
        else continue;
        if (buf && n > 0) {
            strncpy(buf, text.c_str(), n - 1);
            buf[n - 1] = 0;
        }
        return (int)text.size();
    }
    return fail("ss_debug_last_variant: unknown kind: " + w);
}

int ss_tune(const char* key, int value) {
    struct Key {
        const char* name;
        int* target;
        int lo, hi;      // accepted values: lo <= value <= hi
    };
    constexpr int MAXV = 0x7fffffff;
    static const Key keys[] = {
        {"lstm_nw", &g_lstm_nw, 4, 16},      // 4, 8 or 16 (checked below)
        {"lstm_g", &g_lstm_g, 0, 16},
#ifdef SS_DIAG
        {"lstm_mode", &g_lstm_mode, 0, 4},
        {"gemm_diag", &g_gemm_diag, 0, 2047},
        {"seq_prio", &g_seq_prio, 0, 65535},
#else
        {"seq_prio", &g_seq_prio, 0, 1},
#endif
        {"seq_tag", &g_seq_tag, 0, 1},
        {"op_time_major", &g_op_time_major, 0, 1},
        {"seq_var", &g_seq_var, 0, 15},
        {"compact0", &g_compact0, 0, 1},
        {"bf16_img", &g_bf16_img, 0, 1},
        {"dp_model", &g_dp_model, 0, 64},
        {"dp_buckets", &g_dp_buckets, 0, 1},
        {"gemm_ws", &g_gemm_ws, 0, 2},
        {"gemm_pipe", &g_gemm_pipe, 0, 1},
        {"seq_spin_log2", &g_seq_spin_log2, 0, 24},
        {"overlap", &g_overlap, 0, 1},
        {"defer_dw", &g_defer_dw, 0, 1},
        {"dx_batched", &g_dx_batched, 0, 2},
        {"small_lds", &g_small_lds, 0, 2},
        {"gemm_tr", &g_gemm_tr, 0, 2},
        {"own_streams", &g_own_streams, 0, 1},
        {"conv_dw_off", &g_conv_dw_off, 0, 3},
        {"dec_tail_split", &g_dec_tail_split, 0, 10},
        {"early_dw", &g_early_dw, 0, 1},
        {"xcd_dw", &g_xcd_dw, 0, 1},
        {"dp_emulate", &g_dp_emulate, 0, 1},
        {"gn_gather", &g_gn_gather, 0, 1},
        {"img_xcc", &g_img_xcc, 0, 511},      // bit 8: keep a placement log (ss_debug_img_wq)
        {"probe_queues", &g_probe_queues, 0, 1},
        {"prio_order", &g_prio_order, 0, 1},
        {"deterministic", &g_deterministic, 0, 1},
        {"persist", &g_persist, 0, 1},
        {"gemm_want", &g_gemm_want, 1, MAXV},
        {"gemm_mode", &g_gemm_mode, 0, 1},
        {"fwd_f16x2", &g_fwd_f16x2, 0, 1},
        {"bwd_f16x2", &g_bwd_f16x2, 0, 1},
    };
    const std::string k = key ? key : "";
    for (const Key& t : keys) {
        if (k != t.name) continue;
        if (value < t.lo || value > t.hi || (t.target == &g_lstm_nw && value != 4 && value != 8 && value != 16)) break;
        *t.target = value;
        return 0;
    }
    return fail("ss_tune: unknown key or bad value: " + k
#ifndef SS_DIAG
                     + " (the wrong-result timing modes lstm_mode / gemm_diag / seq_prio > 1 exist only in the -DSS_DIAG build: make diag)"
#endif
    );
}

static int op_lstm_fwd(float* gates, const float* whh_f, const float* whh_b, float* out, float* csave, float* scratch,
                       long scratch_floats, const int* len, int B, int T, int H, void* stream) {
    hipStream_t s = S(stream);
    if (H > 32) {
        const long half = 2L * (((B + 15) / 16) * 16) * H, wn = 2L * 4 * H * H;
        if (!scratch || scratch_floats < wn + 2 * half) return fail("ss_op_lstm_fwd: scratch too small");
        float* hf = scratch + wn;
        if (g_persist && lstm_seq_supported(B, H) && wn * 4 >= lstm_seq_xbytes(B, H, false)) {
            // exchange buffer in the (unused) packed-weight area, counters behind it
            HIPCHK(lstm_seq_fwd(gates, whh_f, whh_b, scratch, out, csave, (unsigned*)hf, B, T, H, s, {.time_major = g_op_time_major != 0, .len = len}));
            return 0;
        }
        HIPCHK(lstm_pack_w(whh_f, whh_b, scratch, H, 0, s));
        HIPCHK(hipMemsetAsync(hf, 0, 2 * half * 4, s));
        for (int st = 0; st < T; ++st)
            HIPCHK(lstm_step_fwd(gates, scratch, hf + (st & 1) * half, hf + ((st & 1) ^ 1) * half, out, csave, B, T, H, st, s, len));
    } else {
        HIPCHK(lstm_small_fwd(gates, whh_f, whh_b, out, csave, B, T, H, s, len));
    }
    return 0;
}

int ss_op_lstm_fwd(float* gates, const float* whh_f, const float* whh_b, float* out, float* csave, float* scratch,
                   long scratch_floats, int B, int T, int H, void* stream) {
    return op_lstm_fwd(gates, whh_f, whh_b, out, csave, scratch, scratch_floats, nullptr, B, T, H, stream);
}

int ss_op_lstm_fwd_ragged(float* gates, const float* whh_f, const float* whh_b, float* out, float* csave, float* scratch,
                          long scratch_floats, const int* len_dev, int B, int T, int H, void* stream) {
    if (!gates || !whh_f || !whh_b || !out || !csave || B < 1 || T < 1) return fail("ss_op_lstm_fwd_ragged: null pointer or empty shape");
    return op_lstm_fwd(gates, whh_f, whh_b, out, csave, scratch, scratch_floats, len_dev, B, T, H, stream);
}

int ss_op_lstm_bwd(float* gates, const float* whh_f, const float* whh_b, const float* d_out, const float* csave,
                   float* scratch, long scratch_floats, int B, int T, int H, void* stream) {
    hipStream_t s = S(stream);
    if (H > 32) {
        const long half = 2L * (((B + 15) / 16) * 16) * 4 * H, wn = 2L * 4 * H * H;
        if (!scratch || scratch_floats < wn + 2 * half + 2L * B * H) return fail("ss_op_lstm_bwd: scratch too small");
        float* gf = scratch + wn;
        float* dc = gf + 2 * half;
        const long xbytes = lstm_seq_xbytes(B, H, true);
        if (g_persist && lstm_seq_supported(B, H) && scratch_floats * 4 >= xbytes + 4L * LSTM_SEQ_SYNC_WORDS) {     // [exchange tiles][flags]
            HIPCHK(lstm_seq_bwd(gates, whh_f, whh_b, scratch, d_out, csave, (unsigned*)((char*)scratch + xbytes), B, T, H, s,
                                {.time_major = g_op_time_major != 0}));
            return 0;
        }
        HIPCHK(lstm_pack_w(whh_f, whh_b, scratch, H, 1, s));
        HIPCHK(hipMemsetAsync(gf, 0, 2 * half * 4, s));
        for (int st = 0; st < T; ++st)
            HIPCHK(lstm_step_bwd(gates, scratch, gf + (st & 1) * half, gf + ((st & 1) ^ 1) * half, d_out, csave, dc, B, T, H, st, s));
    } else {
        HIPCHK(lstm_small_bwd(gates, whh_f, whh_b, d_out, csave, B, T, H, s));
    }
    return 0;
}

// The persistent recurrences with every option the engine passes them (SeqFwd / SeqBwd, kernels.h) -- no fall-back to the per-step kernels:
// whatever the persistent kernels cannot run is refused before anything is enqueued.
static long op_seq_scratch_floats(int B, int H, bool backward) { return lstm_seq_xbytes(B, H, backward) / 4 + LSTM_SEQ_SYNC_WORDS; }
static bool misaligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) != 0; }

int ss_op_lstm_seq_fwd(float* gates, const float* whh_f, const float* whh_b, float* out, float* csave, float* scratch, long scratch_floats,
                       const float* xc, int xf, float* out_img, int img_bf16, int hi_only, const int* len, int B, int T, int H, void* stream) {
    if (!gates || !whh_f || !whh_b || !out || !csave || !scratch) return fail("ss_op_lstm_seq_fwd: null pointer");
    if (B < 1 || T < 1 || H < 1) return fail("ss_op_lstm_seq_fwd: empty shape");
    if (xc && (xf < 1 || T % xf != 0)) return fail("ss_op_lstm_seq_fwd: xc_dev needs xf >= 1 and T % xf == 0");
    if (misaligned(gates, 16) || misaligned(whh_f, 16) || misaligned(whh_b, 16) || misaligned(out, 16) || misaligned(csave, 16) || misaligned(xc, 16) ||
        misaligned(scratch, 16))
        return fail("ss_op_lstm_seq_fwd: an operand is not 16-byte aligned");
    if (out_img && !img_bf16 && misaligned(out_img, 32)) return fail("ss_op_lstm_seq_fwd: out_img_dev (format v2) is not 32-byte aligned");
    if (out_img && img_bf16 && misaligned(out_img, 8)) return fail("ss_op_lstm_seq_fwd: out_img_dev (bf16) is not 8-byte aligned");
    if (scratch_floats < op_seq_scratch_floats(B, H, false)) return fail("ss_op_lstm_seq_fwd: scratch too small");
    if (!lstm_seq_supported(B, H)) return fail("ss_op_lstm_seq_fwd: shape not supported by the persistent kernels");
    SeqFwd o{};
    o.xc = xc;
    o.xf = xc ? xf : 0;
    o.out_img = out_img;
    o.img_bf16 = out_img && img_bf16;
    o.hi_only = hi_only != 0;
    o.len = len;
    HIPCHK(lstm_seq_fwd(gates, whh_f, whh_b, scratch, out, csave, (unsigned*)((char*)scratch + lstm_seq_xbytes(B, H, false)), B, T, H, S(stream), o));
    return 0;
}

int ss_op_lstm_seq_bwd(float* gates, const float* whh_f, const float* whh_b, const float* d_out, const float* csave, float* scratch,
                       long scratch_floats, float* amax, float* gbias_f, float* gbias_b, float* dgs, int xf, float* dimg, int img_only, int hi_only,
                       int B, int T, int H, void* stream) {
    if (!gates || !whh_f || !whh_b || !d_out || !csave || !scratch) return fail("ss_op_lstm_seq_bwd: null pointer");
    if (B < 1 || T < 1 || H < 1) return fail("ss_op_lstm_seq_bwd: empty shape");
    if (dgs && (xf < 1 || T % xf != 0)) return fail("ss_op_lstm_seq_bwd: dgs_dev needs xf >= 1 and T % xf == 0");
    if (img_only && !dimg) return fail("ss_op_lstm_seq_bwd: img_only without dimg_dev");
    if (misaligned(gates, 16) || misaligned(whh_f, 16) || misaligned(whh_b, 16) || misaligned(d_out, 16) || misaligned(csave, 16) || misaligned(dgs, 16) ||
        misaligned(scratch, 16) || misaligned(amax, 4) || misaligned(gbias_f, 4) || misaligned(gbias_b, 4))
        return fail("ss_op_lstm_seq_bwd: an operand is not 16-byte aligned (amax_dev, gbias_*_dev: 4-byte)");
    if (dimg && misaligned(dimg, 8)) return fail("ss_op_lstm_seq_bwd: dimg_dev (bf16) is not 8-byte aligned");
    if (scratch_floats < op_seq_scratch_floats(B, H, true)) return fail("ss_op_lstm_seq_bwd: scratch too small");
    if (!lstm_seq_supported(B, H)) return fail("ss_op_lstm_seq_bwd: shape not supported by the persistent kernels");
    SeqBwd o{};
    o.amax = amax;
    o.gbias_f = gbias_f;
    o.gbias_b = gbias_b;
    o.dgs = dgs;
    o.xf = dgs ? xf : 0;
    o.dimg = dimg;
    o.img_only = img_only != 0;
    o.hi_only = hi_only != 0;
    HIPCHK(lstm_seq_bwd(gates, whh_f, whh_b, scratch, d_out, csave, (unsigned*)((char*)scratch + lstm_seq_xbytes(B, H, true)), B, T, H, S(stream), o));
    return 0;
}

int ss_op_lstm_wgrad(const float* dg, const float* x, long x_ld, const float* hout, float* gwih, float* gwhh, float* gb, float* scratch, long scratch_floats,
                     long R, int H, int In, void* stream) {
    if (H < 1 || H > 32 || In < 1 || R < 1) return fail("ss_op_lstm_wgrad: H in 1..32, In >= 1");
    WgradTable w{};
    w.n = 1;
    w.tiles_total = lstm_small_wgrad_tiles(H, In);
    w.row_groups = 16;
    const long need = (long)w.tiles_total * w.row_groups * 4096, ctr_floats = (w.tiles_total + 63) & ~63L;
    if (!scratch || scratch_floats < need + ctr_floats) return fail("ss_op_lstm_wgrad: scratch too small");
    w.part = scratch;
    w.ctr = (unsigned*)(scratch + need);
    HIPCHK(hipMemsetAsync(w.ctr, 0, ctr_floats * 4, S(stream)));
    // gwih [2][4H][In], gwhh [2][4H][H], gb [2][2][4H] (b_ih then b_hh per direction): accumulated into, as the engine's gradient arena is
    w.t[0] = WgradTask{dg, x, x_ld, hout, gwih, gwih + 4L * H * In, gwhh, gwhh + 4L * H * H, gb, gb + 4L * H, gb + 8L * H, gb + 12L * H, H, In, R, 0, 2 * H};
    HIPCHK(lstm_small_wgrad(w, S(stream)));
    return 0;
}

// The GroupNorm + ReLU family (elementwise.hip) on the CALLER's haloed slabs, every form and option the engine launches: the hooks call the
// launchers of kernels.h and nothing else -- no convolution, no engine, no copy.  Whatever a launcher would refuse, silently drop (the image
// of gn_relu_gather) or leave to its caller is refused here before anything is enqueued.
static const char* gn_rows_bad(const float* p, long ld, long bs, int C) {
    if (ld < C) return "row stride below C";
    if (ld % 4 || bs % 4) return "row / batch stride is not a multiple of 4 floats";
    if (misaligned(p, 16)) return "base is not 16-byte aligned";
    return nullptr;
}
#define GN_ROWS(who, name, p, ld, bs)                                                                    \
    if (const char* _m = gn_rows_bad(p, ld, bs, C)) return fail(std::string(who) + ": " + name + ": " + _m)

long ss_op_gn_relu_scratch(int B, int T, int C) {
    if (B < 1 || T < 1 || C < 64 || C % 64) return 0;
    return gn_relu_fwd_scratch_bytes(B, T, C);
}

int ss_op_gn_relu_fwd(const float* x, long x_ld, long x_bs, float* y, long y_ld, long y_bs, const float* gamma, const float* beta, float* stats,
                      const int* len, const int* i0, const float* lam, const int* nrows, int P, float* y_img, const float* img_scale, int img_bf16,
                      void* scratch, long scratch_bytes, int B, int T, int C, void* stream) {
    const char* who = "ss_op_gn_relu_fwd";
    if (!x || !y || !gamma || !beta || !stats) return fail("ss_op_gn_relu_fwd: null pointer");
    if (B < 1 || T < 1) return fail("ss_op_gn_relu_fwd: needs B >= 1 and T >= 1");
    if (C < 64 || C % 64) return fail("ss_op_gn_relu_fwd: needs C % 64 == 0");
    if (T > SS_MAX_EVAL_FRAMES) return fail("ss_op_gn_relu_fwd: T above SS_MAX_EVAL_FRAMES (8192)");
    const bool gather = i0 || lam || nrows;
    if (gather && !(i0 && lam && nrows)) return fail("ss_op_gn_relu_fwd: the gather form needs i0_dev, lam_dev and nrows_dev");
    if (gather && (P < 1 || P > 258)) return fail("ss_op_gn_relu_fwd: the gather form needs 1 <= P <= 258");
    if (gather && T > 256) return fail("ss_op_gn_relu_fwd: T > 256 runs the plain and ragged forms only (no gather)");
    if (gather && len) return fail("ss_op_gn_relu_fwd: len_dev and a plan exclude each other");
    if (y_img && !gather) return fail("ss_op_gn_relu_fwd: y_img_dev without a plan (only the gather form writes an image)");
    GN_ROWS(who, "x", x, x_ld, x_bs);
    GN_ROWS(who, "y", y, y_ld, y_bs);
    if (misaligned(gamma, 16) || misaligned(beta, 16) || misaligned(stats, 4) || misaligned(len, 4) || misaligned(i0, 4) || misaligned(lam, 4) ||
        misaligned(nrows, 4) || misaligned(img_scale, 4))
        return fail("ss_op_gn_relu_fwd: gamma_dev / beta_dev are not 16-byte aligned, or a word array is not 4-byte aligned");
    if (y_img) {
        if (y_ld % 8 || y_bs % 8) return fail("ss_op_gn_relu_fwd: y_img_dev needs y_ld % 8 == 0 and y_bs % 8 == 0");
        if (!img_bf16 && misaligned(y_img, 32)) return fail("ss_op_gn_relu_fwd: y_img_dev (format v2) is not 32-byte aligned");
        if (img_bf16 && misaligned(y_img, 16)) return fail("ss_op_gn_relu_fwd: y_img_dev (bf16) is not 16-byte aligned");
    }
    if (gather) {
        InterpPlan p{};
        p.P = P;
        p.T = T;
        p.i0 = const_cast<int*>(i0);
        p.lam = const_cast<float*>(lam);
        p.nrows = const_cast<int*>(nrows);
        GnGather o{};
        o.y_img = y_img ? reinterpret_cast<float*>(reinterpret_cast<char*>(y_img) + (long)HALO * y_ld * (img_bf16 ? 2 : 4)) : nullptr;
        o.img_scale = img_scale;
        o.img_bf16 = y_img && img_bf16;
        HIPCHK(gn_relu_gather(CRows{x + HALO * x_ld, x_ld, x_bs}, Rows{y + HALO * y_ld, y_ld, y_bs}, gamma, beta, stats, p, B, T, C, S(stream), o));
        return 0;
    }
    const long need = gn_relu_fwd_scratch_bytes(B, T, C);
    if (need && (!scratch || scratch_bytes < need)) return fail("ss_op_gn_relu_fwd: scratch too small (ss_op_gn_relu_scratch)");
    if (need && misaligned(scratch, 8)) return fail("ss_op_gn_relu_fwd: scratch_dev is not 8-byte aligned");
    HIPCHK(gn_relu_fwd(CRows{x + HALO * x_ld, x_ld, x_bs}, Rows{y + HALO * y_ld, y_ld, y_bs}, gamma, beta, stats, B, T, C, S(stream),
                       need ? static_cast<double*>(scratch) : nullptr, len));
    return 0;
}

int ss_op_gn_relu_mask(const float* x, long x_ld, long x_bs, const float* gamma, const float* beta, const float* stats, float* mask, int B, int T,
                       int C, void* stream) {
    if (!x || !gamma || !beta || !stats || !mask) return fail("ss_op_gn_relu_mask: null pointer");
    if (B < 1 || T < 1) return fail("ss_op_gn_relu_mask: needs B >= 1 and T >= 1");
    if (C < 64 || C % 64) return fail("ss_op_gn_relu_mask: needs C % 64 == 0");
    if (T > 256) return fail("ss_op_gn_relu_mask: T > 256 has no backward and no mask");
    GN_ROWS("ss_op_gn_relu_mask", "x", x, x_ld, x_bs);
    if (misaligned(gamma, 4) || misaligned(beta, 4) || misaligned(stats, 4) || misaligned(mask, 4))
        return fail("ss_op_gn_relu_mask: an operand is not 4-byte aligned");
    HIPCHK(gn_relu_mask(CRows{x + HALO * x_ld, x_ld, x_bs}, gamma, beta, stats, mask, B, T, C, S(stream)));
    return 0;
}

int ss_op_gn_relu_bwd(const float* x, long x_ld, long x_bs, float* dy, long dy_ld, long dy_bs, const float* gamma, const float* beta,
                      const float* stats, float* g_gamma, float* g_beta, float* g_bias, float* amax, float* part, const float* lam, const int* start,
                      int P, const float* src, long src_ld, long src_bs, float* dy_img, int B, int T, int C, void* stream) {
    const char* who = "ss_op_gn_relu_bwd";
    if (!x || !dy || !gamma || !beta || !stats || !g_gamma || !g_beta || !g_bias) return fail("ss_op_gn_relu_bwd: null pointer");
    if (B < 1 || T < 1) return fail("ss_op_gn_relu_bwd: needs B >= 1 and T >= 1");
    if (C < 64 || C % 64) return fail("ss_op_gn_relu_bwd: needs C % 64 == 0");
    if (T > 256) return fail("ss_op_gn_relu_bwd: T > 256 has no backward");
    const bool scatter = lam || start || src;
    if (scatter && !(lam && start && src)) return fail("ss_op_gn_relu_bwd: the scatter form needs lam_dev, start_dev and src_dev");
    if (scatter && (P < 1 || P > 258)) return fail("ss_op_gn_relu_bwd: the scatter form needs 1 <= P <= 258");
    GN_ROWS(who, "x", x, x_ld, x_bs);
    GN_ROWS(who, "dy", dy, dy_ld, dy_bs);
    if (scatter) GN_ROWS(who, "src", src, src_ld, src_bs);
    if (misaligned(gamma, 16) || misaligned(beta, 16) || misaligned(stats, 4) || misaligned(g_gamma, 4) || misaligned(g_beta, 4) ||
        misaligned(g_bias, 4) || misaligned(amax, 4) || misaligned(part, 4) || misaligned(lam, 4) || misaligned(start, 4))
        return fail("ss_op_gn_relu_bwd: gamma_dev / beta_dev are not 16-byte aligned, or a word array is not 4-byte aligned");
    if (dy_img && (dy_ld % 8 || dy_bs % 8)) return fail("ss_op_gn_relu_bwd: dy_img_dev needs dy_ld % 8 == 0 and dy_bs % 8 == 0");
    if (dy_img && misaligned(dy_img, 8)) return fail("ss_op_gn_relu_bwd: dy_img_dev (bf16) is not 8-byte aligned");
    InterpPlan p{};
    p.P = P;
    p.T = T;
    p.lam = const_cast<float*>(lam);
    p.start = const_cast<int*>(start);
    GnBwd o{};
    o.amax = amax;
    o.part = part;
    if (scatter) {
        o.scatter = &p;
        o.src = CRows{src + HALO * src_ld, src_ld, src_bs};
    }
    o.dy_img = dy_img;
    HIPCHK(gn_relu_bwd(CRows{x + HALO * x_ld, x_ld, x_bs}, Rows{dy + HALO * dy_ld, dy_ld, dy_bs}, gamma, beta, stats, g_gamma, g_beta, g_bias, B, T, C,
                       S(stream), o));
    return 0;
}
#undef GN_ROWS

// The kernels between the heavy families of a training step -- the two losses, the column sums, the decoder input with its gradient and the
// speaker-embedding contraction -- on the CALLER's views: the hooks hand (pointer, ld, bs) to the launchers of kernels.h and nothing else,
// no private copy.  Every refusal is made before anything is enqueued.
int ss_op_mse_loss(const float* out, long out_ld, long out_bs, const float* tgt, long tgt_ld, long tgt_bs, float* d_out, long d_ld, long d_bs, int B,
                   int T, int C, float grad_scale, float* partials, float* loss, void* stream) {
    if (!out || !tgt || !d_out || !partials || !loss) return fail("ss_op_mse_loss: null pointer");
    if (B < 1 || T < 1 || C < 1) return fail("ss_op_mse_loss: needs B >= 1, T >= 1 and C >= 1");
    if (out_ld < C || tgt_ld < C || d_ld < C) return fail("ss_op_mse_loss: row stride below C");
    HIPCHK(mse_loss(CRows{out, out_ld, out_bs}, CRows{tgt, tgt_ld, tgt_bs}, Rows{d_out, d_ld, d_bs}, B, T, C, grad_scale, partials, loss, S(stream)));
    return 0;
}

int ss_op_ce_loss(const float* logits, long ld, long bs, const int* tgt, float* d_out, long d_ld, long d_bs, int B, int T, int C, float grad_scale,
                  float* partials, float* loss, void* stream) {
    if (!logits || !tgt || !d_out || !partials || !loss) return fail("ss_op_ce_loss: null pointer");
    if (B < 1 || T < 1 || C < 1) return fail("ss_op_ce_loss: needs B >= 1, T >= 1 and C >= 1");
    if (ld < C || d_ld < C) return fail("ss_op_ce_loss: row stride below C");
    HIPCHK(ce_loss(CRows{logits, ld, bs}, tgt, Rows{d_out, d_ld, d_bs}, B, T, C, grad_scale, partials, loss, S(stream)));
    return 0;
}

long ss_op_colsum_scratch_doubles(int cols) { return cols < 1 ? 0 : colsum_scratch_doubles(cols); }

int ss_op_colsum(const float* in, long ld, int R, int C, int two_dir, float* o0, float* o1, float* o2, float* o3, double* part, long part_doubles,
                 unsigned* ctr, int ctr_words, void* stream) {
    if (!in || !o0) return fail("ss_op_colsum: null pointer (in_dev and o0_dev are required)");
    if (R < 1 || C < 1 || C > (1 << 24)) return fail("ss_op_colsum: needs R >= 1 and 1 <= C <= 2^24");
    if (two_dir && !o2) return fail("ss_op_colsum: the two-direction form needs o2_dev");
    if (!two_dir && (o1 || o2 || o3)) return fail("ss_op_colsum: the single-direction form writes o0_dev only (o1_dev .. o3_dev must be NULL)");
    const int cols = two_dir ? 2 * C : C;
    if (ld < cols) return fail("ss_op_colsum: row stride below the number of columns");
    if ((part == nullptr) != (ctr == nullptr)) return fail("ss_op_colsum: part_dev and ctr_dev come together (both NULL: the single-chunk form)");
    if (part) {
        if (part_doubles < colsum_scratch_doubles(cols)) return fail("ss_op_colsum: part_dev too small (ss_op_colsum_scratch_doubles)");
        if (ctr_words < (cols + 63) / 64) return fail("ss_op_colsum: fewer than ceil(cols / 64) counters");
        if (misaligned(part, 8) || misaligned(ctr, 4)) return fail("ss_op_colsum: part_dev is not 8-byte aligned or ctr_dev not 4-byte aligned");
    }
    if (two_dir) HIPCHK(colsum_bias(in, ld, R, C, o0, o1, o2, o3, part, ctr, S(stream)));
    else HIPCHK(colsum_acc(in, ld, R, C, o0, part, ctr, S(stream)));
    return 0;
}

// what dec_in_from_codes refuses (T % freq, columns beyond ld, compact with a freq != f), for slab sources, plus ld_i < 2 H_i
static const char* dec_in_bad(const ss_code_src* src, int nsrc, int max_src, bool backward, const float* emb, int emb_dim, int emb_col, const float* io,
                              int ld, int B, int T, int f) {
    if (!src || !io) return "null pointer";
    if (nsrc < 1 || nsrc > max_src) return "number of sources out of range";
    if (B < 1 || T < 1 || ld < 1) return "needs B >= 1, T >= 1 and ld >= 1";
    if (f < 0 || (f && T % f)) return "f must be 0 (slab form) or a divisor of T (compact form)";
    if (emb_dim < 0 || emb_col < 0 || (emb_dim && !emb && !backward)) return "bad speaker columns, or emb_dim > 0 without emb_dev";
    if ((long)emb_col + emb_dim > ld) return "speaker columns beyond ld";
    for (int i = 0; i < nsrc; ++i) {
        const ss_code_src& c = src[i];
        if (backward ? !c.d_o : !c.o) return "a source's slab pointer is null";
        if (c.H < 1 || c.freq < 1 || c.col < 0) return "a source needs H >= 1, freq >= 1 and col >= 0";
        if (T % c.freq) return "T is not a multiple of a source's freq";
        if ((long)c.col + 2L * c.H > ld) return "a source's columns lie beyond ld";
        if (c.ld < 2L * c.H) return "a source's row stride is below 2 H";
        if (f && c.freq != f) return "the compact form needs every source's freq == f";
    }
    return nullptr;
}
static void code_srcs(const ss_code_src* src, int nsrc, CodeSrc* out) {
    for (int i = 0; i < nsrc; ++i) out[i] = CodeSrc{src[i].o, src[i].d_o, src[i].H, src[i].freq, src[i].col, src[i].ld};
}

int ss_op_dec_in(const ss_code_src* src, int nsrc, const float* emb, int emb_dim, int emb_col, float* dst, int ld, int B, int T, int f, void* stream) {
    if (const char* m = dec_in_bad(src, nsrc, 4, false, emb, emb_dim, emb_col, dst, ld, B, T, f)) return fail(std::string("ss_op_dec_in: ") + m);
    CodeSrc cs[4];
    code_srcs(src, nsrc, cs);
    if (f) HIPCHK(build_dec_in_compact(cs, nsrc, emb, emb_dim, emb_col, dst, ld, B, T, f, S(stream)));
    else HIPCHK(build_dec_in(cs, nsrc, emb, emb_dim, emb_col, dst, ld, B, T, S(stream)));
    return 0;
}

int ss_op_dec_in_grad(const ss_code_src* src, int nsrc, const float* d_in, int ld, int B, int T, int f, void* stream) {
    if (const char* m = dec_in_bad(src, nsrc, 4, true, nullptr, 0, 0, d_in, ld, B, T, f)) return fail(std::string("ss_op_dec_in_grad: ") + m);
    CodeSrc cs[4];
    code_srcs(src, nsrc, cs);
    if (f) HIPCHK(dec_in_grad_compact(cs, nsrc, d_in, ld, B, T, f, S(stream)));
    else HIPCHK(dec_in_grad(cs, nsrc, d_in, ld, B, T, S(stream)));
    return 0;
}

int ss_op_dec_in_codes_grad(const ss_code_src* src, int nsrc, const float* d_in, int ld, int B, int T, int f, void* stream) {
    if (const char* m = dec_in_bad(src, nsrc, 3, true, nullptr, 0, 0, d_in, ld, B, T, f)) return fail(std::string("ss_op_dec_in_codes_grad: ") + m);
    CodeGrad cg[3];
    for (int i = 0; i < nsrc; ++i) cg[i] = CodeGrad{src[i].d_o, src[i].H, src[i].freq, src[i].col};      // d_o: the DENSE code gradient here
    HIPCHK(dec_in_codes_grad(cg, nsrc, d_in, ld, B, T, f, S(stream)));
    return 0;
}

int ss_op_dec_in_codes(const ss_code_src* src, int nsrc, const float* emb, int emb_dim, int emb_col, float* codes, long codes_floats, float* dst, int ld,
                       int B, int T, int f, void* stream) {
    if (const char* m = dec_in_bad(src, nsrc, 3, false, emb, emb_dim, emb_col, dst, ld, B, T, f)) return fail(std::string("ss_op_dec_in_codes: ") + m);
    long need = 0;
    for (int i = 0; i < nsrc; ++i) need += ((long)B * (T / src[i].freq) * 2 * src[i].H + 3) / 4 * 4;
    if (!codes || codes_floats < need || misaligned(codes, 16)) return fail("ss_op_dec_in_codes: codes_dev too small or not 16-byte aligned");
    CodeOut co[3];
    CodeIn ci[3];
    float* p = codes;
    for (int i = 0; i < nsrc; ++i) {
        co[i] = CodeOut{src[i].o, p, src[i].H, src[i].freq, src[i].ld, 0};
        ci[i] = CodeIn{p, src[i].H, src[i].freq, src[i].col};
        p += ((long)B * (T / src[i].freq) * 2 * src[i].H + 3) / 4 * 4;
    }
    HIPCHK(export_codes(co, nsrc, B, T, S(stream)));
    HIPCHK(dec_in_from_codes(ci, nsrc, emb, emb_dim, emb_col, dst, ld, B, T, f, S(stream)));
    return 0;
}

int ss_op_spk_grad(const float* dg, long ld, long b_stride, int rows, const float* w_f, const float* w_r, long w_ld, int col0, int H4, int E, float* out,
                   int B, void* stream) {
    if (!dg || !w_f || !w_r || !out) return fail("ss_op_spk_grad: null pointer");
    if (E < 1 || E > 1024 || H4 < 1 || rows < 1 || B < 1 || col0 < 0 || b_stride < 0) return fail("ss_op_spk_grad: needs 1 <= E <= 1024, H4 >= 1, rows >= 1, B >= 1, col0 >= 0");
    if ((2L * H4 + (1024 / E) * E) * 4 > 64 * 1024) return fail("ss_op_spk_grad: 2 H4 + floor(1024 / E) E floats exceed 64 KiB of LDS");
    if (ld < 2L * H4) return fail("ss_op_spk_grad: row stride below 2 H4");
    if (w_ld < (long)col0 + E) return fail("ss_op_spk_grad: w_ld below col0 + E");
    HIPCHK(spk_grad(dg, ld, b_stride, rows, w_f, w_r, w_ld, col0, H4, E, out, B, S(stream)));
    return 0;
}

// lstm_small_wgrad as the engine launches it: a table of tasks, each with its own H, In, R and strides, the caller's row_groups, scratch and
// counters.  The table's tiles are laid out task after task (tile0), as the engine's table is.
static const char* wgrad_table_bad(const ss_wgrad_task* t, int n, int row_groups, long* tiles_out) {
    if (!t) return "null pointer";
    if (n < 1 || n > WGRAD_MAX) return "number of tasks out of range (1 .. 8)";
    if (row_groups < 1 || row_groups > 1024) return "row_groups outside 1 .. 1024";
    long tiles = 0;
    for (int i = 0; i < n; ++i) {
        const ss_wgrad_task& k = t[i];
        if (!k.dg || !k.x || !k.hout || !k.gwih || !k.gwhh || !k.gb) return "a task's pointer is null";
        if (k.H < 1 || k.H > 32 || k.In < 1 || k.R < 1) return "a task needs H in 1 .. 32, In >= 1 and R >= 1";
        if (k.x_ld < k.In) return "a task's x_ld is below In";
        if (k.h_ld < 2L * k.H || k.h_ld > (1L << 30)) return "a task's h_ld is below 2 H";
        if (misaligned(k.dg, 16)) return "a task's dg is not 16-byte aligned";
        if (misaligned(k.x, 4) || misaligned(k.hout, 4) || misaligned(k.gwih, 4) || misaligned(k.gwhh, 4) || misaligned(k.gb, 4))
            return "a task's operand is not 4-byte aligned";
        tiles += lstm_small_wgrad_tiles(k.H, k.In);
    }
    if (tiles > 65535) return "more than 65535 tiles";
    *tiles_out = tiles;
    return nullptr;
}

long ss_op_lstm_wgrad_table_floats(const ss_wgrad_task* t, int n, int row_groups) {
    long tiles = 0;
    return wgrad_table_bad(t, n, row_groups, &tiles) ? 0 : tiles * row_groups * 4096;
}

int ss_op_lstm_wgrad_table_counters(const ss_wgrad_task* t, int n) {
    long tiles = 0;
    return wgrad_table_bad(t, n, 1, &tiles) ? 0 : (int)tiles;
}

int ss_op_lstm_wgrad_table(const ss_wgrad_task* t, int n, int row_groups, float* part, long part_floats, unsigned* ctr, int ctr_words, void* stream) {
    long tiles = 0;
    if (const char* m = wgrad_table_bad(t, n, row_groups, &tiles)) return fail(std::string("ss_op_lstm_wgrad_table: ") + m);
    if (!part || part_floats < tiles * row_groups * 4096) return fail("ss_op_lstm_wgrad_table: part_dev too small (ss_op_lstm_wgrad_table_floats)");
    if (!ctr || ctr_words < tiles) return fail("ss_op_lstm_wgrad_table: fewer counters than tiles (ss_op_lstm_wgrad_table_counters)");
    if (misaligned(part, 16) || misaligned(ctr, 4)) return fail("ss_op_lstm_wgrad_table: part_dev is not 16-byte aligned or ctr_dev not 4-byte aligned");
    WgradTable w{};
    w.n = n;
    w.row_groups = row_groups;
    w.part = part;
    w.ctr = ctr;
    int tile0 = 0;
    for (int i = 0; i < n; ++i) {
        const ss_wgrad_task& k = t[i];
        const long H = k.H;
        w.t[i] = WgradTask{k.dg, k.x, k.x_ld, k.hout, k.gwih, k.gwih + 4 * H * k.In, k.gwhh, k.gwhh + 4 * H * H, k.gb, k.gb + 4 * H, k.gb + 8 * H, k.gb + 12 * H,
                           k.H, k.In, k.R, tile0, (int)k.h_ld};
        tile0 += lstm_small_wgrad_tiles(k.H, k.In);
    }
    w.tiles_total = tile0;
    HIPCHK(lstm_small_wgrad(w, S(stream)));
    return 0;
}

// The random-resampling kernels (interp.hip) on the CALLER's memory, plan and value path apart: the hooks hand their arguments to
// interp_plan / interp_gather / interp_quant / interp_scatter and nothing else.  What the launchers refuse (P above 512, ncand above 64),
// silently drop (interp_gather's image when its alignment rule fails) or leave to the caller is refused here before anything is enqueued.
int ss_op_interp_plan(const float* scales, const int* len_seg, const int* len_seq, int len_seq_const, int n_seg, int ncand, int P, int T, int B,
                      int* i0, float* lam, int* nrows, int* counts, int* start, void* stream) {
    if (!scales || !len_seg || !i0 || !lam || !nrows || !counts || !start) return fail("ss_op_interp_plan: null pointer");
    if (B < 1 || n_seg < 1 || T < 1) return fail("ss_op_interp_plan: needs B >= 1, S >= 1 and T >= 1");
    if (ncand < 1 || ncand > 64) return fail("ss_op_interp_plan: ncand outside 1 .. 64");
    if (P < 1 || P > 512) return fail("ss_op_interp_plan: P outside 1 .. 512");
    if (!len_seq && (len_seq_const < 0 || len_seq_const > T)) return fail("ss_op_interp_plan: len_seq_const outside 0 .. T");
    if (misaligned(scales, 4) || misaligned(len_seg, 4) || misaligned(len_seq, 4) || misaligned(i0, 4) || misaligned(lam, 4) || misaligned(nrows, 4) ||
        misaligned(counts, 4) || misaligned(start, 4))
        return fail("ss_op_interp_plan: a word array is not 4-byte aligned");
    InterpPlan p{n_seg, ncand, P, T, i0, lam, nrows, counts, start};
    HIPCHK(interp_plan(p, scales, len_seg, len_seq, len_seq_const, B, S(stream)));
    return 0;
}

static const char* plan_rows_bad(const void* a, const void* b, const void* c, int P, int B) {
    if (!a || !b || !c) return "null pointer";
    if (B < 1 || B > 65535) return "B outside 1 .. 65535";
    if (P < 1 || P > 65535) return "P outside 1 .. 65535";
    if (misaligned(a, 4) || misaligned(b, 4) || misaligned(c, 4)) return "a word array is not 4-byte aligned";
    return nullptr;
}

int ss_op_interp_gather(const int* i0, const float* lam, const int* nrows, int P, const float* x, long x_ld, long x_bs, float* y, long y_ld, long y_bs,
                        int C, int B, float* y_img, const float* img_scale, void* stream) {
    if (const char* m = plan_rows_bad(i0, lam, nrows, P, B)) return fail(std::string("ss_op_interp_gather: ") + m);
    if (!x || !y) return fail("ss_op_interp_gather: null pointer");
    if (C < 1 || x_ld < C || y_ld < C) return fail("ss_op_interp_gather: needs C >= 1 and row strides of at least C");
    if (misaligned(x, 4) || misaligned(y, 4) || misaligned(img_scale, 4)) return fail("ss_op_interp_gather: an operand is not 4-byte aligned");
    if (img_scale && !y_img) return fail("ss_op_interp_gather: img_scale_dev without y_img_dev");
    if (y_img && (C % 8 || x_ld % 4 || y_ld % 8 || x_bs % 4 || y_bs % 8 || misaligned(x, 16) || misaligned(y, 16) || misaligned(y_img, 32)))
        return fail("ss_op_interp_gather: y_img_dev needs C % 8 == 0, x_ld % 4 == 0, x_bs % 4 == 0, y_ld % 8 == 0, y_bs % 8 == 0, x_dev and y_dev 16-byte "
                    "aligned and y_img_dev 32-byte aligned (the launcher would drop the image)");
    InterpPlan p{};
    p.P = P;
    p.i0 = const_cast<int*>(i0);
    p.lam = const_cast<float*>(lam);
    p.nrows = const_cast<int*>(nrows);
    HIPCHK(interp_gather(p, CRows{x, x_ld, x_bs}, Rows{y, y_ld, y_bs}, C, B, S(stream), y_img, img_scale));
    return 0;
}

int ss_op_interp_quant(const int* i0, const float* lam, const int* nrows, int P, int T, const float* mel, const float* f0, int CM, float* ymel,
                       long ym_ld, long ym_bs, float* yoh, long yo_ld, long yo_bs, int NOH, int* qidx, int B, void* stream) {
    if (const char* m = plan_rows_bad(i0, lam, nrows, P, B)) return fail(std::string("ss_op_interp_quant: ") + m);
    if (!mel || !f0 || !ymel || !yoh || !qidx) return fail("ss_op_interp_quant: null pointer");
    if (T < 2 || CM < 1 || NOH < 2) return fail("ss_op_interp_quant: needs T >= 2, CM >= 1 and NOH >= 2");
    if (ym_ld < CM || yo_ld < NOH) return fail("ss_op_interp_quant: row stride below CM (ymel) or below NOH (yoh)");
    if (misaligned(mel, 4) || misaligned(f0, 4) || misaligned(ymel, 4) || misaligned(yoh, 4) || misaligned(qidx, 4))
        return fail("ss_op_interp_quant: an operand is not 4-byte aligned");
    InterpPlan p{};
    p.P = P;
    p.T = T;
    p.i0 = const_cast<int*>(i0);
    p.lam = const_cast<float*>(lam);
    p.nrows = const_cast<int*>(nrows);
    HIPCHK(interp_quant(p, mel, f0, CM, Rows{ymel, ym_ld, ym_bs}, Rows{yoh, yo_ld, yo_bs}, NOH, qidx, B, S(stream)));
    return 0;
}

int ss_op_interp_scatter(const float* lam, const int* start, int P, int T, const float* dy, long dy_ld, long dy_bs, float* dx, long dx_ld, long dx_bs,
                         int C, int B, void* stream) {
    if (const char* m = plan_rows_bad(lam, start, dy, P, B)) return fail(std::string("ss_op_interp_scatter: ") + m);
    if (!dx) return fail("ss_op_interp_scatter: null pointer");
    if (T < 1 || C < 1 || dy_ld < C || dx_ld < C) return fail("ss_op_interp_scatter: needs T >= 1, C >= 1 and row strides of at least C");
    if (misaligned(dx, 4)) return fail("ss_op_interp_scatter: an operand is not 4-byte aligned");
    InterpPlan p{};
    p.P = P;
    p.T = T;
    p.lam = const_cast<float*>(lam);
    p.start = const_cast<int*>(start);
    HIPCHK(interp_scatter(p, CRows{dy, dy_ld, dy_bs}, Rows{dx, dx_ld, dx_bs}, C, B, S(stream)));
    return 0;
}

// The re-layout and guard kernels (elementwise.hip, input_grads.hip) on the CALLER's memory: weight packs and their images, gradient unpacks,
// the parameter prep table, transpose, row copies, the activation scales and the parameter guard.  Each hook calls its launcher and nothing
// else; what the launcher would refuse, silently drop (an image whose alignment rule fails) or leave to its caller is refused here first.
// an image of `n` elements beside its fp32 tensor: format v2 is written in whole groups of 8 from a 32-byte aligned base, bf16 8 bytes at a time
static const char* img_bad(const float* img, long n, int img_bf16) {
    if (!img) return nullptr;
    if (img_bf16) return misaligned(img, 8) ? "a bf16 image is not 8-byte aligned" : nullptr;
    if (n % 8) return "a format-v2 image needs an element count that is a multiple of 8";
    return misaligned(img, 32) ? "a format-v2 image is not 32-byte aligned" : nullptr;
}
static const char* conv_pack_bad(const float* w, int Co, int Ci, int Cp, const float* wf, const float* wb, const float* wf_img, const float* wb_img,
                                 int img_bf16) {
    if (!w || !wf) return "null pointer (w and wf are required)";
    if (Co < 1 || Ci < 1 || Cp < 1) return "needs Co >= 1, Ci >= 1 and Cp >= 1";
    if (Co % 4 || Cp % 4) return "needs Co % 4 == 0 and Cp % 4 == 0";
    if (Cp < Ci) return "Cp below Ci";
    if (wb_img && !wb) return "wb_img without wb";
    if (misaligned(w, 4) || misaligned(wf, 16) || misaligned(wb, 16)) return "w is not 4-byte aligned, or wf / wb not 16-byte aligned";
    if (const char* m = img_bad(wf_img, (long)Co * 5 * Cp, img_bf16)) return m;
    return img_bad(wb_img, (long)Ci * 5 * Co, img_bf16);
}

int ss_op_conv_pack(const float* w, int Co, int Ci, int Cp, float* wf, float* wb, float* wf_img, float* wb_img, int img_bf16, void* stream) {
    if (const char* m = conv_pack_bad(w, Co, Ci, Cp, wf, wb, wf_img, wb_img, img_bf16)) return fail(std::string("ss_op_conv_pack: ") + m);
    HIPCHK(conv_pack(w, Co, Ci, Cp, wf, wb, wf_img, wb_img, S(stream), img_bf16 != 0));
    return 0;
}

int ss_op_conv_pack_many(const ss_conv_pack_task* t, int n, int img_bf16, void* stream) {
    if (!t) return fail("ss_op_conv_pack_many: null pointer");
    if (n < 1 || n > 8) return fail("ss_op_conv_pack_many: number of tasks out of range (1 .. 8)");
    ConvPackTable tb{};
    tb.n = n;
    tb.img_bf16 = img_bf16 != 0;
    for (int i = 0; i < n; ++i) {
        if (const char* m = conv_pack_bad(t[i].w, t[i].Co, t[i].Ci, t[i].Cp, t[i].wf, t[i].wb, t[i].wf_img, t[i].wb_img, img_bf16))
            return fail(std::string("ss_op_conv_pack_many: ") + m);
        tb.t[i] = ConvPackTask{t[i].w, t[i].wf, t[i].wb, t[i].wf_img, t[i].wb_img, t[i].Co, t[i].Ci, t[i].Cp};
    }
    HIPCHK(conv_pack_many(tb, S(stream)));
    return 0;
}

int ss_op_conv_pack_dx(const float* w, int Co, int Ci, float* wb, void* stream) {
    if (!w || !wb) return fail("ss_op_conv_pack_dx: null pointer");
    if (Co < 1 || Ci < 1) return fail("ss_op_conv_pack_dx: needs Co >= 1 and Ci >= 1");
    if (misaligned(w, 4) || misaligned(wb, 4)) return fail("ss_op_conv_pack_dx: an operand is not 4-byte aligned");
    HIPCHK(conv_pack_dx(w, Co, Ci, wb, S(stream)));
    return 0;
}

static const char* conv_unpack_bad(const float* gp, int Co, int Ci, int Cp, const float* g) {
    if (!gp || !g) return "null pointer";
    if (Co < 1 || Ci < 1 || Cp < 1) return "needs Co >= 1, Ci >= 1 and Cp >= 1";
    if (Cp < Ci) return "Cp below Ci";
    if (misaligned(gp, 4) || misaligned(g, 4)) return "an operand is not 4-byte aligned";
    return nullptr;
}

int ss_op_conv_unpack(const float* gp, int Co, int Ci, int Cp, float* g, int acc, void* stream) {
    if (const char* m = conv_unpack_bad(gp, Co, Ci, Cp, g)) return fail(std::string("ss_op_conv_unpack: ") + m);
    HIPCHK(conv_unpack_grad(gp, Co, Ci, Cp, g, S(stream), acc != 0));
    return 0;
}

int ss_op_conv_unpack_many(const ss_conv_unpack_task* t, int n, int acc, void* stream) {
    if (!t) return fail("ss_op_conv_unpack_many: null pointer");
    if (n < 1 || n > CONV_UNPACK_MAX) return fail("ss_op_conv_unpack_many: number of tasks out of range (1 .. 8)");
    ConvUnpackTable tb{};
    tb.n = n;
    for (int i = 0; i < n; ++i) {
        if (const char* m = conv_unpack_bad(t[i].gp, t[i].Co, t[i].Ci, t[i].Cp, t[i].g)) return fail(std::string("ss_op_conv_unpack_many: ") + m);
        tb.t[i] = ConvUnpackTask{t[i].gp, t[i].g, t[i].Co, t[i].Ci, t[i].Cp};
    }
    HIPCHK(conv_unpack_grads(tb, S(stream), acc != 0));
    return 0;
}

int ss_op_prep(const ss_prep_task* t, int n, int img_bf16, void* stream) {
    if (!t) return fail("ss_op_prep: null pointer");
    if (n < 1 || n > PREP_MAX) return fail("ss_op_prep: number of tasks out of range (1 .. 48)");
    PrepTable tb{};
    tb.n = n;
    tb.img_bf16 = img_bf16 != 0;
    for (int i = 0; i < n; ++i) {
        const ss_prep_task& k = t[i];
        if (!k.a || !k.dst) return fail("ss_op_prep: a task's a or dst is null");
        if (k.n < 1) return fail("ss_op_prep: a task needs n >= 1");
        if (misaligned(k.a, 4) || misaligned(k.b, 4) || misaligned(k.dst, 4)) return fail("ss_op_prep: an operand is not 4-byte aligned");
        if (k.img) {     // the kernel writes the image on its float4 path only
            if (k.n % 4 || misaligned(k.a, 16) || misaligned(k.b, 16) || misaligned(k.dst, 16))
                return fail("ss_op_prep: a task with an image needs n % 4 == 0 and a, b, dst 16-byte aligned");
            if (const char* m = img_bad(k.img, k.n, img_bf16)) return fail(std::string("ss_op_prep: ") + m);
        }
        tb.t[i] = PrepTask{k.a, k.b, k.dst, k.n, k.img};
    }
    HIPCHK(prep_run(tb, S(stream)));
    return 0;
}

int ss_op_transpose(const float* in, int R, int C, float* out, void* stream) {
    if (!in || !out) return fail("ss_op_transpose: null pointer");
    if (R < 1 || C < 1) return fail("ss_op_transpose: needs R >= 1 and C >= 1");
    if (R > 65535 * 32) return fail("ss_op_transpose: R above 65535 * 32 (the row tiles are the grid's y dimension)");
    if (misaligned(in, 4) || misaligned(out, 4)) return fail("ss_op_transpose: an operand is not 4-byte aligned");
    HIPCHK(transpose2d(in, R, C, out, S(stream)));
    return 0;
}

int ss_op_copy_rows(const float* src, long s_ld, long s_bs, float* dst, long d_ld, long d_bs, const int* len, int B, int T, int C, void* stream) {
    if (!src || !dst) return fail("ss_op_copy_rows: null pointer");
    if (B < 1 || B > 65535 || T < 1 || C < 1) return fail("ss_op_copy_rows: needs 1 <= B <= 65535, T >= 1 and C >= 1");
    if (s_ld < C || d_ld < C) return fail("ss_op_copy_rows: row stride below C");
    if (misaligned(src, 4) || misaligned(dst, 4) || misaligned(len, 4)) return fail("ss_op_copy_rows: an operand is not 4-byte aligned");
    HIPCHK(copy_rows(CRows{src, s_ld, s_bs}, Rows{dst, d_ld, d_bs}, B, T, C, S(stream), len));
    return 0;
}

int ss_op_act_scales(const float* const* gamma, const float* const* beta, const int* C, int n, int T, float* out, void* stream) {
    if (!gamma || !beta || !C || !out) return fail("ss_op_act_scales: null pointer");
    if (n < 1 || n > ACT_SCALE_MAX) return fail("ss_op_act_scales: number of blocks out of range (1 .. 8)");
    if (T < 1) return fail("ss_op_act_scales: needs T >= 1");
    if (misaligned(out, 4)) return fail("ss_op_act_scales: out_dev is not 4-byte aligned");
    ActScaleTable tb{};
    tb.n = n;
    for (int i = 0; i < n; ++i) {
        if (C[i] < 0) return fail("ss_op_act_scales: a block's C is negative");
        if (C[i] && (!gamma[i] || !beta[i])) return fail("ss_op_act_scales: a block with C > 0 needs gamma and beta");
        if (misaligned(gamma[i], 4) || misaligned(beta[i], 4)) return fail("ss_op_act_scales: gamma / beta is not 4-byte aligned");
        tb.gamma[i] = gamma[i];
        tb.beta[i] = beta[i];
        tb.C[i] = C[i];
    }
    HIPCHK(act_scales(tb, T, out, S(stream)));
    return 0;
}

int ss_op_param_guard(const float* p, long n, float limit, unsigned* sticky, void* stream) {
    if (!p || !sticky) return fail("ss_op_param_guard: null pointer");
    if (n < 4 || n % 4) return fail("ss_op_param_guard: n must be a positive multiple of 4");
    if (misaligned(p, 16) || misaligned(sticky, 4)) return fail("ss_op_param_guard: p_dev is not 16-byte aligned or sticky_dev not 4-byte aligned");
    HIPCHK(param_guard(p, n, limit, sticky, S(stream)));
    return 0;
}

int ss_op_optim_ext(const ss_optim_ext_op* o, void* stream) {
    if (!o || !o->p || !o->state) return fail("ss_op_optim_ext: null pointer (the descriptor, p and state are required)");
    if (o->mode < 0 || o->mode > 2) return fail("ss_op_optim_ext: mode must be 0 (optimiser step), 1 (ema_range) or 2 (arena_swap)");
    if (o->lo < 0 || o->hi < o->lo || o->lo % 4 || o->hi % 4) return fail("ss_op_optim_ext: lo and hi must be multiples of 4 with 0 <= lo <= hi");
    if (misaligned(o->p, 16) || misaligned(o->g, 16) || misaligned(o->m, 16) || misaligned(o->v, 16) || misaligned(o->ema, 16) || misaligned(o->state, 256))
        return fail("ss_op_optim_ext: arenas must be 16-byte aligned and state 256-byte aligned");
    if (o->mode == 0 && (!o->g || !o->m || !o->v)) return fail("ss_op_optim_ext: null pointer (an optimiser step needs g, m and v)");
    if (o->mode != 0 && !o->ema) return fail("ss_op_optim_ext: null pointer (ema_range and arena_swap need ema)");
    if (!(o->weight_decay >= 0.0f) || !(o->ema_decay >= 0.0 && o->ema_decay < 1.0) || o->n_runs < 0 || o->n_runs > WD_RUN_MAX || (o->n_runs && (!o->run_start || !o->run_len || !o->run_decayed)))
        return fail("ss_op_optim_ext: weight_decay must be >= 0, ema_decay in [0, 1), n_runs in 0 .. 96 with its three arrays");
    hipStream_t s = S(stream);
    if (o->mode == 2) {
        HIPCHK(arena_swap(o->p + o->lo, o->ema + o->lo, o->hi - o->lo, s));
        return 0;
    }
    if (o->mode == 1 && o->step < 0) {      // the state as an earlier call left it: nothing is copied, nothing waited for, no prepare runs
        HIPCHK(ema_range(o->ema + o->lo, o->p + o->lo, o->hi - o->lo, (const AdamState*)o->state,
                         (const OptExtState*)((char*)o->state + OPT_EXT_STATE_BYTE), s));
        return 0;
    }
    // the head of a workspace as ss_bind and the setters leave it: Adam state at byte 0, clip coefficient at 128, the extension at 144
    alignas(16) char head[256] = {};
    AdamState* st = (AdamState*)head;
    ClipState* clip = (ClipState*)(head + CLIP_STATE_BYTE);
    OptExtState* ext = (OptExtState*)(head + OPT_EXT_STATE_BYTE);
    st->lr = o->lr;
    st->beta1 = o->beta1;
    st->beta2 = o->beta2;
    st->eps = o->eps;
    st->step = o->step;
    clip->coef = o->clip_coef;
    ext->ema_decay = o->ema_decay;
    ext->n = o->ema_updates;
    ext->wd = o->weight_decay;
    ext->flags = (o->ema ? OPT_EXT_EMA : 0u) | (o->ema_warmup ? OPT_EXT_WARMUP : 0u);
    HIPCHK(hipMemcpyAsync(o->state, head, 256, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    AdamState* dst = (AdamState*)o->state;
    AdamExt x;
    x.ext = (OptExtState*)((char*)o->state + OPT_EXT_STATE_BYTE);
    x.wd = o->weight_decay > 0.0f;
    x.ema = o->ema;
    WdRunTable tb{};
    if (x.wd && o->n_runs) {
        tb.n = o->n_runs;
        for (int k = 0; k < o->n_runs; ++k) {
            tb.start[k] = o->run_start[k];
            tb.len[k] = o->run_len[k];
            tb.decayed[k] = o->run_decayed[k];
        }
        x.runs = &tb;
    }
    if (!x.on()) return fail("ss_op_optim_ext: neither weight decay nor an EMA arena: that is the plain Adam step");
    HIPCHK(adam_prepare_ext(dst, x, nullptr, o->skip_status, s));
    if (o->mode == 1) {
        HIPCHK(ema_range(o->ema + o->lo, o->p + o->lo, o->hi - o->lo, dst, x.ext, s));
        return 0;
    }
    const float* coef = o->clip_coef > 0.0f ? &((ClipState*)((char*)o->state + CLIP_STATE_BYTE))->coef : nullptr;
    HIPCHK(adam_range_ext(o->p, o->g, o->m, o->v, o->lo, o->hi, dst, o->grad_scale, coef, x, s));
    return 0;
}

int ss_op_lr_schedule(int kind, double base, int warmup_steps, double warmup_start, int total_steps, double gamma, int period, double min_lr,
                      const long* steps_dev, long n, double* lr_dev, void* stream) {
    if (const char* why = lr_schedule_refusal(kind, warmup_steps, warmup_start, total_steps, gamma, period, min_lr))
        return fail(std::string("ss_op_lr_schedule: ") + why);
    if (!steps_dev || !lr_dev) return fail("ss_op_lr_schedule: null pointer");
    if (n < 1 || n > (1L << 24)) return fail("ss_op_lr_schedule: n must lie in 1 .. 2^24");
    if (misaligned(steps_dev, 8) || misaligned(lr_dev, 8)) return fail("ss_op_lr_schedule: steps_dev and lr_dev must be 8-byte aligned");
    LrSchedState q{};         // as ss_set_lr_schedule leaves it on the device
    q.kind = kind;
    q.W = warmup_steps;
    q.sf = warmup_start;
    q.N = total_steps > 0 ? total_steps : 1;
    q.gamma = gamma;
    q.P = period > 0 ? period : 1;
    q.min_lr = min_lr;
    HIPCHK(lr_schedule_eval(q, base, steps_dev, n, lr_dev, S(stream)));
    return 0;
}

}  // extern "C"
