// C entry points of the audio / data front end (include/speechsplit_amd.h): collation, mel spectrograms, F0 normalisation, the pitch
// tracker, batched feature extraction, the resampler, silence removal, numpy's MT19937 stream, the Griffin-Lim vocoder, the conversion scores and the waveform scores.  None of them takes an engine: each checks its arguments, refuses by
// the argument's name through ss_last_error() and hands the rest to the launchers of kernels.h.
#include <cmath>
#include <cstdint>
#include <string>

#include "abi.h"
#include "kernels.h"
#include "../../include/speechsplit_amd.h"

using namespace ss;

extern "C" {

int ss_collate(const float* mel_cat, const float* f0_cat, const float* emb_tab, const long* row0, const int* len, const int* item,
               int B, int T, int n_mel, int emb_dim, float* mel, float* f0, float* emb, void* stream) {
    if (!mel_cat || !f0_cat || !emb_tab || !row0 || !len || !item || !mel || !f0 || !emb) return fail("ss_collate: null pointer");
    if (B <= 0 || T <= 0 || n_mel <= 0 || emb_dim <= 0) return fail("ss_collate: bad shape");
    HIPCHK(collate(mel_cat, f0_cat, emb_tab, row0, len, item, B, T, n_mel, emb_dim, mel, f0, emb, S(stream)));
    return 0;
}

int ss_melspec_frames(int n) { return n >= 513 ? (n + 256) / 256 : 0; }

int ss_melspec(const double* wav, int n, const double* mel_basis, int n_mels, float* out, void* stream) {
    if (!wav || !mel_basis || !out) return fail("ss_melspec: null pointer");
    if (n < 513) return fail("ss_melspec: at least 513 samples (reflect padding by 512)");
    HIPCHK(melspec(wav, n, mel_basis, n_mels, out, ss_melspec_frames(n), S(stream)));
    return 0;
}

int ss_f0_normalize(const double* f0, int n, float* out, void* stream) {
    if (!f0 || !out || n < 1) return fail("ss_f0_normalize: bad arguments");
    HIPCHK(f0_normalize(f0, n, out, S(stream)));
    return 0;
}

// ---- pitch tracker (pitch.hip).  Everything is refused here, by the argument's name, before anything is enqueued.
namespace {
int pitch_shape(const char* who, int B, int max_n, double lo_hz, double hi_hz, PitchLags* g) {
    if (B < 1 || B > PITCH_MAX_ROWS) return fail(std::string(who) + ": B outside 1 .. 65535");
    if (max_n < 513 || max_n > 256 * (SS_MAX_EVAL_FRAMES - 1))
        return fail(std::string(who) + ": max_n outside 513 .. 256 * (SS_MAX_EVAL_FRAMES - 1)");
    if (!(lo_hz > 0.0)) return fail(std::string(who) + ": lo_hz is NaN or not positive");
    if (!(hi_hz > 0.0)) return fail(std::string(who) + ": hi_hz is NaN or not positive");
    if (!(lo_hz < hi_hz)) return fail(std::string(who) + ": lo_hz is not below hi_hz");
    if (!(floor(16000.0 / hi_hz) >= PITCH_MIN_LAG)) return fail(std::string(who) + ": hi_hz above 1000 (the shortest lag would be below 16 samples)");
    if (!(ceil(16000.0 / lo_hz) <= PITCH_MAX_LAG)) return fail(std::string(who) + ": lo_hz below 40 (the longest lag would be above 400 samples)");
    if (!pitch_lags(lo_hz, hi_hz, g)) return fail(std::string(who) + ": lo_hz .. hi_hz covers fewer than 3 lags");
    return 0;
}
int pitch_scratch_ok(const char* who, int B, int max_n, const PitchLags& g, const void* scratch, long scratch_bytes) {
    if (!scratch) return fail(std::string(who) + ": null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail(std::string(who) + ": scratch_dev is not 256-byte aligned");
    if (scratch_bytes < pitch_scratch_bytes(B, ss_melspec_frames(max_n), g.lmax - g.lmin + 1))
        return fail(std::string(who) + ": scratch_bytes below ss_pitch_scratch_bytes(B, max_n, lo_hz, hi_hz)");
    return 0;
}
}  // namespace

long ss_pitch_scratch_bytes(int B, int max_n, double lo_hz, double hi_hz) {
    PitchLags g;
    CHK(pitch_shape("ss_pitch_scratch_bytes", B, max_n, lo_hz, hi_hz, &g));
    return pitch_scratch_bytes(B, ss_melspec_frames(max_n), g.lmax - g.lmin + 1);
}

int ss_pitch_track(const double* wav, const int* n, int B, int max_n, double scale, double lo_hz, double hi_hz, double* f0, void* scratch,
                   long scratch_bytes, void* stream) {
    PitchLags g;
    if (!wav) return fail("ss_pitch_track: null pointer: wav_dev");
    if (!f0) return fail("ss_pitch_track: null pointer: f0_dev");
    CHK(pitch_shape("ss_pitch_track", B, max_n, lo_hz, hi_hz, &g));
    if (!(scale > 0.0) || std::isinf(scale)) return fail("ss_pitch_track: scale is not finite or not positive");
    CHK(pitch_scratch_ok("ss_pitch_track", B, max_n, g, scratch, scratch_bytes));
    const PitchScratch sc = pitch_scratch(scratch, B, ss_melspec_frames(max_n), g.lmax - g.lmin + 1);
    HIPCHK(pitch_nccf(wav, n, B, max_n, scale, g, sc.phi, sc.rms, S(stream)));
    HIPCHK(pitch_dp(sc.phi, sc.rms, nullptr, n, B, max_n, g, f0, sc, S(stream)));
    return 0;
}

int ss_op_nccf(const double* wav, const int* n, int B, int max_n, double scale, double lo_hz, double hi_hz, double* phi, double* rms,
               void* stream) {
    PitchLags g;
    if (!wav) return fail("ss_op_nccf: null pointer: wav_dev");
    if (!phi) return fail("ss_op_nccf: null pointer: phi_dev");
    if (!rms) return fail("ss_op_nccf: null pointer: rms_dev");
    CHK(pitch_shape("ss_op_nccf", B, max_n, lo_hz, hi_hz, &g));
    if (!(scale > 0.0) || std::isinf(scale)) return fail("ss_op_nccf: scale is not finite or not positive");
    HIPCHK(pitch_nccf(wav, n, B, max_n, scale, g, phi, rms, S(stream)));
    return 0;
}

int ss_op_pitch_dp(const double* phi, const double* rms, const int* n, int B, int max_n, double lo_hz, double hi_hz, double* f0,
                   void* scratch, long scratch_bytes, void* stream) {
    PitchLags g;
    if (!phi) return fail("ss_op_pitch_dp: null pointer: phi_dev");
    if (!rms) return fail("ss_op_pitch_dp: null pointer: rms_dev");
    if (!f0) return fail("ss_op_pitch_dp: null pointer: f0_dev");
    CHK(pitch_shape("ss_op_pitch_dp", B, max_n, lo_hz, hi_hz, &g));
    CHK(pitch_scratch_ok("ss_op_pitch_dp", B, max_n, g, scratch, scratch_bytes));
    HIPCHK(pitch_dp(phi, rms, nullptr, n, B, max_n, g, f0, pitch_scratch(scratch, B, ss_melspec_frames(max_n), g.lmax - g.lmin + 1), S(stream)));
    return 0;
}

// ---- the same with RAPT's spectral-stationarity term (stat_kernel, dp_kernel<true>)
long ss_pitch_stat_scratch_bytes(int B, int max_n, double lo_hz, double hi_hz) {
    PitchLags g;
    CHK(pitch_shape("ss_pitch_stat_scratch_bytes", B, max_n, lo_hz, hi_hz, &g));
    return pitch_stat_scratch_bytes(B, ss_melspec_frames(max_n), g.lmax - g.lmin + 1);
}

int ss_pitch_track_stat(const double* wav, const int* n, int B, int max_n, double scale, double lo_hz, double hi_hz, double* f0,
                        void* scratch, long scratch_bytes, void* stream) {
    PitchLags g;
    if (!wav) return fail("ss_pitch_track_stat: null pointer: wav_dev");
    if (!f0) return fail("ss_pitch_track_stat: null pointer: f0_dev");
    CHK(pitch_shape("ss_pitch_track_stat", B, max_n, lo_hz, hi_hz, &g));
    if (!(scale > 0.0) || std::isinf(scale)) return fail("ss_pitch_track_stat: scale is not finite or not positive");
    const int F = ss_melspec_frames(max_n), K = g.lmax - g.lmin + 1;
    if (!scratch) return fail("ss_pitch_track_stat: null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail("ss_pitch_track_stat: scratch_dev is not 256-byte aligned");
    if (scratch_bytes < pitch_stat_scratch_bytes(B, F, K))
        return fail("ss_pitch_track_stat: scratch_bytes below ss_pitch_stat_scratch_bytes(B, max_n, lo_hz, hi_hz)");
    const PitchScratch sc = pitch_scratch(scratch, B, F, K);
    double* stat = pitch_stat_track(scratch, B, F, K);
    HIPCHK(pitch_nccf(wav, n, B, max_n, scale, g, sc.phi, sc.rms, S(stream)));
    HIPCHK(pitch_stationarity(wav, n, B, max_n, scale, stat, S(stream)));
    HIPCHK(pitch_dp(sc.phi, sc.rms, stat, n, B, max_n, g, f0, sc, S(stream)));
    return 0;
}

int ss_op_pitch_stationarity(const double* wav, const int* n, int B, int max_n, double scale, double* stat, void* stream) {
    if (!wav) return fail("ss_op_pitch_stationarity: null pointer: wav_dev");
    if (!stat) return fail("ss_op_pitch_stationarity: null pointer: stat_dev");
    if (B < 1 || B > PITCH_MAX_ROWS) return fail("ss_op_pitch_stationarity: B outside 1 .. 65535");
    if (max_n < 513 || max_n > 256 * (SS_MAX_EVAL_FRAMES - 1))
        return fail("ss_op_pitch_stationarity: max_n outside 513 .. 256 * (SS_MAX_EVAL_FRAMES - 1)");
    if (!(scale > 0.0) || std::isinf(scale)) return fail("ss_op_pitch_stationarity: scale is not finite or not positive");
    HIPCHK(pitch_stationarity(wav, n, B, max_n, scale, stat, S(stream)));
    return 0;
}

int ss_op_pitch_dp_stat(const double* phi, const double* rms, const double* stat, const int* n, int B, int max_n, double lo_hz, double hi_hz,
                        double* f0, void* scratch, long scratch_bytes, void* stream) {
    PitchLags g;
    if (!phi) return fail("ss_op_pitch_dp_stat: null pointer: phi_dev");
    if (!rms) return fail("ss_op_pitch_dp_stat: null pointer: rms_dev");
    if (!stat) return fail("ss_op_pitch_dp_stat: null pointer: stat_dev");
    if (!f0) return fail("ss_op_pitch_dp_stat: null pointer: f0_dev");
    CHK(pitch_shape("ss_op_pitch_dp_stat", B, max_n, lo_hz, hi_hz, &g));
    CHK(pitch_scratch_ok("ss_op_pitch_dp_stat", B, max_n, g, scratch, scratch_bytes));
    HIPCHK(pitch_dp(phi, rms, stat, n, B, max_n, g, f0, pitch_scratch(scratch, B, ss_melspec_frames(max_n), g.lmax - g.lmin + 1), S(stream)));
    return 0;
}

// ---- batched feature extraction (filtfilt.hip, features.hip).  Everything is refused here, by the argument's name, before anything is enqueued.
namespace {
int feat_shape(const char* who, int B, int max_n) {
    if (B < 1 || B > FEAT_MAX_ROWS) return fail(std::string(who) + ": B outside 1 .. 65535");
    if (max_n < 513 || max_n > 256 * (SS_MAX_EVAL_FRAMES - 1))
        return fail(std::string(who) + ": max_n outside 513 .. 256 * (SS_MAX_EVAL_FRAMES - 1)");
    return 0;
}
}  // namespace

long ss_filtfilt_scratch_bytes(int B, int max_n) {
    CHK(feat_shape("ss_filtfilt_scratch_bytes", B, max_n));
    return filtfilt_scratch_bytes(B, max_n);
}

int ss_filtfilt(const double* x, const int* n, int B, int max_n, const double* b, const double* a, const double* zi, double gain,
                const double* dither, double dither_scale, double* y, void* scratch, long scratch_bytes, void* stream) {
    if (!x) return fail("ss_filtfilt: null pointer: x_dev");
    if (!b) return fail("ss_filtfilt: null pointer: b");
    if (!a) return fail("ss_filtfilt: null pointer: a");
    if (!zi) return fail("ss_filtfilt: null pointer: zi");
    if (!y) return fail("ss_filtfilt: null pointer: y_dev");
    CHK(feat_shape("ss_filtfilt", B, max_n));
    FiltCoef c;
    for (int i = 0; i < FILT_NCOEF; ++i) {
        if (!std::isfinite(b[i])) return fail("ss_filtfilt: b[" + std::to_string(i) + "] is not finite");
        if (!std::isfinite(a[i])) return fail("ss_filtfilt: a[" + std::to_string(i) + "] is not finite");
        if (i < FILT_NCOEF - 1 && !std::isfinite(zi[i])) return fail("ss_filtfilt: zi[" + std::to_string(i) + "] is not finite");
        c.b[i] = b[i];
        c.a[i] = a[i];
        if (i < FILT_NCOEF - 1) c.zi[i] = zi[i];
    }
    if (a[0] != 1.0) return fail("ss_filtfilt: a[0] is not exactly 1 (normalise b and a on the host, as scipy does)");
    if (!std::isfinite(gain)) return fail("ss_filtfilt: gain is not finite");
    if (!std::isfinite(dither_scale)) return fail("ss_filtfilt: dither_scale is not finite");
    if (!scratch) return fail("ss_filtfilt: null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail("ss_filtfilt: scratch_dev is not 256-byte aligned");
    if (scratch_bytes < filtfilt_scratch_bytes(B, max_n)) return fail("ss_filtfilt: scratch_bytes below ss_filtfilt_scratch_bytes(B, max_n)");
    HIPCHK(filtfilt(x, n, B, max_n, c, gain, dither, dither_scale, y, (double*)scratch, S(stream)));
    return 0;
}

int ss_melspec_batch(const double* wav, const int* n, int B, int max_n, const double* mel_basis, int n_mels, float* out, void* stream) {
    if (!wav) return fail("ss_melspec_batch: null pointer: wav_dev");
    if (!mel_basis) return fail("ss_melspec_batch: null pointer: mel_basis_dev");
    if (!out) return fail("ss_melspec_batch: null pointer: out_dev");
    CHK(feat_shape("ss_melspec_batch", B, max_n));
    if (n_mels < 1) return fail("ss_melspec_batch: n_mels below 1");
    HIPCHK(melspec_batch(wav, n, B, max_n, mel_basis, n_mels, out, S(stream)));
    return 0;
}

int ss_f0_normalize_batch(const double* f0, const int* n, int B, int max_n, double unvoiced, float* out, void* stream) {
    if (!f0) return fail("ss_f0_normalize_batch: null pointer: f0_dev");
    if (!out) return fail("ss_f0_normalize_batch: null pointer: out_dev");
    CHK(feat_shape("ss_f0_normalize_batch", B, max_n));
    if (std::isnan(unvoiced)) return fail("ss_f0_normalize_batch: unvoiced is NaN");
    HIPCHK(f0_normalize_batch(f0, n, B, max_n, unvoiced, out, S(stream)));
    return 0;
}

// ---- rational-rate resampler (resample.hip).  Everything is refused here, by the argument's name, before anything is enqueued.
namespace {
int resample_rates(const char* who, int up, int down) {
    if (up < 1 || up > RESAMPLE_MAX_RATE) return fail(std::string(who) + ": up outside 1 .. 1024");
    if (down < 1 || down > RESAMPLE_MAX_RATE) return fail(std::string(who) + ": down outside 1 .. 1024");
    return 0;
}
int resample_taps(const char* who, int n_taps) {
    if (n_taps < 1) return fail(std::string(who) + ": n_taps below 1");
    if (n_taps % 2 == 0) return fail(std::string(who) + ": n_taps is even (the filter needs a centre tap)");
    return 0;
}
}  // namespace

long ss_resample_len(long n, int up, int down) {
    if (n < 0 || n > (1L << 40)) return fail("ss_resample_len: n outside 0 .. 2^40");
    CHK(resample_rates("ss_resample_len", up, down));
    return resample_len(n, up, down);
}

long ss_resample_scratch_bytes(int up, int n_taps) {
    if (up < 1 || up > RESAMPLE_MAX_RATE) return fail("ss_resample_scratch_bytes: up outside 1 .. 1024");
    CHK(resample_taps("ss_resample_scratch_bytes", n_taps));
    return resample_scratch_bytes(up, n_taps);
}

int ss_resample(const double* x, const int* n, int B, int max_n, int up, int down, const double* h, int n_taps, double* y, void* scratch,
                long scratch_bytes, void* stream) {
    if (!x) return fail("ss_resample: null pointer: x_dev");
    if (!h) return fail("ss_resample: null pointer: h_dev");
    if (!y) return fail("ss_resample: null pointer: y_dev");
    if (B < 1 || B > FEAT_MAX_ROWS) return fail("ss_resample: B outside 1 .. 65535");
    if (max_n < 1) return fail("ss_resample: max_n below 1");
    CHK(resample_rates("ss_resample", up, down));
    CHK(resample_taps("ss_resample", n_taps));
    if (resample_len(max_n, up, down) > 2147483647L)
        return fail("ss_resample: max_n: M = ceil(max_n up / down) does not fit an int (the 16 kHz chain behind it takes an int max_n)");
    const long need = resample_scratch_bytes(up, n_taps);
    if (scratch_bytes < need) return fail("ss_resample: scratch_bytes below ss_resample_scratch_bytes(up, n_taps)");
    if (need > 0 && !scratch) return fail("ss_resample: null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail("ss_resample: scratch_dev is not 256-byte aligned");
    HIPCHK(resample(x, n, B, max_n, up, down, h, n_taps, y, S(stream)));
    return 0;
}

// ---- silence removal (silence.hip).  Everything is refused here, by the argument's name, before anything is enqueued.
namespace {
int silence_rows(const char* who, int B, int max_n) {
    if (B < 1 || B > FEAT_MAX_ROWS) return fail(std::string(who) + ": B outside 1 .. 65535");
    if (max_n < 1 || max_n > 256 * (SS_MAX_EVAL_FRAMES - 1)) return fail(std::string(who) + ": max_n outside 1 .. 256 * (SS_MAX_EVAL_FRAMES - 1)");
    return 0;
}
int silence_options(const char* who, double ratio, int hang, int edge, int pause) {
    if (!(ratio > 0.0 && ratio < 1.0)) return fail(std::string(who) + ": ratio outside (0, 1) or NaN");
    if (hang < 0) return fail(std::string(who) + ": hang is negative");
    if (edge < 0) return fail(std::string(who) + ": edge is negative");
    if (pause < -1) return fail(std::string(who) + ": pause below -1");
    return 0;
}
int silence_fade(const char* who, const double* g) {
    if (!g) return fail(std::string(who) + ": null pointer: g");
    for (int r = 0; r < 128; ++r)
        if (!std::isfinite(g[r])) return fail(std::string(who) + ": g[" + std::to_string(r) + "] is not finite");
    return 0;
}
}  // namespace

static_assert(SIL_MAX_BLOCKS == SS_MAX_EVAL_FRAMES - 1, "the refusals above and the header spell this bound out");

long ss_silence_scratch_bytes(int B, int max_n) {
    CHK(silence_rows("ss_silence_scratch_bytes", B, max_n));
    return silence_scratch_bytes(B, max_n);
}

int ss_remove_silence(const double* x, const int* n, int B, int max_n, double ratio, int hang, int edge, int pause, const double* g, double* y,
                      int* m, int* inv, int* k, void* scratch, long scratch_bytes, void* stream) {
    if (!x) return fail("ss_remove_silence: null pointer: x_dev");
    if (!y) return fail("ss_remove_silence: null pointer: y_dev");
    if (!m) return fail("ss_remove_silence: null pointer: m_dev");
    CHK(silence_rows("ss_remove_silence", B, max_n));
    CHK(silence_options("ss_remove_silence", ratio, hang, edge, pause));
    CHK(silence_fade("ss_remove_silence", g));
    if (!scratch) return fail("ss_remove_silence: null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail("ss_remove_silence: scratch_dev is not 256-byte aligned");
    if (scratch_bytes < silence_scratch_bytes(B, max_n)) return fail("ss_remove_silence: scratch_bytes below ss_silence_scratch_bytes(B, max_n)");
    const SilenceScratch sc = silence_scratch(scratch, B, max_n);
    int* inv_w = inv ? inv : sc.inv;
    int* k_w = k ? k : sc.k;
    HIPCHK(silence_levels(x, n, B, max_n, sc.e, S(stream)));
    HIPCHK(silence_mask(sc.e, n, true, B, max_n, ratio, hang, edge, pause, inv_w, k_w, S(stream)));
    HIPCHK(silence_gather(x, n, B, max_n, inv_w, k_w, g, y, m, S(stream)));
    return 0;
}

int ss_op_silence_levels(const double* x, const int* n, int B, int max_n, double* e, void* stream) {
    if (!x) return fail("ss_op_silence_levels: null pointer: x_dev");
    if (!e) return fail("ss_op_silence_levels: null pointer: e_dev");
    CHK(silence_rows("ss_op_silence_levels", B, max_n));
    HIPCHK(silence_levels(x, n, B, max_n, e, S(stream)));
    return 0;
}

int ss_op_silence_mask(const double* e, const int* j, int B, int max_j, double ratio, int hang, int edge, int pause, int* inv, int* k,
                       void* stream) {
    if (!e) return fail("ss_op_silence_mask: null pointer: e_dev");
    if (!inv) return fail("ss_op_silence_mask: null pointer: inv_dev");
    if (!k) return fail("ss_op_silence_mask: null pointer: k_dev");
    if (B < 1 || B > FEAT_MAX_ROWS) return fail("ss_op_silence_mask: B outside 1 .. 65535");
    if (max_j < 1 || max_j > SIL_MAX_BLOCKS) return fail("ss_op_silence_mask: max_j outside 1 .. SS_MAX_EVAL_FRAMES - 1");
    CHK(silence_options("ss_op_silence_mask", ratio, hang, edge, pause));
    HIPCHK(silence_mask(e, j, false, B, 256 * max_j, ratio, hang, edge, pause, inv, k, S(stream)));
    return 0;
}

int ss_op_silence_gather(const double* x, const int* n, int B, int max_n, const int* inv, const int* k, const double* g, double* y, int* m,
                         void* stream) {
    if (!x) return fail("ss_op_silence_gather: null pointer: x_dev");
    if (!inv) return fail("ss_op_silence_gather: null pointer: inv_dev");
    if (!k) return fail("ss_op_silence_gather: null pointer: k_dev");
    if (!y) return fail("ss_op_silence_gather: null pointer: y_dev");
    if (!m) return fail("ss_op_silence_gather: null pointer: m_dev");
    CHK(silence_rows("ss_op_silence_gather", B, max_n));
    CHK(silence_fade("ss_op_silence_gather", g));
    HIPCHK(silence_gather(x, n, B, max_n, inv, k, g, y, m, S(stream)));
    return 0;
}

// ---- numpy's MT19937 stream and the dither gather (mtrand.hip). Everything is refused here, by the argument's name, before anything is enqueued.
int ss_mt19937_rand(unsigned* state, long count, double* out, void* stream) {
    if (!state) return fail("ss_mt19937_rand: null pointer: state_dev");
    if (count < 0 || count > MT_MAX_COUNT) return fail("ss_mt19937_rand: count outside 0 .. 2^40");
    if (count > 0 && !out) return fail("ss_mt19937_rand: null pointer: out_dev (it may be NULL only when count is 0)");
    HIPCHK(mt19937_rand(state, count, out, S(stream)));
    return 0;
}

int ss_dither_rows(const double* draws, long count, const long* first, const int* n, int B, int max_n, double* out, void* stream) {
    if (!draws) return fail("ss_dither_rows: null pointer: draws_dev");
    if (!first) return fail("ss_dither_rows: null pointer: first_dev");
    if (!n) return fail("ss_dither_rows: null pointer: n_dev");
    if (!out) return fail("ss_dither_rows: null pointer: out_dev");
    if (count < 0 || count > MT_MAX_COUNT) return fail("ss_dither_rows: count outside 0 .. 2^40");
    if (B < 1 || B > FEAT_MAX_ROWS) return fail("ss_dither_rows: B outside 1 .. 65535");
    if (max_n < 1) return fail("ss_dither_rows: max_n below 1");
    HIPCHK(dither_rows(draws, count, first, n, B, max_n, out, S(stream)));
    return 0;
}

// ---- Griffin-Lim vocoder (vocoder.hip).  Everything is refused here, by the argument's name, before anything is enqueued.
namespace {
int voc_shape(const char* who, int B, int max_frames) {
    if (B < 1 || B > VOC_MAX_ROWS) return fail(std::string(who) + ": B outside 1 .. 65535");
    if (max_frames < 4 || max_frames > SS_MAX_EVAL_FRAMES)
        return fail(std::string(who) + ": max_frames outside 4 .. SS_MAX_EVAL_FRAMES (reflect padding needs 4 frames)");
    return 0;
}
int voc_scratch(const char* who, int B, int max_frames, const void* scratch, long scratch_bytes) {
    if (!scratch) return fail(std::string(who) + ": null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail(std::string(who) + ": scratch_dev is not 256-byte aligned");
    if (scratch_bytes < vocoder_scratch_bytes(B, max_frames))
        return fail(std::string(who) + ": scratch_bytes below ss_griffinlim_scratch_bytes(B, max_frames)");
    return 0;
}
}  // namespace

int ss_griffinlim_samples(int frames) { return frames >= 4 ? 256 * (frames - 1) : 0; }

long ss_griffinlim_scratch_bytes(int B, int max_frames) {
    CHK(voc_shape("ss_griffinlim_scratch_bytes", B, max_frames));
    return vocoder_scratch_bytes(B, max_frames);
}

int ss_mel_to_linear(const float* mel, const double* inv_basis, const int* frames, int B, int max_frames, int n_mels, double floor,
                     double* mag, void* stream) {
    if (!mel) return fail("ss_mel_to_linear: null pointer: mel_dev");
    if (!inv_basis) return fail("ss_mel_to_linear: null pointer: inv_basis_dev");
    if (!mag) return fail("ss_mel_to_linear: null pointer: mag_dev");
    CHK(voc_shape("ss_mel_to_linear", B, max_frames));
    if (n_mels < 1 || n_mels > VOC_MAX_MELS) return fail("ss_mel_to_linear: n_mels outside 1 .. 4096");
    if (!(floor >= 0.0)) return fail("ss_mel_to_linear: floor is negative or NaN");
    HIPCHK(mel_to_linear(mel, inv_basis, frames, B, max_frames, n_mels, floor, mag, S(stream)));
    return 0;
}

static_assert(NNLS_MAX_PACKED == 3072 && VOC_MAX_MELS == 4096, "the refusals below and the header spell these numbers out");

long ss_mel_nnls_pack(const double* basis, int n_mels, double* packed, long cap_doubles) {
    if (!basis) return fail("ss_mel_nnls_pack: null pointer: basis_host");
    if (n_mels < 1 || n_mels > VOC_MAX_MELS) return fail("ss_mel_nnls_pack: n_mels outside 1 .. 4096");
    const int nbin = 513;
    long nnz = 0;
    for (int m = 0; m < n_mels; ++m) {
        int first = -1, last = -1, count = 0;
        for (int k = 0; k < nbin; ++k) {
            const double v = basis[(long)k * n_mels + m];
            if (!(v >= 0.0) || std::isinf(v))
                return fail("ss_mel_nnls_pack: basis_host: band " + std::to_string(m) + ", bin " + std::to_string(k) +
                            ": the weight is negative or not finite");
            if (v > 0.0) {
                if (first < 0) first = k;
                last = k;
                ++count;
            }
        }
        if (count && last - first + 1 != count)
            return fail("ss_mel_nnls_pack: basis_host: the non-zero weights of band " + std::to_string(m) + " are not one contiguous run of bins");
        nnz += count;
    }
    const long size = 2L * n_mels + nnz;
    if (size > NNLS_MAX_PACKED)
        return fail("ss_mel_nnls_pack: the packed basis takes " + std::to_string(size) + " doubles, beyond the 3072 the kernel's LDS holds");
    if (packed && cap_doubles >= size) {
        double* w = packed + 2L * n_mels;
        for (int m = 0; m < n_mels; ++m) {
            int first = 0, len = 0;
            for (int k = 0; k < nbin; ++k)
                if (basis[(long)k * n_mels + m] > 0.0) {
                    if (!len) first = k;
                    *w++ = basis[(long)k * n_mels + m];
                    ++len;
                }
            packed[2 * m] = (double)first;
            packed[2 * m + 1] = (double)len;
        }
    }
    return size;
}

int ss_mel_to_linear_nnls(const float* mel, const double* inv_basis, const double* packed, long packed_doubles, const int* frames, int B,
                          int max_frames, int n_mels, int n_iter, double step, double floor, double* mag, void* stream) {
    if (!mel) return fail("ss_mel_to_linear_nnls: null pointer: mel_dev");
    if (!inv_basis) return fail("ss_mel_to_linear_nnls: null pointer: inv_basis_dev");
    if (!packed) return fail("ss_mel_to_linear_nnls: null pointer: packed_dev");
    if (!mag) return fail("ss_mel_to_linear_nnls: null pointer: mag_dev");
    CHK(voc_shape("ss_mel_to_linear_nnls", B, max_frames));
    if (n_mels < 1 || n_mels > VOC_MAX_MELS) return fail("ss_mel_to_linear_nnls: n_mels outside 1 .. 4096");
    if (packed_doubles < 2L * n_mels || packed_doubles > 515L * n_mels)
        return fail("ss_mel_to_linear_nnls: packed_doubles disagrees with n_mels (2 n_mels + the number of weights, at most 513 a band)");
    if (packed_doubles > NNLS_MAX_PACKED) return fail("ss_mel_to_linear_nnls: packed_doubles beyond the 3072 the kernel's LDS holds");
    if (n_iter < 0 || n_iter > 100000) return fail("ss_mel_to_linear_nnls: n_iter outside 0 .. 100000");
    if (!(step > 0.0) || std::isinf(step)) return fail("ss_mel_to_linear_nnls: step is not finite and positive");
    if (!(floor >= 0.0)) return fail("ss_mel_to_linear_nnls: floor is negative or NaN");
    HIPCHK(mel_to_linear_nnls(mel, inv_basis, packed, packed_doubles, frames, B, max_frames, n_mels, n_iter, step, floor, mag, S(stream)));
    return 0;
}

static_assert(HARM_MAX == 190, "the header spells this number out");

int ss_mel_to_linear_harmonic(const float* mel, const double* f0_hz, const double* inv_basis, const double* packed, long packed_doubles,
                              const int* frames, int B, int max_frames, int n_mels, double f_top, int n_iter, double floor, double* mag,
                              double* share, void* stream) {
    if (!mel) return fail("ss_mel_to_linear_harmonic: null pointer: mel_dev");
    if (!f0_hz) return fail("ss_mel_to_linear_harmonic: null pointer: f0_hz_dev");
    if (!inv_basis) return fail("ss_mel_to_linear_harmonic: null pointer: inv_basis_dev");
    if (!packed) return fail("ss_mel_to_linear_harmonic: null pointer: packed_dev");
    if (!mag) return fail("ss_mel_to_linear_harmonic: null pointer: mag_dev");
    if (!share) return fail("ss_mel_to_linear_harmonic: null pointer: share_dev");
    CHK(voc_shape("ss_mel_to_linear_harmonic", B, max_frames));
    if (n_mels < 1 || n_mels > VOC_MAX_MELS) return fail("ss_mel_to_linear_harmonic: n_mels outside 1 .. 4096");
    if (packed_doubles < 2L * n_mels || packed_doubles > 515L * n_mels)
        return fail("ss_mel_to_linear_harmonic: packed_doubles disagrees with n_mels (2 n_mels + the number of weights, at most 513 a band)");
    if (packed_doubles > NNLS_MAX_PACKED) return fail("ss_mel_to_linear_harmonic: packed_doubles beyond the 3072 the kernel's LDS holds");
    if (!(f_top >= 1000.0 && f_top <= 8000.0)) return fail("ss_mel_to_linear_harmonic: f_top outside 1000 .. 8000 or NaN");
    if (n_iter < 0 || n_iter > 100000) return fail("ss_mel_to_linear_harmonic: n_iter outside 0 .. 100000");
    if (!(floor >= 0.0)) return fail("ss_mel_to_linear_harmonic: floor is negative or NaN");
    HIPCHK(mel_to_linear_harmonic(mel, f0_hz, inv_basis, packed, packed_doubles, frames, B, max_frames, n_mels, f_top, n_iter, floor, mag,
                                  share, S(stream)));
    return 0;
}

long ss_harmonic_phase_scratch_bytes(int B, int max_frames) {
    CHK(voc_shape("ss_harmonic_phase_scratch_bytes", B, max_frames));
    return harmonic_phase_scratch_bytes(B, max_frames);
}

int ss_harmonic_phase(const double* f0_hz, const double* share, const double* rand_phase, const int* frames, int B, int max_frames,
                      double f_top, double* phase0, void* scratch, long scratch_bytes, void* stream) {
    if (!f0_hz) return fail("ss_harmonic_phase: null pointer: f0_hz_dev");
    if (!share) return fail("ss_harmonic_phase: null pointer: share_dev");
    if (!phase0) return fail("ss_harmonic_phase: null pointer: phase0_dev");
    CHK(voc_shape("ss_harmonic_phase", B, max_frames));
    if (!(f_top >= 1000.0 && f_top <= 8000.0)) return fail("ss_harmonic_phase: f_top outside 1000 .. 8000 or NaN");
    if (!scratch) return fail("ss_harmonic_phase: null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail("ss_harmonic_phase: scratch_dev is not 256-byte aligned");
    if (scratch_bytes < harmonic_phase_scratch_bytes(B, max_frames))
        return fail("ss_harmonic_phase: scratch_bytes below ss_harmonic_phase_scratch_bytes(B, max_frames)");
    HIPCHK(harmonic_phase(f0_hz, share, rand_phase, frames, B, max_frames, f_top, phase0, (double*)scratch, S(stream)));
    return 0;
}

int ss_op_harmonic_u(const double* f0_hz, const int* frames, int B, int max_frames, double* u, void* stream) {
    if (!f0_hz) return fail("ss_op_harmonic_u: null pointer: f0_hz_dev");
    if (!u) return fail("ss_op_harmonic_u: null pointer: u_dev");
    CHK(voc_shape("ss_op_harmonic_u", B, max_frames));
    HIPCHK(harmonic_u(f0_hz, frames, B, max_frames, u, S(stream)));
    return 0;
}

int ss_griffinlim(const double* mag, const double* phase0, const int* frames, int B, int max_frames, int n_iter, double momentum,
                  double* wav, void* scratch, long scratch_bytes, void* stream) {
    if (!mag) return fail("ss_griffinlim: null pointer: mag_dev");
    if (!wav) return fail("ss_griffinlim: null pointer: wav_dev");
    CHK(voc_shape("ss_griffinlim", B, max_frames));
    if (n_iter < 0 || n_iter > 1024) return fail("ss_griffinlim: n_iter outside 0 .. 1024");
    if (!(momentum >= 0.0 && momentum < 1.0)) return fail("ss_griffinlim: momentum outside [0, 1) or NaN");
    CHK(voc_scratch("ss_griffinlim", B, max_frames, scratch, scratch_bytes));
    HIPCHK(griffinlim(mag, phase0, frames, B, max_frames, n_iter, momentum, wav, vocoder_scratch(scratch, B, max_frames), S(stream)));
    return 0;
}

int ss_op_stft(const double* wav, const int* frames, int B, int max_frames, double* spec, void* stream) {
    if (!wav) return fail("ss_op_stft: null pointer: wav_dev");
    if (!spec) return fail("ss_op_stft: null pointer: spec_dev");
    CHK(voc_shape("ss_op_stft", B, max_frames));
    HIPCHK(stft(wav, frames, B, max_frames, spec, S(stream)));
    return 0;
}

int ss_op_istft(const double* spec, const int* frames, int B, int max_frames, double* wav, void* scratch, long scratch_bytes,
                void* stream) {
    if (!spec) return fail("ss_op_istft: null pointer: spec_dev");
    if (!wav) return fail("ss_op_istft: null pointer: wav_dev");
    CHK(voc_shape("ss_op_istft", B, max_frames));
    CHK(voc_scratch("ss_op_istft", B, max_frames, scratch, scratch_bytes));
    HIPCHK(istft(spec, frames, B, max_frames, wav, vocoder_scratch(scratch, B, max_frames).frame_buf, S(stream)));
    return 0;
}

// ---- conversion scores (dtw.hip).  Everything is refused here, by the argument's name, before anything is enqueued.
namespace {
int dtw_shape(const char* who, int B, int max_tx, int max_ty) {
    if (B < 1 || B > DTW_MAX_ROWS) return fail(std::string(who) + ": B outside 1 .. 65535");
    if (max_tx < 1 || max_tx > SS_MAX_EVAL_FRAMES) return fail(std::string(who) + ": max_tx outside 1 .. SS_MAX_EVAL_FRAMES");
    if (max_ty < 1 || max_ty > SS_MAX_EVAL_FRAMES) return fail(std::string(who) + ": max_ty outside 1 .. SS_MAX_EVAL_FRAMES");
    return 0;
}
}  // namespace

static_assert(DTW_MAX_DIM == 40 && DTW_MAX_ROWS == 65535, "the refusals below and the header spell these numbers out");

int ss_mel_cepstra(const float* mel, const int* len, int B, int max_t, int n_mels, const double* dct, int n_ceps, double* out, void* stream) {
    if (!mel) return fail("ss_mel_cepstra: null pointer: mel_dev");
    if (!dct) return fail("ss_mel_cepstra: null pointer: dct_dev");
    if (!out) return fail("ss_mel_cepstra: null pointer: out_dev");
    if (B < 1 || B > DTW_MAX_ROWS) return fail("ss_mel_cepstra: B outside 1 .. 65535");
    if (max_t < 1 || max_t > SS_MAX_EVAL_FRAMES) return fail("ss_mel_cepstra: max_t outside 1 .. SS_MAX_EVAL_FRAMES");
    if (n_mels < 1 || n_mels > 128) return fail("ss_mel_cepstra: n_mels outside 1 .. 128");
    if (n_ceps < 1 || n_ceps > DTW_MAX_DIM) return fail("ss_mel_cepstra: n_ceps outside 1 .. 40");
    HIPCHK(mel_cepstra(mel, len, B, max_t, n_mels, dct, n_ceps, out, S(stream)));
    return 0;
}

long ss_dtw_scratch_bytes(int B, int max_tx, int max_ty) {
    CHK(dtw_shape("ss_dtw_scratch_bytes", B, max_tx, max_ty));
    return dtw_scratch_bytes(B, max_tx, max_ty);
}

int ss_dtw(const double* fx, const int* tx, const double* fy, const int* ty, int B, int max_tx, int max_ty, int dim, double scale,
           double* out, int* path, int* path_len, void* scratch, long scratch_bytes, void* stream) {
    if (!fx) return fail("ss_dtw: null pointer: fx_dev");
    if (!fy) return fail("ss_dtw: null pointer: fy_dev");
    if (!out) return fail("ss_dtw: null pointer: out_dev");
    CHK(dtw_shape("ss_dtw", B, max_tx, max_ty));
    if (dim < 1 || dim > DTW_MAX_DIM) return fail("ss_dtw: dim outside 1 .. 40");
    if (!(scale > 0.0) || std::isinf(scale)) return fail("ss_dtw: scale is not finite or not positive");
    if (!path != !path_len) return fail("ss_dtw: path_dev and path_len_dev must both be given or both be NULL");
    if (!scratch) return fail("ss_dtw: null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail("ss_dtw: scratch_dev is not 256-byte aligned");
    if (scratch_bytes < dtw_scratch_bytes(B, max_tx, max_ty))
        return fail("ss_dtw: scratch_bytes below ss_dtw_scratch_bytes(B, max_tx, max_ty)");
    HIPCHK(dtw(fx, tx, fy, ty, B, max_tx, max_ty, dim, scale, out, path, path_len, dtw_scratch(scratch, B, max_tx, max_ty), S(stream)));
    return 0;
}

int ss_path_f0_stats(const int* path, const int* path_len, const double* f0x, const double* f0y, int B, int max_tx, int max_ty, double* out,
                     void* stream) {
    if (!path) return fail("ss_path_f0_stats: null pointer: path_dev");
    if (!f0x) return fail("ss_path_f0_stats: null pointer: f0x_dev");
    if (!f0y) return fail("ss_path_f0_stats: null pointer: f0y_dev");
    if (!out) return fail("ss_path_f0_stats: null pointer: out_dev");
    CHK(dtw_shape("ss_path_f0_stats", B, max_tx, max_ty));
    HIPCHK(path_f0_stats(path, path_len, f0x, f0y, B, max_tx, max_ty, out, S(stream)));
    return 0;
}

// ---- waveform scores (stoi.hip).  Everything is refused here, by the argument's name, before anything is enqueued.
namespace {
int stoi_rows(const char* who, int B, int max_n) {
    if (B < 1 || B > STOI_MAX_ROWS) return fail(std::string(who) + ": B outside 1 .. 65535");
    if (max_n < STOI_FRAME) return fail(std::string(who) + ": max_n below 256 (one frame)");
    long bytes = 0;                                       // an int max_n cannot get there today; the check stays with the arithmetic
    if (__builtin_mul_overflow((long)B * 24L * STOI_MAX_BANDS, (long)max_n, &bytes))
        return fail(std::string(who) + ": max_n so large that the scratch does not fit a long");
    return 0;
}
int stoi_band_table(const char* who, const int* lo, const int* hi, int n_bands, StoiTables* tb) {
    if (!lo) return fail(std::string(who) + ": null pointer: band_lo");
    if (!hi) return fail(std::string(who) + ": null pointer: band_hi");
    if (n_bands < 1 || n_bands > STOI_MAX_BANDS) return fail(std::string(who) + ": n_bands outside 1 .. 32");
    for (int j = 0; j < n_bands; ++j) {
        if (lo[j] < 0) return fail(std::string(who) + ": band_lo[" + std::to_string(j) + "] is negative");
        if (hi[j] > 257) return fail(std::string(who) + ": band_hi[" + std::to_string(j) + "] is above 257 (the bins of a 512-point transform)");
        if (lo[j] >= hi[j]) return fail(std::string(who) + ": band_lo[" + std::to_string(j) + "] is not below band_hi[" + std::to_string(j) + "]");
    }
    stoi_tables(lo, hi, n_bands, tb);
    return 0;
}
}  // namespace

static_assert(STOI_MAX_ROWS == 65535 && STOI_MAX_BANDS == 32 && STOI_FRAME == 256, "the refusals below and the header spell these numbers out");

long ss_stoi_scratch_bytes(int B, int max_n) {
    CHK(stoi_rows("ss_stoi_scratch_bytes", B, max_n));
    return stoi_scratch_bytes(B, max_n);
}

int ss_stoi(const double* x, const double* y, const int* n, int B, int max_n, const int* band_lo, const int* band_hi, int n_bands,
            int extended, double* out, void* scratch, long scratch_bytes, void* stream) {
    StoiTables tb;
    if (!x) return fail("ss_stoi: null pointer: x_dev");
    if (!y) return fail("ss_stoi: null pointer: y_dev");
    if (!out) return fail("ss_stoi: null pointer: out_dev");
    CHK(stoi_rows("ss_stoi", B, max_n));
    CHK(stoi_band_table("ss_stoi", band_lo, band_hi, n_bands, &tb));
    if (extended != 0 && extended != 1) return fail("ss_stoi: extended is neither 0 nor 1");
    if (!scratch) return fail("ss_stoi: null pointer: scratch_dev");
    if ((uintptr_t)scratch % 256) return fail("ss_stoi: scratch_dev is not 256-byte aligned");
    if (scratch_bytes < stoi_scratch_bytes(B, max_n)) return fail("ss_stoi: scratch_bytes below ss_stoi_scratch_bytes(B, max_n)");
    HIPCHK(stoi(x, y, n, B, max_n, tb, extended, out, stoi_scratch(scratch, B, max_n), S(stream)));
    return 0;
}

int ss_op_stoi_compact(const double* x, const double* y, const int* n, int B, int max_n, int from_map, double* e, int* inv, int* k,
                       double* xp, double* yp, void* stream) {
    StoiTables tb;
    const int lo = 0, hi = 1;
    if (!x) return fail("ss_op_stoi_compact: null pointer: x_dev");
    if (!y) return fail("ss_op_stoi_compact: null pointer: y_dev");
    if (from_map != 0 && from_map != 1) return fail("ss_op_stoi_compact: from_map is neither 0 nor 1");
    if (!from_map && !e) return fail("ss_op_stoi_compact: null pointer: e_dev (it may be NULL only with from_map)");
    if (!inv) return fail("ss_op_stoi_compact: null pointer: inv_dev");
    if (!k) return fail("ss_op_stoi_compact: null pointer: k_dev");
    if (!xp) return fail("ss_op_stoi_compact: null pointer: xp_dev");
    if (!yp) return fail("ss_op_stoi_compact: null pointer: yp_dev");
    CHK(stoi_rows("ss_op_stoi_compact", B, max_n));
    stoi_tables(&lo, &hi, 1, &tb);
    HIPCHK(stoi_compact(x, y, n, B, max_n, tb, from_map != 0, e, inv, k, xp, yp, S(stream)));
    return 0;
}

int ss_op_stoi_bands(const double* sig, const int* len, int B, int max_len, const int* band_lo, const int* band_hi, int n_bands, double* env,
                     void* stream) {
    StoiTables tb;
    if (!sig) return fail("ss_op_stoi_bands: null pointer: sig_dev");
    if (!env) return fail("ss_op_stoi_bands: null pointer: env_dev");
    if (B < 1 || B > STOI_MAX_ROWS) return fail("ss_op_stoi_bands: B outside 1 .. 65535");
    if (max_len < STOI_FRAME + 1) return fail("ss_op_stoi_bands: max_len below 257 (no transform frame starts strictly below max_len - 256)");
    CHK(stoi_band_table("ss_op_stoi_bands", band_lo, band_hi, n_bands, &tb));
    HIPCHK(stoi_bands(sig, len, B, max_len, tb, env, S(stream)));
    return 0;
}

}  // extern "C"
