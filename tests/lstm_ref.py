"""Float64 yardsticks of one bidirectional LSTM recurrence, the input scenarios, the per-step checks and their bars, shared by
test_gpu_lstm_steps.py (the HIP recurrence kernels) and test_lstm_ref_selftest.py (which proves on the CPU that the checks accept two correct
fp32 restatements and report every wrong variant listed there).  Plain numpy; importing it needs no GPU.

Layout (speechsplit_amd.engine.blstm_recurrence): pre / act / dgates [B, T, 8H] -- the forward direction in columns [0, 4H), the reverse
direction in [4H, 8H), gate order i, f, g, o; out / csave / d_out [B, T, 2H]; w_hh = (forward, reverse) [4H, H].  The forward direction walks
t = 0 .. T-1, the reverse direction T-1 .. 0 (a ragged row: len-1 .. 0), both from the zero state:
    i, f, o = sigmoid(pre + W_hh h_prev)   g = tanh(pre + W_hh h_prev)   c = f c_prev + i g   h = o tanh(c)

An ulp is 2^-23 times the magnitude named (ULP); every bar also admits FLT_MIN = 2^-126 absolute, the one floor of the fp32 format: below the
smallest normal number a result may be kept or flushed to zero and both are correct.

Forward step checks -- elementwise on the kernel's OWN fp32 act / csave / out, so they hold for any W_hh:
  F1  |c_t - (f_t c_prev + i_t g_t)| <= 2 ulp of (|f c_prev| + |i g|): two roundings or one fma.  c_prev is the neighbouring frame in the
      direction's walking order, 0 at its start.
  F2  |h_t - o_t tanh64(c_t)| <= 4 ulp of |o_t tanh64(c_t)|: the header (csrc/common.h) claims ~3 ulp for ss_tanh, the product adds 1/2.
  F3  (W_hh = 0 only) |act - float64 sigmoid / tanh of pre| <= 2 ulp at scale 1 (2.4e-7, the header's claim for ss_sigmoid) for i, f, o and
      twice that for g = 2 r - 1.
The bars are the header's documented claims, not measurements of a kernel.  Measured on the CPU for the header's formulas with correctly
rounded exp2 / rcp (the hardware's add about one ulp each, so the bars leave about 2x headroom) over all scenarios at B = 3, H = 8 and 32,
T = 48 (MEASURED below, as fractions of each bar; the self-test re-measures and holds them): F1 0.47; F2 0.64 = 5.1 * 2^-24 relative; F3
0.38 = 1.5 * 2^-24 for the sigmoid gates and 0.38 = 3.0 * 2^-24 for g.  (torch's own fp32 functions: 0.47, 0.24, 0.38, 0.07.)

Backward checks:
  B1  (W_hh = 0) the backward has a closed form on the forward's saved state, walked against each direction's forward order:
          dc_t = d_out_t o (1 - tc^2) + dc_next f_next        tc = tanh(c_t)             d_o = d_out tc o (1 - o)
          d_i = dc g i (1 - i)      d_f = dc c_prev f (1 - f)      d_g = dc i (1 - g^2)
      evaluated in float64 from the kernel's own act and csave; E is the same recursion on absolute values with every 1 - x^2 replaced by
      1 + x^2 (the magnitude whose rounding the differences carry).  Assert |dgates - ref| <= K_B1 (steps walked + 4) 2^-24 E elementwise.
      K_B1: the backward restated in fp32 on the CPU over all scenarios, d_out >= 0 and signed, H = 8 and 32, T = 48, gives a worst ratio
      of 0.741 with torch's own functions (B1_TORCH) and 0.806 with the header's formulas (B1_HEADER); K_B1 = 2 x the larger, rounded up to
      1.62 -- the doubling covers the hardware's rcp / exp2 inside ss_tanh, which the CPU restatements round correctly.
  B2  the chain budget at trained-scale weights (W_hh ~ U(+-ws / sqrt(H)), ws in {3, 6}, pre = randn ws): out, dgates and
      dW_hh = dgates^T h_prev (float64 products on both sides) against the float64 recurrence, max-norm per tensor relative to the
      reference's largest magnitude: error <= max(8 x the error of the fp32 restatement with torch's functions on the same inputs,
      4 * 2^-24).  The factor: 4 for 22-bit against 24-bit products, 2 for one draw's sampling noise.  Deliberately coarse (the guard for
      the 1e-6 .. 1e-4 band); F1 .. F3 and B1 are the sharp checks.

The recurrent products per step -- any W_hh, every family; q is the family's operand rounding (recurrent_operands: exact for lstm_small /
lstm_step; f16x2 for lstm_seq, hi = fp16(x) and lo = fp16(x - hi) of h 2^14, W_hh 2^4 and da 2^s (s per utterance and 16-unit block, the
block's maximum in [2^7, 2^8)), products hi.lo + lo.hi + hi.hi; f16hi under hi_only, hi.hi alone; the tagged forward hand-off forces bit 0
of every even-k piece to tag_of(step), emulated exactly):
  F4  a = pre + sum_k q(h_k) q(w_k) in float64 from the kernel's OWN out (the neighbouring frame in walking order, zero at the start);
      |act - f64(a)| <= F3's bar + slope 2^-24 (K_F4 M + 2 (c_split P + P_even)), f64 the float64 sigmoid / tanh, slope its derivative at a,
      P = sum |q(h_k) q(w_k)|, M = |pre| + P, P_even the same sum over even k on a tagged f16x2 hand-off (0 otherwise).  c_split is derived:
      0 for exact and f16hi (the emulation is exact), 3 for f16x2 (two operand roundings at 22 bits and the dropped lo.lo), so 4 on the
      even k of a tagged hand-off.  The inputs being the kernel's own fp32 h, no operand rounding can flip between kernel and reference:
      the check does not see the chain's amplification.  K_F4 covers the fp32 accumulation order: an fp32 restatement that adds the exact
      products one after another (the least favourable order; MFMA's blockwise order is better), with the header's formulas, on
      trained(B, T, H, ws), ws 3 and 6, at (5, 40, 256) and (3, 24, 64) in every operand mode gives a worst ratio at k = 1 of 2.236
      (F4_SEQUENTIAL = 2.24, rounded up in the third digit like B1_HEADER); K_F4 = 2 x that = 4.48, K_B1's convention.  The header's numpy
      restatement is the recorded one because it is plain elementwise numpy: the figure does not depend on a library's vectorised sigmoid.
  B3  B1 for any W_hh: dh_t = d_out_t + sum q(da_next) q(w), da_next the kernel's OWN dgates of the step walked before (zero at the walk's
      start), then B1's closed form with dh_t in the place of d_out_t.  E gains sum |q(da) q(w)|; bar K_B1 (steps walked + 4) 2^-24 E + X,
      X = 2^-24 (K_F4 + c_split) sum |q(da) q(w)| carried through the same recursion.  The backward's step tag sits in bit 0 of the fp32
      partial sums, not in an operand: one ulp of a partial sum, inside K_F4.
Side outputs of the persistent kernels, each from the run's own dgates / out: block_sums (SeqBwd::dgs: fp32, direction 0 adds t descending,
direction 1 ascending, each sum started from +0 as the kernel starts it), bias_sums / check_gbias (float64 column sums per 16-utterance
tile; bar (nbt + 1) 2^-23 (|g0| + sum |S_tile|): one fp32 rounding per tile sum and one per atomic add, generous by about 2x), bf16_bits
(round to nearest even, a NaN stays a NaN), amax_bits.
check_b2_hi, the coarse chain check of the 16-bit data path: error of out / dgates / dW_hh against layer64 <= 4 x the error of layer16
(the float64 recurrence with the f16hi operand rounding, untagged) on the same inputs -- x 2 because a tagged even element is off by up to
one fp16 ulp instead of half, x 2 for one draw's sampling noise.  A cap, so the inputs must keep a correct kernel inside and a wrong one
outside: with the exact emulation, at (5, 40, 256), (17, 40, 256), (16, 24, 512) and ws 3 and 6 the tagged layer16 is 1.08 .. 1.68 x the
untagged error (held: <= 2.6) and a bf16-wide operand 5.6 .. 10.1 x (held: > 4).
Every check returns its worst error / bar ratio (a pass is <= 1; anything non-finite gives inf), so that a test can print before it asserts.
"""
import numpy as np

F32 = np.float32
ULP = 2.0 ** -23
FLT_MIN = 2.0 ** -126
K_B1 = 1.62
B1_TORCH, B1_HEADER = 0.741, 0.806          # worst B1 ratios (k = 1) of the two correct fp32 restatements, see the docstring
MEASURED = dict(F1=0.47, F2=0.64, F3_sigmoid=0.38, F3_g=0.38)      # header restatement, fraction of each bar; the self-test holds them
B2_FACTOR, B2_FLOOR = 8.0, 4 * 2.0 ** -24
HSCALE, WSCALE = 16384.0, 16.0              # csrc/lstm_seq.hip: the fixed scales of h and W_hh in front of the fp16 split
F4_SEQUENTIAL = 2.24                        # worst F4 ratio (k = 1) of the sequential-order fp32 restatement (2.236), see the docstring
K_F4 = 4.48                                 # 2 x F4_SEQUENTIAL
B2_HI_FACTOR = 4.0                          # check_b2_hi: 2 (a tagged even element is off by up to one fp16 ulp, not half) x 2 (one draw)
B2_HI_TAGGED, B2_HI_BF16 = 2.6, 4.0         # the self-test holds: tagged / untagged layer16 error <= 2.6, bf16-wide operand > 4
SCENARIOS = ('sweep', 'smallc', 'grow', 'reset', 'extreme')


# ------------------------------------------------------------------------------------------------ scenarios
def scenario(name, B, T, H, seed=0):
    """Seeded pre-activations [B, T, 8H] (float32) of one scenario."""
    rng = np.random.default_rng([seed, SCENARIOS.index(name), B, T, H])
    p = np.empty((B, T, 2, 4, H))
    if name in ('sweep', 'extreme', 'reset'):
        s = np.logspace(-3, np.log10(40.0), 2 * H).reshape(2, 1, H)        # unit n of each gate: U(-s_n, s_n), over both directions
        p[:] = rng.uniform(-1, 1, p.shape) * s
    if name == 'smallc':        # i small, o open, f in 0.2 .. 0.95: cells of 0.01 .. 1 on both sides of the |c| = 0.7 branch of ss_tanh
        p[:] = rng.standard_normal(p.shape) * 0.5
        p[:, :, :, 0] -= 2.0
        p[:, :, :, 3] += 3.0
        p[:, :, :, 1] += rng.uniform(0.0, 3.0, (B, 1, 2, H))
        p[:, :, :, 2] = p[:, :, :, 2] * 2.0 + rng.choice([-2.0, 2.0], (B, 1, 2, H))
    if name == 'grow':          # i = f = 1 - 6e-6, g = 1 - 1e-5: the cells ramp by about 1 per step to |c| ~ T
        p[:] = rng.standard_normal(p.shape)
        p[:, :, :, :2] += 12.0
        p[:, :, :, 2] += 6.0
    if name == 'reset':         # the forget gate alternates between shut and open per frame
        p[:, :, :, 1] = np.where(np.arange(T) % 2 == 0, -12.0, 12.0).reshape(1, T, 1, 1)
    if name == 'extreme':       # exact overflow / underflow points of exp2 among the sweep
        vals = np.array([300.0, -300.0, 88.0, -88.0, 0.0, -0.0, 1e-40, -1e-40])
        flat = p.reshape(-1)
        idx = rng.choice(flat.size, size=max(flat.size // 4, 8 * len(vals)) // len(vals) * len(vals), replace=False)
        flat[idx] = np.tile(vals, idx.size // len(vals))
    return np.ascontiguousarray(p.reshape(B, T, 8 * H).astype(F32))


def d_out_for(B, T, H, signed, seed=0):
    """Output gradient [B, T, 2H] (float32): |randn| (every term of dc non-negative: E equals the value) or randn."""
    d = np.random.default_rng([seed, 77, B, T, H]).standard_normal((B, T, 2 * H))
    return (d if signed else np.abs(d)).astype(F32)


def trained(B, T, H, ws, seed=0):
    """B2's inputs: (pre, (w_hh forward, reverse), d_out) at weight scale ws."""
    rng = np.random.default_rng([seed, 99, B, T, H, int(ws)])
    pre = (rng.standard_normal((B, T, 8 * H)) * ws).astype(F32)
    w = tuple((rng.uniform(-1, 1, (4 * H, H)) * ws / np.sqrt(H)).astype(F32) for _ in range(2))
    return pre, w, (rng.standard_normal((B, T, 2 * H)) * 1e-3).astype(F32)


# ------------------------------------------------------------------------------------------------ geometry
def _parts(a, H, d):
    """The four gate planes [B, T, H] of direction d."""
    return [a[:, :, d * 4 * H + g * H:d * 4 * H + (g + 1) * H] for g in range(4)]


def _prev(x, d, lengths=None):
    """x [B, T, H] of direction d -> the previous frame's value in the direction's walking order, 0 at its start."""
    p = np.zeros_like(x)
    if d == 0:
        p[:, 1:] = x[:, :-1]
    else:
        p[:, :-1] = x[:, 1:]
        if lengths is not None:
            for b, n in enumerate(lengths):
                if 0 < n <= x.shape[1]:
                    p[b, n - 1] = 0
    return p


def _mask(B, T, lengths):
    m = np.ones((B, T, 1), bool)
    if lengths is not None:
        m = (np.arange(T)[None, :] < np.asarray(lengths)[:, None])[:, :, None]
    return m


def _worst(err, bar, mask=None):
    with np.errstate(all='ignore'):
        r = err / bar
    r = np.where(np.isfinite(r), r, np.inf)
    if mask is not None:
        r = np.where(mask, r, 0.0)
    return float(r.max()) if r.size else 0.0


sigmoid64 = lambda x: np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


# ------------------------------------------------------------------------------------------------ the checks
def check_f1(act, csave, lengths=None):
    """F1: worst |c - (f c_prev + i g)| / (2 ulp of (|f c_prev| + |i g|) + FLT_MIN) inside each row's length."""
    act, csave = np.asarray(act, np.float64), np.asarray(csave, np.float64)
    B, T, H = csave.shape[0], csave.shape[1], csave.shape[2] // 2
    worst = 0.0
    for d in range(2):
        i, f, g, _ = _parts(act, H, d)
        c = csave[:, :, d * H:(d + 1) * H]
        cp = _prev(c, d, lengths)
        worst = max(worst, _worst(np.abs(c - (f * cp + i * g)), 2 * ULP * (np.abs(f * cp) + np.abs(i * g)) + FLT_MIN, _mask(B, T, lengths)))
    return worst


def check_f2(act, csave, out, lengths=None):
    """F2: worst |h - o tanh64(c)| / (4 ulp of |o tanh64(c)| + FLT_MIN) inside each row's length."""
    act, csave, out = np.asarray(act, np.float64), np.asarray(csave, np.float64), np.asarray(out, np.float64)
    B, T, H = csave.shape[0], csave.shape[1], csave.shape[2] // 2
    worst = 0.0
    for d in range(2):
        o = _parts(act, H, d)[3]
        ref = o * np.tanh(csave[:, :, d * H:(d + 1) * H])
        worst = max(worst, _worst(np.abs(out[:, :, d * H:(d + 1) * H] - ref), 4 * ULP * np.abs(ref) + FLT_MIN, _mask(B, T, lengths)))
    return worst


def check_f3(pre, act, lengths=None):
    """F3 (W_hh = 0): worst absolute error of the activated gates over its bar, (sigmoid gates: 2 ulp at scale 1, g gate: 4 ulp)."""
    pre, act = np.asarray(pre, np.float64), np.asarray(act, np.float64)
    B, T, H = pre.shape[0], pre.shape[1], pre.shape[2] // 8
    ws = wg = 0.0
    for d in range(2):
        for k, (p, a) in enumerate(zip(_parts(pre, H, d), _parts(act, H, d))):
            if k == 2:
                wg = max(wg, _worst(np.abs(a - np.tanh(p)), 4 * ULP, _mask(B, T, lengths)))
            else:
                ws = max(ws, _worst(np.abs(a - sigmoid64(p)), 2 * ULP, _mask(B, T, lengths)))
    return ws, wg


def tail_is_zero(x, lengths):
    """out / csave of a ragged forward hold zeros behind each row's length."""
    return all(not np.asarray(x)[b, n:].any() for b, n in enumerate(lengths))


def b1_reference(act, csave, d_out):
    """(ref, bound) [B, T, 8H] float64: the closed-form W_hh = 0 backward on the saved state and (steps walked + 4) 2^-24 E + FLT_MIN."""
    act, csave, d_out = np.asarray(act, np.float64), np.asarray(csave, np.float64), np.asarray(d_out, np.float64)
    B, T, H = csave.shape[0], csave.shape[1], csave.shape[2] // 2
    ref, bound = np.zeros_like(act), np.zeros_like(act)
    for d in range(2):
        i, f, g, o = _parts(act, H, d)
        c = csave[:, :, d * H:(d + 1) * H]
        cp = _prev(c, d)
        tc = np.tanh(c)
        dc = np.zeros((B, H))
        edc = np.zeros((B, H))
        walk = range(T - 1, -1, -1) if d == 0 else range(T)
        for s, t in enumerate(walk):
            nxt = t + 1 if d == 0 else t - 1
            fn = f[:, nxt] if 0 <= nxt < T else 0.0
            do = d_out[:, t, d * H:(d + 1) * H]
            dc = do * o[:, t] * (1 - tc[:, t] ** 2) + dc * fn
            edc = np.abs(do) * o[:, t] * (1 + tc[:, t] ** 2) + edc * fn
            vals = (dc * g[:, t] * i[:, t] * (1 - i[:, t]), dc * cp[:, t] * f[:, t] * (1 - f[:, t]), dc * i[:, t] * (1 - g[:, t] ** 2),
                    do * tc[:, t] * o[:, t] * (1 - o[:, t]))
            es = (edc * np.abs(g[:, t]) * i[:, t] * (1 - i[:, t]), edc * np.abs(cp[:, t]) * f[:, t] * (1 - f[:, t]),
                  edc * i[:, t] * (1 + g[:, t] ** 2), np.abs(do * tc[:, t]) * o[:, t] * (1 - o[:, t]))
            for k in range(4):
                col = slice(d * 4 * H + k * H, d * 4 * H + (k + 1) * H)
                ref[:, t, col] = vals[k]
                bound[:, t, col] = (s + 1 + 4) * 2.0 ** -24 * es[k] + FLT_MIN
    return ref, bound


def check_b1(act, csave, d_out, dgates, k=K_B1):
    """B1: worst |dgates - ref| / (k x the running bound)."""
    ref, bound = b1_reference(act, csave, d_out)
    return _worst(np.abs(np.asarray(dgates, np.float64) - ref), k * bound)


# ------------------------------------------------------------------------------------------------ recurrent operands, F4 and B3
def tag_of(st):
    """csrc/lstm_seq.hip tag_of: the tag bit of the payload consumed at walking step st >= 1 (1, 1, 0, 0, 1, 1, ...)."""
    return (((np.asarray(st) - 1) >> 1) + 1) & 1


def _f16(y):
    with np.errstate(all='ignore'):
        return np.asarray(y, F32).astype(np.float16)


def _force_bit0(h16, tag):
    """fp16 array with bit 0 of every element's pattern replaced by tag (broadcast)."""
    bits = (h16.view(np.uint16) & np.uint16(0xFFFE)) | np.broadcast_to(np.asarray(tag, np.uint16), h16.shape)
    return bits.astype(np.uint16).view(np.float16)


def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; a NaN stays a NaN (quiet bit set, as v_cvt_pk_bf16_f32 gives it)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(np.asarray(x, F32)), ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_value(bits):
    """bf16 bit patterns -> float32."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


class Operands:
    """How one kernel family rounds the two operands of its recurrent products (recurrent_operands builds it).  Every method returns a
    pair (hi, lo) of float64 arrays in the operand's own units; the product taken is hi.lo + lo.hi + hi.hi (mfma3_each; lo.lo is never
    formed), hi.hi alone for f16hi and the plain product for exact.  The class attributes below are the self-test's wrong variants."""
    drop_lohi = bf16_width = skip_chunk = tag_odd = da_row_scale = w_untransposed = False

    def __init__(self, mode, tagged, H):
        assert mode in ('exact', 'f16x2', 'f16hi') and (mode == 'exact' or H % 32 == 0), (mode, H)
        self.mode, self.tagged, self.H = mode, bool(tagged) and mode != 'exact', H
        self.c_split = 3.0 if mode == 'f16x2' else 0.0
        self.c_tag = 1.0 if mode == 'f16x2' and self.tagged else 0.0            # even k of a tagged hand-off: c_split = 4 there

    def _split(self, y, tag=None):
        """y (already scaled, fp32) -> its fp16 pieces as float64; tag (0 / 1, broadcast): forced into bit 0 of the even-k pieces."""
        y = np.asarray(y, F32)
        if self.bf16_width:
            y = bf16_value(bf16_bits(y))
        if self.mode == 'exact':
            return _d(y), np.zeros(y.shape)
        hi = _f16(y)
        if tag is not None:
            k = (np.arange(y.shape[-1]) % 2 == (1 if self.tag_odd else 0))
            hi = np.where(k, _force_bit0(hi, tag), hi)
        if self.mode == 'f16hi':
            return _d(hi), np.zeros(y.shape)
        with np.errstate(all='ignore'):
            lo = _f16(y - hi.astype(F32))
        if tag is not None:
            lo = np.where(k, _force_bit0(lo, tag), lo)
        return _d(hi), _d(lo)

    def h(self, h, st):
        """Pieces of h(st - 1) as the step st >= 1 (int or array broadcast against h's leading axes) of the walk consumes them."""
        s = 1.0 if self.mode == 'exact' else HSCALE
        tag = tag_of(st) if self.tagged else None
        if tag is not None and np.ndim(tag):
            tag = np.asarray(tag)[..., None]
        return tuple(p / s for p in self._split(np.asarray(h, F32) * F32(s), tag))

    def w(self, w):
        """Pieces of W_hh [4H, H]."""
        s = 1.0 if self.mode == 'exact' else WSCALE
        return tuple(p / s for p in self._split(np.asarray(w, F32) * F32(s)))

    def w_backward(self, w):
        """... as the backward's product da [B, 4H] . W_hh [4H, H] reads them."""
        w = np.asarray(w, F32)
        if self.w_untransposed:
            w = np.concatenate([w[g * self.H:(g + 1) * self.H].T for g in range(4)])
        return self.w(w)

    def da_scale(self, da, per_row=False):
        """The power of two per utterance and 16-unit column block (all four gates of the block) that brings the block's largest
        magnitude into [2^7, 2^8), capped like the kernel's: [..., 4H] -> the same shape."""
        da = np.asarray(da, F32)
        v = np.abs(da).reshape(da.shape[:-1] + (4, self.H // 16, 16))
        m = v.max(axis=(-3, -2, -1) if per_row else (-3, -1), keepdims=True)
        se = np.clip(261 - (np.ascontiguousarray(m, F32).view(np.uint32) >> np.uint32(23)).astype(np.int64), 1, 187)
        return np.broadcast_to(np.exp2(_d(se - 127)), v.shape).reshape(da.shape)

    def da(self, da):
        """Pieces of the pre-activation gradients of one step and direction [..., 4H] (gate-major)."""
        if self.mode == 'exact':
            return self._split(da)
        sc, un = self.da_scale(da, self.da_row_scale), self.da_scale(da)
        with np.errstate(all='ignore'):
            return tuple(p / un for p in self._split((_d(np.asarray(da, F32)) * sc).astype(F32)))

    def _terms(self, a, wk):
        (ah, al), (wh, wl) = a, wk
        if self.skip_chunk:
            ah, al = ah.copy(), al.copy()
            ah[..., 32:64] = 0
            al[..., 32:64] = 0
        if self.mode != 'f16x2':
            return [(ah, wh)]
        return [(ah, wl)] + ([] if self.drop_lohi else [(al, wh)]) + [(ah, wh)]

    def product(self, a, wk, dt=np.float64, sequential=False):
        """sum over k of the family's products of a [.., K] and wk [K, N] (pieces): exact in float64, or an fp32 restatement -- fp32
        matrix products of the pieces, or with sequential the exact products added one after another in fp32 (the least favourable order)."""
        terms = self._terms(a, wk)
        if sequential:
            acc = np.zeros(terms[0][0].shape[:-1] + (terms[0][1].shape[1],), F32)
            for k in range(terms[0][0].shape[-1]):
                for x, y in terms:
                    acc = _r(_d(acc) + x[..., k:k + 1] * y[k:k + 1])
            return acc
        with np.errstate(all='ignore'):
            return sum(np.asarray(x, dt) @ np.asarray(y, dt) for x, y in terms)

    def magnitude(self, a, wk, even_only=False):
        """sum over k of |the products| (the magnitude whose rounding the sum carries); even_only: over even k."""
        sl = slice(None, None, 2) if even_only else slice(None)
        return sum(np.abs(x[..., sl]) @ np.abs(y[sl]) for x, y in self._terms(a, wk))


def recurrent_operands(mode, tagged=False, H=32):
    """The operand rounding of a kernel family's recurrent products, read from the code:
      exact  csrc/lstm_small.hip, lstm_step.hip: fp32 operands (fma chains / v_mfma_f32_16x16x4_f32).
      f16x2  csrc/lstm_seq.hip: h HSCALE and W WSCALE (forward), da (block scale) and W WSCALE (backward) split into hi = fp16(x) to
             nearest and lo = fp16(x - hi); products hi.lo, lo.hi, hi.hi.
      f16hi  the same kernels under hi_only: the high pieces alone.
    tagged (forward hand-off under seq_tag = 1, xb_store): bit 0 of every even-k high piece is tag_of(step); in f16x2 the low piece is
    taken from what is then left and tagged likewise.  The backward's da is never tagged (its tag sits in the fp32 partial sums)."""
    return Operands(mode, tagged, H)


def operands_of(H, knobs=None, hi_only=False, B=1):
    """The Operands of the kernel family engine.blstm_recurrence selects at hidden size H (csrc/lstm_seq.hip lstm_seq_supported: the
    persistent kernels at H = 256 and 512 unless persist = 0; lstm_seq_fwd: the tagged hand-off under seq_tag = 1 where the 2 ceil(B / 16)
    groups are expected on one XCD each -- up to 8 groups, or a multiple of 8).  Everything else -- H = 64 and 128, and H = 256 / 512 under
    persist = 0 -- runs csrc/lstm_step.hip, whose operands are `exact` in every instance: lstm_nw (waves that split K) and lstm_g (16-wide
    chunks requested ahead) move loads between waves and in time, every operand of v_mfma_f32_16x16x4_f32 is the fp32 word in memory, so
    both keys are ignored here.  (They do change where the fp32 sum is cut: that is what F4 / B3's summation term covers.)"""
    knobs = knobs or {}
    if H in (256, 512) and knobs.get('persist', 1):
        groups = 2 * ((B + 15) // 16)
        return recurrent_operands('f16hi' if hi_only else 'f16x2', knobs.get('seq_tag', 1) and (groups <= 8 or groups % 8 == 0), H)
    return recurrent_operands('exact', False, H)


def _f3_bar(H):
    return np.concatenate([np.full(H, 2 * ULP), np.full(H, 2 * ULP), np.full(H, 4 * ULP), np.full(H, 2 * ULP)])


def f4_reference(pre, out, w_hh, ops, wrong_neighbour=False):
    """F4's float64 pre-activations a = pre + sum_k q(h_k) q(w_k) from the kernel's OWN out, with M = |pre| + sum |q(h_k) q(w_k)| and
    the same sum over the even k: three arrays [B, T, 8H]."""
    pre, out = np.asarray(pre, F32), np.asarray(out, F32)
    B, T, H = pre.shape[0], pre.shape[1], pre.shape[2] // 8
    a, M, Me = np.zeros(pre.shape), np.zeros(pre.shape), np.zeros(pre.shape)
    for d in range(2):
        hp = _prev(out[:, :, d * H:(d + 1) * H], (d if not wrong_neighbour else 1 - d))
        st = np.arange(T) if d == 0 else T - 1 - np.arange(T)
        first = (st == 0)[None, :, None]
        hq = tuple(np.where(first, 0.0, p) for p in ops.h(hp, np.maximum(st, 1)[None, :]))
        wk = tuple(x.T for x in ops.w(w_hh[d]))
        col = slice(d * 4 * H, (d + 1) * 4 * H)
        a[:, :, col] = _d(pre[:, :, col]) + ops.product(hq, wk)
        M[:, :, col] = np.abs(_d(pre[:, :, col])) + ops.magnitude(hq, wk)
        Me[:, :, col] = ops.magnitude(hq, wk, even_only=True)
    return a, M, Me


def check_f4(pre, act, out, w_hh, ops, k=None):
    """F4: worst |act - f64(a)| / (F3's bar + slope 2^-24 (K_F4 M + 2 (c_split M_products + M_even on a tagged f16x2 hand-off)))."""
    k = K_F4 if k is None else k
    a, M, Me = f4_reference(pre, out, w_hh, ops)
    H = a.shape[2] // 8
    Mp = M - np.abs(_d(np.asarray(pre, F32)))
    is_g = np.tile(np.concatenate([np.zeros(2 * H, bool), np.ones(H, bool), np.zeros(H, bool)]), 2)
    with np.errstate(all='ignore'):
        ref = np.where(is_g, np.tanh(a), sigmoid64(a))
        slope = np.where(is_g, 1 - ref * ref, ref * (1 - ref))
    bar = np.tile(_f3_bar(H), 2) + slope * 2.0 ** -24 * (k * M + 2 * (ops.c_split * Mp + ops.c_tag * Me))
    return _worst(np.abs(_d(act) - ref), bar)


def b3_reference(act, csave, d_out, dgates, w_hh, ops, k1=None, k4=None):
    """(ref, bound) [B, T, 8H] float64: B1's closed form with dh_t = d_out_t + sum q(da_next) q(w) in the place of d_out_t, da_next the
    kernel's OWN dgates of the step walked before (zero at the walk's start), and
    K_B1 (steps walked + 4) 2^-24 E + X + FLT_MIN, E B1's magnitude recursion with |d_out| + sum |q(da) q(w)| and X the same recursion
    started from 2^-24 (K_F4 + c_split) sum |q(da) q(w)|."""
    k1, k4 = K_B1 if k1 is None else k1, K_F4 if k4 is None else k4
    act, csave, d_out = np.asarray(act, np.float64), np.asarray(csave, np.float64), np.asarray(d_out, np.float64)
    dgates = np.asarray(dgates, F32)
    B, T, H = csave.shape[0], csave.shape[1], csave.shape[2] // 2
    ref, bound = np.zeros_like(act), np.zeros_like(act)
    for d in range(2):
        i, f, g, o = _parts(act, H, d)
        c = csave[:, :, d * H:(d + 1) * H]
        cp = _prev(c, d)
        tc = np.tanh(c)
        da_next = _prev(dgates[:, :, d * 4 * H:(d + 1) * 4 * H], 1 - d)           # the backward walks against the forward's order
        aq, wk = ops.da(da_next), ops.w_backward(w_hh[d])
        prod, pm = ops.product(aq, wk), ops.magnitude(aq, wk)
        dh_all, edh_all, xdh_all = d_out[:, :, d * H:(d + 1) * H] + prod, np.abs(d_out[:, :, d * H:(d + 1) * H]) + pm, 2.0 ** -24 * (k4 + ops.c_split) * pm
        dc, edc, xdc = np.zeros((B, H)), np.zeros((B, H)), np.zeros((B, H))
        walk = range(T - 1, -1, -1) if d == 0 else range(T)
        for s, t in enumerate(walk):
            nxt = t + 1 if d == 0 else t - 1
            fn = f[:, nxt] if 0 <= nxt < T else 0.0
            dh, edh, xdh = dh_all[:, t], edh_all[:, t], xdh_all[:, t]
            dc = dh * o[:, t] * (1 - tc[:, t] ** 2) + dc * fn
            edc = edh * o[:, t] * (1 + tc[:, t] ** 2) + edc * fn
            xdc = xdh * o[:, t] * (1 + tc[:, t] ** 2) + xdc * fn
            vals = (dc * g[:, t] * i[:, t] * (1 - i[:, t]), dc * cp[:, t] * f[:, t] * (1 - f[:, t]), dc * i[:, t] * (1 - g[:, t] ** 2),
                    dh * tc[:, t] * o[:, t] * (1 - o[:, t]))
            fac = (np.abs(g[:, t]) * i[:, t] * (1 - i[:, t]), np.abs(cp[:, t]) * f[:, t] * (1 - f[:, t]), i[:, t] * (1 + g[:, t] ** 2),
                   np.abs(tc[:, t]) * o[:, t] * (1 - o[:, t]))
            for q in range(4):
                col = slice(d * 4 * H + q * H, d * 4 * H + (q + 1) * H)
                e, x = (edc, xdc) if q < 3 else (edh, xdh)
                ref[:, t, col] = vals[q]
                bound[:, t, col] = (k1 * (s + 1 + 4) * 2.0 ** -24 * e + x) * fac[q] + FLT_MIN
    return ref, bound


def check_b3(act, csave, d_out, dgates, w_hh, ops, k1=None, k4=None):
    """B3: worst |dgates - ref| / bound."""
    ref, bound = b3_reference(act, csave, d_out, dgates, w_hh, ops, k1, k4)
    return _worst(np.abs(np.asarray(dgates, np.float64) - ref), bound)


# ------------------------------------------------------------------------------------------------ side outputs of the persistent kernels
def block_sums(dgates, xf):
    """SeqBwd::dgs from the run's own dgates [B, T, 8H]: float32 sums per block of xf frames as the storing wave forms them
    (csrc/lstm_seq.hip: bsm = 0, then bsm += v per step) -- direction 0 adds t descending, direction 1 ascending, each sum started from +0,
    so a block of -0 addends gives +0 and xf = 1 gives 0 + dgates: [B, T / xf, 8H] float32."""
    dg = np.asarray(dgates, F32)
    B, T, C = dg.shape
    blocks = dg.reshape(B, T // xf, xf, C)
    res = np.empty((B, T // xf, C), F32)
    for d in range(2):
        col = slice(d * C // 2, (d + 1) * C // 2)
        acc = np.zeros((B, T // xf, C // 2), F32)
        for j in (range(xf - 1, -1, -1) if d == 0 else range(xf)):
            acc = (acc + blocks[:, :, j, col]).astype(F32)
        res[:, :, col] = acc
    return res


def bias_sums(dgates, nbt):
    """Float64 column sums of dgates [B, T, 8H] per tile of 16 utterances: [nbt, 8H]."""
    dg = np.asarray(dgates, np.float64)
    return np.stack([dg[16 * k:16 * (k + 1)].sum(axis=(0, 1)) for k in range(nbt)])


def check_gbias(got, g0, dgates, nbt):
    """SeqBwd::gbias_* pre-filled with g0 [8H]: worst |got - (g0 + sum over tiles S_tile)| / ((nbt + 1) 2^-23 (|g0| + sum |S_tile|)) --
    one fp32 rounding of each tile's float64 sum and one per atomic add, generous by about 2x."""
    S = bias_sums(dgates, nbt)
    g0 = np.asarray(g0, np.float64)
    return _worst(np.abs(np.asarray(got, np.float64) - (g0 + S.sum(0))), (nbt + 1) * ULP * (np.abs(g0) + np.abs(S).sum(0)) + FLT_MIN)


def amax_bits(dgates):
    """SeqBwd::amax started at 0: the bit pattern of the largest |dgates| (uint32)."""
    return int(np.abs(np.asarray(dgates, F32)).max().view(np.uint32))


def check_b2_hi(got, ref64, ref16):
    """The coarse chain check of the 16-bit data path: {tensor: (error, error of layer16(tagged=False), ratio to B2_HI_FACTOR x it)}."""
    res = {}
    for name in got.keys() & {'out', 'dgates', 'dw_hh'}:
        e, e16 = max_norm_error(got[name], ref64[name]), max_norm_error(ref16[name], ref64[name])
        res[name] = (e, e16, e / (B2_HI_FACTOR * e16))
    return res


# ------------------------------------------------------------------------------------------------ the float64 layer (B2's reference)
def dw_hh(dgates, out):
    """dW_hh = dgates^T h_prev per direction in float64: [2, 4H, H]."""
    dgates, out = np.asarray(dgates, np.float64), np.asarray(out, np.float64)
    H = out.shape[2] // 2
    return np.stack([np.einsum('btg,bth->gh', dgates[:, :, d * 4 * H:(d + 1) * 4 * H], _prev(out[:, :, d * H:(d + 1) * H], d)) for d in range(2)])


def layer64(pre, w_hh, d_out=None):
    """The recurrence and its BPTT in float64 (what torch.nn.LSTM computes; the self-test compares it with torch's own in double):
    dict out, csave, act and, with d_out, dgates and dw_hh."""
    return _layer(pre, w_hh, d_out, np.float64, Formulas64())


def max_norm_error(x, ref):
    """max |x - ref| / max |ref| (inf when x is not finite)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    e = np.abs(x - ref).max() / np.abs(ref).max()
    return float(e) if np.isfinite(e) else float('inf')


def check_b2(got, ref64, ref32):
    """B2: {tensor: (engine error, fp32 restatement's error, ratio to the bar)} for out, dgates, dw_hh."""
    res = {}
    for name in ('out', 'dgates', 'dw_hh'):
        e, e32 = max_norm_error(got[name], ref64[name]), max_norm_error(ref32[name], ref64[name])
        res[name] = (e, e32, e / max(B2_FACTOR * e32, B2_FLOOR))
    return res


# ------------------------------------------------------------------------------------------------ restatements (float64, fp32, wrong variants)
class Formulas64:
    """The gate functions in float64."""
    sigmoid = staticmethod(sigmoid64)
    gate_g = staticmethod(np.tanh)
    tanh_c = staticmethod(np.tanh)
    swap_og = cprev_wrong = f_current = tc_from_h = df_uses_c = False


class TorchF32(Formulas64):
    """torch's own fp32 sigmoid / tanh."""
    @staticmethod
    def _t(fn, x):
        import torch
        return getattr(torch, fn)(torch.from_numpy(np.ascontiguousarray(x, dtype=F32))).numpy()
    sigmoid = classmethod(lambda cls, x: cls._t('sigmoid', x))
    gate_g = classmethod(lambda cls, x: cls._t('tanh', x))
    tanh_c = classmethod(lambda cls, x: cls._t('tanh', x))


def _r(x):
    with np.errstate(all='ignore'):
        return np.asarray(x, np.float64).astype(F32)


_d = lambda x: np.asarray(x, np.float64)
_exp2 = lambda x: _r(np.exp2(_d(x)))                    # correctly rounded stand-ins for the hardware's exp2 / rcp
_rcp = lambda x: _r(1.0 / _d(x))
_fma = lambda a, b, c: _r(_d(a) * _d(b) + _d(c))         # the float64 product of two fp32 numbers is exact


class HeaderF32(Formulas64):
    """csrc/common.h's ss_sigmoid / ss_gate / ss_tanh restated in fp32, operation by operation."""
    thresh = 0.7

    @staticmethod
    def sigmoid(x):
        with np.errstate(all='ignore'):
            return _rcp(F32(1) + _exp2(x * F32(-1.44269504)))

    @staticmethod
    def gate_g(x):
        with np.errstate(all='ignore'):
            return _fma(F32(2), _rcp(F32(1) + _exp2(x * F32(2) * F32(-1.44269504))), F32(-1))

    @classmethod
    def tanh_c(cls, x):
        with np.errstate(all='ignore'):
            x = np.asarray(x, F32)
            e = _exp2(x * F32(2.88539008))
            q = _fma(F32(-2), _rcp(e + F32(1)), F32(1))
            a = F32(0.5) * x
            y = a * a
            y2 = y * y
            p01, p23 = _fma(y, F32(-0.333333343), F32(1)), _fma(y, F32(-0.0539682545), F32(0.13333334))
            p45 = _fma(y, F32(-0.00886323582), F32(0.0218694881))
            p = a * _fma(y2 * y2, p45, _fma(y2, p23, p01))
            t = (p + p) * _rcp(_fma(p, p, F32(1)))
            return np.where(np.abs(x) < F32(cls.thresh), t, q)


def _layer(pre, w_hh, d_out, dt, fn, ops=None, sequential=False):
    """Forward (and with d_out the BPTT, in the kernels' operation order) of both directions in precision dt with the formulas fn.  ops
    (an Operands, H a multiple of 32): the recurrent products take that family's operand rounding; sequential: they add the exact products
    one after another in fp32 (K_F4's restatement)."""
    pre = np.asarray(pre, dt)
    B, T, H = pre.shape[0], pre.shape[1], pre.shape[2] // 8
    act, out, csave = np.zeros((B, T, 8 * H), dt), np.zeros((B, T, 2 * H), dt), np.zeros((B, T, 2 * H), dt)
    one = dt(1)
    with np.errstate(all='ignore'):
        for d in range(2):
            w = np.asarray(w_hh[d], dt)
            rec = bool(w.any())
            h, c = np.zeros((B, H), dt), np.zeros((B, H), dt)
            wk = None if ops is None else tuple(x.T for x in ops.w(w_hh[d]))
            for st, t in enumerate(range(T) if d == 0 else range(T - 1, -1, -1)):
                p = pre[:, t, d * 4 * H:(d + 1) * 4 * H]
                if rec and ops is None:
                    p = p + h @ w.T
                elif rec and st > 0:                        # the kernels multiply nothing at the first step: h(-1) = 0
                    p = p + ops.product(ops.h(h, st), wk, dt, sequential)
                pi, pf, pg, po = (p[:, k * H:(k + 1) * H] for k in range(4))
                if fn.swap_og:
                    pg, po = po, pg
                gi, gf, gg, go = (np.asarray(x, dt) for x in (fn.sigmoid(pi), fn.sigmoid(pf), fn.gate_g(pg), fn.sigmoid(po)))
                c = gf * c + gi * gg
                h = go * np.asarray(fn.tanh_c(c), dt)
                act[:, t, d * 4 * H:(d + 1) * 4 * H] = np.concatenate([gi, gf, gg, go], 1)
                csave[:, t, d * H:(d + 1) * H] = c
                out[:, t, d * H:(d + 1) * H] = h
    res = dict(out=out, csave=csave, act=act)
    if d_out is not None:
        res['dgates'] = backward(act, csave, out, d_out, w_hh, dt, fn, ops)
        res['dw_hh'] = dw_hh(res['dgates'], out)
    return res


def backward(act, csave, out, d_out, w_hh, dt, fn, ops=None):
    """BPTT on a saved forward state in precision dt, in the kernels' operation order (csrc/lstm_small.hip): dgates [B, T, 8H].  ops: the
    recurrent product da . W_hh with that family's operand rounding."""
    act, csave, out, d_out = (np.asarray(x, dt) for x in (act, csave, out, d_out))
    B, T, H = csave.shape[0], csave.shape[1], csave.shape[2] // 2
    dg = np.zeros((B, T, 8 * H), dt)
    one = dt(1)
    with np.errstate(all='ignore'):
        for d in range(2):
            w = np.asarray(w_hh[d], dt)
            rec = bool(w.any())
            gi, gf, gg, go = _parts(act, H, d)
            wk = None if ops is None else ops.w_backward(w_hh[d])
            c = csave[:, :, d * H:(d + 1) * H]
            cp = _prev(c, d if not fn.cprev_wrong else 0)
            dh_rec, dc_rec = np.zeros((B, H), dt), np.zeros((B, H), dt)
            for t in (range(T - 1, -1, -1) if d == 0 else range(T)):
                dh = d_out[:, t, d * H:(d + 1) * H] + dh_rec
                tc = out[:, t, d * H:(d + 1) * H] / go[:, t] if fn.tc_from_h else np.asarray(fn.tanh_c(c[:, t]), dt)
                d_o = dh * tc
                if fn.f_current:
                    dc_rec = dc_rec * gf[:, t]
                dc = dc_rec + dh * go[:, t] * (one - tc * tc)
                dc_rec = dc if fn.f_current else dc * gf[:, t]
                da = np.concatenate([dc * gg[:, t] * gi[:, t] * (one - gi[:, t]),
                                     dc * (c[:, t] if fn.df_uses_c else cp[:, t]) * gf[:, t] * (one - gf[:, t]),
                                     dc * gi[:, t] * (one - gg[:, t] * gg[:, t]), d_o * go[:, t] * (one - go[:, t])], 1)
                dg[:, t, d * 4 * H:(d + 1) * 4 * H] = da
                if rec:
                    dh_rec = da @ w if ops is None else np.asarray(ops.product(ops.da(da), wk, dt), dt)
    return dg


def layer32(pre, w_hh, d_out=None, fn=TorchF32, ops=None, sequential=False):
    """The recurrence restated in fp32 on the CPU with the formulas fn (TorchF32, HeaderF32 or a wrong variant of the self-test) and, with
    ops, a kernel family's recurrent operand rounding (or a wrong variant of it)."""
    return _layer(pre, w_hh, d_out, F32, fn(), ops, sequential)


def layer16(pre, w_hh, d_out=None, tagged=False, ops=None):
    """check_b2_hi's yardstick: the float64 recurrence whose recurrent products take the f16hi operand rounding (everything else exact)."""
    H = np.asarray(pre).shape[2] // 8
    return _layer(pre, w_hh, d_out, np.float64, Formulas64(), ops or recurrent_operands('f16hi', tagged, H))


def layer32_ragged(pre, w_hh, lengths, fn=TorchF32):
    """layer32 over a ragged batch: row b runs its first lengths[b] frames, out / csave are zero behind."""
    B, T, H8 = pre.shape
    res = dict(out=np.zeros((B, T, H8 // 4), F32), csave=np.zeros((B, T, H8 // 4), F32), act=np.full((B, T, H8), np.nan, F32))
    for b, n in enumerate(lengths):
        r = layer32(pre[b:b + 1, :n], w_hh, None, fn)
        for k in res:
            res[k][b, :n] = r[k][0]
    return res
