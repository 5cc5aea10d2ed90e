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


def _layer(pre, w_hh, d_out, dt, fn):
    """Forward (and with d_out the BPTT, in the kernels' operation order) of both directions in precision dt with the formulas fn."""
    pre = np.asarray(pre, dt)
    B, T, H = pre.shape[0], pre.shape[1], pre.shape[2] // 8
    act, out, csave = np.zeros((B, T, 8 * H), dt), np.zeros((B, T, 2 * H), dt), np.zeros((B, T, 2 * H), dt)
    one = dt(1)
    with np.errstate(all='ignore'):
        for d in range(2):
            w = np.asarray(w_hh[d], dt)
            rec = bool(w.any())
            h, c = np.zeros((B, H), dt), np.zeros((B, H), dt)
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                p = pre[:, t, d * 4 * H:(d + 1) * 4 * H]
                if rec:
                    p = p + h @ w.T
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
        res['dgates'] = backward(act, csave, out, d_out, w_hh, dt, fn)
        res['dw_hh'] = dw_hh(res['dgates'], out)
    return res


def backward(act, csave, out, d_out, w_hh, dt, fn):
    """BPTT on a saved forward state in precision dt, in the kernels' operation order (csrc/lstm_small.hip): dgates [B, T, 8H]."""
    act, csave, out, d_out = (np.asarray(x, dt) for x in (act, csave, out, d_out))
    B, T, H = csave.shape[0], csave.shape[1], csave.shape[2] // 2
    dg = np.zeros((B, T, 8 * H), dt)
    one = dt(1)
    with np.errstate(all='ignore'):
        for d in range(2):
            w = np.asarray(w_hh[d], dt)
            rec = bool(w.any())
            gi, gf, gg, go = _parts(act, H, d)
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
                    dh_rec = da @ w
    return dg


def layer32(pre, w_hh, d_out=None, fn=TorchF32):
    """The recurrence restated in fp32 on the CPU with the formulas fn (TorchF32, HeaderF32 or a wrong variant of the self-test)."""
    return _layer(pre, w_hh, d_out, F32, fn())


def layer32_ragged(pre, w_hh, lengths, fn=TorchF32):
    """layer32 over a ragged batch: row b runs its first lengths[b] frames, out / csave are zero behind."""
    B, T, H8 = pre.shape
    res = dict(out=np.zeros((B, T, H8 // 4), F32), csave=np.zeros((B, T, H8 // 4), F32), act=np.full((B, T, H8), np.nan, F32))
    for b, n in enumerate(lengths):
        r = layer32(pre[b:b + 1, :n], w_hh, None, fn)
        for k in res:
            res[k][b, :n] = r[k][0]
    return res
