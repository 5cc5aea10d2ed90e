"""A float64 Adam step, stock fp32 torch.optim.Adam as the yardstick, the ulp comparator and the controlled gradients of the optimiser
tests (test_gpu_optimizer.py; proven on wrong stand-ins by test_adam_ref_selftest.py).  Importing it needs no GPU; every function works on
tensors of any device.

The reference is torch.optim.Adam's single-tensor update without amsgrad and weight decay, evaluated in float64 on the fp32 inputs
promoted exactly (t: the step being applied, the number of updates already applied plus one):

    g  = grad_scale * grad                 m' = beta1 m + (1 - beta1) g            v' = beta2 v + (1 - beta2) g^2
    p' = p - lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)

Errors are fp32 ulps of the float64 value (ulp32(x) = 2^(floor(log2 |x|) - 23), 2^-149 for zero and subnormals), with two floors:
  * the update p - p' is read off a p' that is itself rounded: its unit is at least half an ulp of the larger of |p| and |p'|;
  * a v' below the smallest normal fp32 has that number as its unit, so flushing it to zero and keeping it both pass.
cancel_floor=True (real gradients only: there g is whatever the backward left, and among 2 * 10^7 elements some beta1 m + (1 - beta1) g
cancels to 10^-6 of its terms) adds a third: the unit of m' is at least an ulp of m, the term whose rounding survives the cancellation --
no fp32 Adam can do better, torch's included -- and the unit of the update grows by the same factor.  The controlled gradients below never
cancel by more than the alternating class's fixed factor, and are compared without it.

BARS is 4 x YARDSTICK, and YARDSTICK is what adam_f32_torch showed against adam_f64 over the whole case grid of test_gpu_optimizer.py
(CASES, 9 steps each, 19.4 M elements, on the CPU): the worst error per quantity and gradient class.  The factor covers an equally valid
operation order (lerp form of m, sqrt(bc2) held as a float, step_size * (m / denom)) and a sqrtf / division that is not correctly rounded.
Nothing in BARS comes from the engine.  test_adam_ref_selftest.py re-measures the yardstick at a small size and holds it under YARDSTICK.
"""
import math

import torch

CLASSES = ('ordinary', 'zero', 'near_eps', 'large', 'tiny', 'alternating', 'fading')
NCLS = len(CLASSES)
FLT_MIN = 2.0 ** -126

HP_DEFAULT = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)
HP_FAST = dict(lr=1e-3, beta1=0.5, beta2=0.9, eps=1e-3)
HP_MID = dict(lr=3e-4, beta1=0.9, beta2=0.98, eps=1e-6)

# (hyper-parameters, restored step, grad_scale): every value of the three settings at least once, not their product
CASES = [
    ('default_t0_gs1', HP_DEFAULT, 0, 1.0),
    ('fast_t0_gs05', HP_FAST, 0, 0.5),
    ('mid_t7_gs2m10', HP_MID, 7, 2.0 ** -10),
    ('default_t999_gs05', HP_DEFAULT, 999, 0.5),
    ('fast_t1e6_gs1', HP_FAST, 1000000, 1.0),
    ('mid_t1e6_gs2m10', HP_MID, 1000000, 2.0 ** -10),
    ('default_t7_gs1', HP_DEFAULT, 7, 1.0),
]

# worst error of stock fp32 torch.optim.Adam against float64, per quantity and class, in the units above (see the module docstring)
YARDSTICK = {
    'm':   dict(ordinary=1.54, zero=0.0, near_eps=1.53, large=1.53, tiny=1.54, alternating=9.61, fading=0.625),
    'v':   dict(ordinary=2.27, zero=0.0, near_eps=2.25, large=2.27, tiny=1.2e-7, alternating=2.26, fading=2.26),
    'upd': dict(ordinary=6.28, zero=0.0, near_eps=5.19, large=5.16, tiny=1.72e-6, alternating=6.96, fading=4.84),
}
FACTOR = 4.0
BARS = {q: {c: FACTOR * y for c, y in row.items()} for q, row in YARDSTICK.items()}
# v' of the tiny class is g^2 below the smallest normal fp32, and its unit is that number: the bar is one unit, so that a kernel that
# flushes subnormals to zero and one that keeps them both pass (stock torch keeps them: 1.2e-7), and nothing larger does
BARS['v']['tiny'] = 1.0


# ------------------------------------------------------------------------------------------------ the two Adams
def adam_f64(p, g, m, v, *, lr, beta1, beta2, eps, t, grad_scale=1.0):
    """One Adam step in float64: (p', m', v').  grad_scale is taken as the fp32 number the C ABI receives."""
    p, g, m, v = (x.detach().double() for x in (p, g, m, v))
    g = g * float(torch.tensor(grad_scale, dtype=torch.float32))
    m1 = beta1 * m + (1.0 - beta1) * g
    v1 = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m1 / denom), m1, v1


def adam_f32_torch(p, g, m, v, *, lr, beta1, beta2, eps, t, grad_scale=1.0):
    """The same step by stock torch.optim.Adam(foreach=False, fused=False) on fp32 CPU tensors, its state (step t - 1, exp_avg, exp_avg_sq)
    loaded through load_state_dict: (p', m', v') in fp32."""
    f = lambda x: x.detach().to(device='cpu', dtype=torch.float32).clone()
    par = torch.nn.Parameter(f(p))
    opt = torch.optim.Adam([par], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=0, amsgrad=False, foreach=False, fused=False)
    sd = opt.state_dict()
    sd['state'] = {0: dict(step=torch.tensor(float(t - 1)), exp_avg=f(m), exp_avg_sq=f(v))}
    opt.load_state_dict(sd)
    par.grad = f(g) * torch.tensor(grad_scale, dtype=torch.float32)
    opt.step()
    st = opt.state[par]
    assert float(st['step']) == float(t)
    return par.detach(), st['exp_avg'], st['exp_avg_sq']


# ------------------------------------------------------------------------------------------------ the comparator
def ulp32(x):
    """fp32 unit in the last place at the magnitude of the float64 tensor x: 2^(floor(log2 |x|) - 23), 2^-149 below the smallest normal."""
    _, e = torch.frexp(x.abs())                                    # |x| = mant * 2^e, mant in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e.clamp(min=-125) - 24)


def _per_class(err, cls):
    """Worst error per class as a [NCLS] tensor (cls None: everything is 'ordinary').  One masked maximum per class: a scatter with
    2 * 10^7 elements onto 7 addresses serialises on the atomics."""
    if cls is None:
        out = torch.zeros(NCLS, dtype=torch.float64, device=err.device)
        out[0] = err.max()
        return out
    zero = torch.zeros((), dtype=torch.float64, device=err.device)
    return torch.stack([torch.where(cls == c, err, zero).max() for c in range(NCLS)])


def compare(got, want64, before, cls=None, mask=None, cancel_floor=False):
    """got = (p', m', v') of the step under test, want64 = adam_f64's, before = (p, m, v) the step started from; flat tensors of one length.
    cls: int64 class index per element (default: all 'ordinary'); mask: bool, the elements that are parameters (alignment gaps and the status
    slot are not compared; default: all).  EVERY masked element is compared.  Returns dict(m=, v=, upd= {class: worst error}, worst=(quantity,
    flat index, error, class name)); a NaN or an infinity in `got` counts as an infinite error."""
    pg, mg, vg = (x.detach().double().reshape(-1) for x in got)
    pw, mw, vw = (x.detach().double().reshape(-1) for x in want64)
    p0, m0 = before[0].detach().double().reshape(-1), before[1].detach().double().reshape(-1)
    unit_m = ulp32(mw)
    kappa = 1.0
    if cancel_floor:
        floor_m = torch.maximum(unit_m, ulp32(m0))
        kappa = floor_m / unit_m
        unit_m = floor_m
    unit_v = torch.where(vw < FLT_MIN, torch.full_like(vw, FLT_MIN), ulp32(vw))
    upd_w, upd_g = p0 - pw, p0 - pg
    unit_u = torch.maximum(kappa * ulp32(upd_w), 0.5 * ulp32(torch.maximum(p0.abs(), pw.abs())))
    res, worst = {}, ('', -1, -1.0, '')
    for q, e in (('m', (mg - mw).abs() / unit_m), ('v', (vg - vw).abs() / unit_v), ('upd', (upd_g - upd_w).abs() / unit_u)):
        e = torch.nan_to_num(e, nan=float('inf'), posinf=float('inf'))
        if mask is not None:
            e = torch.where(mask, e, torch.zeros_like(e))
        res[q] = e
    stacked = torch.stack([_per_class(res[q], cls) for q in ('m', 'v', 'upd')]).tolist()
    out = {}
    for k, q in enumerate(('m', 'v', 'upd')):
        out[q] = dict(zip(CLASSES, stacked[k]))
        top = max(stacked[k])
        if top > worst[2]:
            i = int(res[q].argmax())
            worst = (q, i, top, CLASSES[int(cls[i]) if cls is not None else 0])
    out['worst'] = worst
    return out


def excess(rep, bars=None, only=None):
    """[(quantity, class, error, bar)] of a compare() result beyond the bars (default BARS; only: hold every class to that class's bar)."""
    bars = BARS if bars is None else bars
    bad = []
    for q in ('m', 'v', 'upd'):
        for c, e in rep[q].items():
            bar = bars[q][only or c]
            if not e <= bar:
                bad.append((q, c, e, bar))
    return bad


def merge(into, rep):
    """Running worst of several compare() results (into: {} to start with)."""
    for q in ('m', 'v', 'upd'):
        row = into.setdefault(q, dict.fromkeys(CLASSES, 0.0))
        for c, e in rep[q].items():
            row[c] = max(row[c], e)
    if rep['worst'][2] > into.get('worst', ('', -1, -1.0, ''))[2]:
        into['worst'] = rep['worst']
    return into


def table(rep):
    return '\n'.join(f'    {q:4s}' + ''.join(f' {c} {rep[q][c]:.3g}' for c in CLASSES) for q in ('m', 'v', 'upd'))


# ------------------------------------------------------------------------------------------------ controlled inputs
def classes(n, device='cpu'):
    """Class of every flat index: index mod 7.  7 is coprime to the kernels' float4, so every lane meets every class, every tensor (the
    257-float head bias too) holds all of them, and so do the 8 elements either side of any seam."""
    return torch.arange(n, dtype=torch.int64, device=device) % NCLS


def _u(n, salt, device):
    """U[0, 1) on a 2^-24 grid as a float64 tensor: a counter hash of (flat index, salt) in int64 arithmetic, the same bits on every device."""
    M = 0xFFFFFFFF
    x = (torch.arange(n, dtype=torch.int64, device=device) * 2654435761 + (salt * 40503 + 12345)) & M
    x = x ^ (x >> 15)
    x = (x * 2246822519) & M
    x = x ^ (x >> 13)
    x = (x * 3266489917) & M
    x = x ^ (x >> 16)
    return (x >> 8).double() / float(1 << 24)


def _sign(n, device):
    return torch.where(_u(n, 1, device) < 0.5, -1.0, 1.0)


def make_params(n, device='cpu'):
    """p = +-10^U(-3, 0) as fp32: three decades, so the update is compared at its own ulps where p is small and at p's where it is large."""
    return (torch.where(_u(n, 2, device) < 0.5, -1.0, 1.0) * 10.0 ** (-3.0 + 3.0 * _u(n, 3, device))).float()


def make_grad(n, k, eps, device='cpu'):
    """The raw gradient of step k = 1, 2, .. of a case (before grad_scale), fp32, by class (the sign of an element is fixed over the steps
    unless its class says otherwise, so beta1 m + (1 - beta1) g never cancels by chance):
      ordinary     sign * 10^U(-6, 0), the magnitude drawn again every step
      zero         0
      near_eps     sign * eps * 10^U(-1, 1): eps and its placement decide the update
      large        sign * 10^U(15, 18): g^2 close to the fp32 ceiling
      tiny         sign * 10^U(-25, -20): g^2 subnormal or zero in fp32
      alternating  a fixed magnitude 10^U(-4, -1), the sign flipped every step: m crosses zero
      fading       as ordinary on step 1, then 0: the moments decay geometrically"""
    cls, s = classes(n, device), _sign(n, device)
    u = _u(n, 100 + k, device)
    mag = torch.zeros(n, dtype=torch.float64, device=device)
    mag = torch.where(cls == 0, 10.0 ** (-6.0 * u), mag)
    mag = torch.where(cls == 2, eps * 10.0 ** (2.0 * u - 1.0), mag)
    mag = torch.where(cls == 3, 10.0 ** (15.0 + 3.0 * u), mag)
    mag = torch.where(cls == 4, 10.0 ** (-25.0 + 5.0 * u), mag)
    mag = torch.where(cls == 5, (1.0 if k % 2 else -1.0) * 10.0 ** (-4.0 + 3.0 * _u(n, 4, device)), mag)
    if k == 1:
        mag = torch.where(cls == 6, 10.0 ** (-6.0 * u), mag)
    return torch.where(mag == 0, mag, s * mag).float()            # the zeros are +0: what 'bit-identical' is checked against


def make_moments(n, restored, eps, grad_scale=1.0, device='cpu'):
    """(m, v) a case starts from: zeros at step 0; after a restored step random non-zero ones at the scale of the scaled gradient of step 1,
    m = g1 * U(0.2, 0.4) and v = g1^2 * U(0.5, 1.5) >= 0 -- zero where the class is 'zero'."""
    if not restored:
        z = torch.zeros(n, dtype=torch.float32, device=device)
        return z, z.clone()
    g1 = make_grad(n, 1, eps, device).double() * grad_scale
    return (g1 * (0.2 + 0.2 * _u(n, 5, device))).float(), (g1 * g1 * (0.5 + _u(n, 6, device))).float()


def bits_equal(a, b, sel=None):
    a, b = a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32)
    return bool(torch.equal(a[sel], b[sel])) if sel is not None else bool(torch.equal(a, b))
