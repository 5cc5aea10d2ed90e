"""Float64 restatement of the differentiable decode (ss_*_decode_train / ss_*_decode_backward / ss_adam_step_decoder /
ss_g3_decode_train_step), in torch autograd over the oracle's decoder as tests/codes_ref.py uses it: out, every decoder / head gradient,
the code gradients and dc_trg; the decoder-only Adam step on a flat arena; and the wrong variants a kernel or an engine could compute
instead.  tests/test_decode_grad_ref_selftest.py checks the restatement against central finite differences and shows every wrong variant
at least 100 x above the GPU bar on the inputs the GPU tests use.  Importing it needs no GPU.

Inputs of the GPU tests: codes and speaker rows are random normal with standard deviation SCALE = 0.25.  That is the scale of real codes:
ss_g3_encode on the suite's test weights (codes_ref.SEED_G3, inputs(11, 4, 64)) gives standard deviations 0.16 (content), 0.09 (rhythm)
and 0.29 (pitch), Generator_6's encoders 0.39 and 0.27; tests/test_gpu_decode_grad.py prints the figures of the engine's own encode."""
import numpy as np
import torch

from oracle import ref_model
from tests import adam_ref
from tests.codes_ref import p64, rel  # noqa: F401  (re-exported for the tests)

BAR = 1e-4                         # the project's parity bar: relative max-norm per tensor (tests/test_gpu_parity.py)
SCALE = 0.25
WRONG_FACTOR = 100.0               # every wrong variant must show at least this many bars


def factors(kind, hp):
    """(name, factor, width) of the codes in the engine's column order (model.py:301-309 / 341-347)"""
    f = [('r', hp.freq_2, 2 * hp.dim_neck_2), ('f0', hp.freq_3, 2 * hp.dim_neck_3)]
    return ([('x', hp.freq, 2 * hp.dim_neck)] if kind == 'G3' else []) + f


def make_inputs(kind, hp, B, T, seed):
    """codes (engine order), speaker rows (None for Generator_6) and d_out, fp32: N(0, SCALE) codes and rows, N(0, 1) d_out / (B T)"""
    g = torch.Generator().manual_seed(seed)
    codes = [SCALE * torch.randn(B, T // f, w, generator=g) for _, f, w in factors(kind, hp)]
    emb = SCALE * torch.randn(B, hp.dim_spk_emb, generator=g) if kind == 'G3' else None
    head = hp.dim_freq if kind == 'G3' else hp.dim_f0
    d_out = torch.randn(B, T, head, generator=g) / (B * T)
    return codes, emb, d_out


def dec_params(P, grad=True):
    """the decoder + head parameters of a float64 weight dict as fresh leaves"""
    return {k: v.detach().clone().requires_grad_(grad) for k, v in P.items() if k.startswith('decoder.')}


def dec_input(kind, hp, codes, emb):
    T = codes[0].shape[1] * factors(kind, hp)[0][1]
    parts = [c.repeat_interleave(f, 1) for c, (_, f, _) in zip(codes, factors(kind, hp))]
    if kind == 'G3':
        parts.append(emb[:, None, :].expand(-1, T, -1))
    return torch.cat(parts, -1)


def decode_grad(kind, P, hp, codes, emb, d_out=None, target=None):
    """The float64 computation: out = decoder(dec_input(codes, emb)); loss = <out, d_out>, or mean((out - target)^2) when target is given.
    Returns dict(out, loss, grads {decoder.* name: tensor}, d_codes [per code], dc_trg [B, E] or None, d_in [B, T, In])."""
    Pd = dec_params(P)
    codes = [c.detach().double().clone().requires_grad_(True) for c in codes]
    emb = emb.detach().double().clone().requires_grad_(True) if emb is not None else None
    enc = dec_input(kind, hp, codes, emb)
    enc.retain_grad()
    out = ref_model.decoder(enc, Pd, 3 if kind == 'G3' else 2)
    loss = ((out - target.double()) ** 2).mean() if target is not None else (out * d_out.double()).sum()
    loss.backward()
    return dict(out=out.detach(), loss=float(loss.detach()), grads={k: v.grad for k, v in Pd.items()}, d_codes=[c.grad for c in codes],
                dc_trg=emb.grad if emb is not None else None, d_in=enc.grad)


# ------------------------------------------------------------------------------------------------ the code-gradient reduction and its wrong variants
CODE_VARIANTS = ('block_mean', 'first_frame', 'off_by_one', 'factors_swapped')


def reduce_codes(kind, hp, d_in, variant=None):
    """The code gradients from the decoder-input gradient d_in [B, T, In]: the sum over each block's frames (variant None), or what a
    wrong kernel would give.  factors_swapped exchanges the factors of the first two codes and needs them to differ or gives the right
    answer (the caller checks that the configuration can tell)."""
    B, T, _ = d_in.shape
    fs = factors(kind, hp)
    fac = [f for _, f, _ in fs]
    if variant == 'factors_swapped':
        fac[0], fac[1] = fac[1], fac[0]
    out, col = [], 0
    for (_, f0, w), f in zip(fs, fac):
        g = torch.cat((d_in[:, :, col:col + w], torch.zeros_like(d_in[:, :1, col:col + w])), 1)      # frame T: a zero row
        col += w
        # code row blk (T / f0 of them, the shape the caller gets) sums frames blk * f + shift + [0, count); frames at or behind T add zero
        shift = 1 if variant == 'off_by_one' else 0
        count = 1 if variant == 'first_frame' else f
        idx = torch.arange(T // f0)[:, None] * f + shift + torch.arange(count)[None, :]
        r = g[:, idx.clamp(max=T)].sum(2)
        out.append(r / f if variant == 'block_mean' else r)
    return out


def sum_order_budget(d_in_abs_blocksum, f):
    """Rounding budget of a float32 sum of f terms added in order: f - 1 roundings, each of relative size at most u = 2^-24, on partial
    sums bounded by the sum of the |terms| -- ((1 + u)^(f - 1) - 1) times that sum (tests/step_ops_ref.py derives its budgets the same
    way).  f == 1 (and the compact form, a copy): zero, the result is exact."""
    return ((1.0 + 2.0 ** -24) ** (f - 1) - 1.0) * d_in_abs_blocksum


# ------------------------------------------------------------------------------------------------ dc_trg and its wrong variants
def dc_trg_by_direction(P, hp, codes, emb, d_out):
    """dc_trg of Generator_3 split by the decoder layer-0 direction the speaker columns feed: (forward part, reverse part), each [B, E];
    their sum is dc_trg.  Layer 0 is evaluated as two one-direction LSTMs, each on its own copy of the speaker rows."""
    Pd = dec_params(P, grad=False)
    e_f = emb.detach().double().clone().requires_grad_(True)
    e_r = emb.detach().double().clone().requires_grad_(True)
    cs = [c.detach().double() for c in codes]
    x_f, x_r = dec_input('G3', hp, cs, e_f), dec_input('G3', hp, cs, e_r)
    pre = 'decoder.lstm'
    hid = Pd[pre + '.weight_hh_l0'].shape[1]
    h0 = x_f.new_zeros(1, x_f.shape[0], hid)
    w = lambda sfx: [Pd[f'{pre}.{n}_l0{sfx}'] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    o_f, _, _ = torch._VF.lstm(x_f, (h0, h0), w(''), True, 1, 0.0, False, False, True)
    o_r, _, _ = torch._VF.lstm(x_r.flip(1), (h0, h0), w('_reverse'), True, 1, 0.0, False, False, True)
    h = torch.cat((o_f, o_r.flip(1)), -1)
    B = h.shape[0]
    z = h.new_zeros(2, B, hid)
    flat = ref_model._lstm_flat(Pd, pre, 3)
    for l in (1, 2):
        h, _, _ = torch._VF.lstm(h, (z, z), flat[8 * l:8 * l + 8], True, 1, 0.0, False, True, True)
    out = torch.nn.functional.linear(h, Pd['decoder.linear_projection.linear_layer.weight'], Pd['decoder.linear_projection.linear_layer.bias'])
    (out * d_out.double()).sum().backward()
    return out.detach(), e_f.grad, e_r.grad


def dc_batch_summed(dc):
    """what a kernel that sums dc_trg over the batch would put in every row"""
    return dc.sum(0, keepdim=True).expand_as(dc)


# ------------------------------------------------------------------------------------------------ the decoder-only Adam step
def adam_decoder(p, g, m, v, split, *, lr, beta1, beta2, eps, t, grad_scale=1.0, variant=None):
    """ss_adam_step_decoder on flat arenas in float64: adam_ref.adam_f64 with step t on [split, n), everything below split unchanged.
    variant 'whole_arena': the encoder range updated as well (what ss_adam_step does).  Returns (p', m', v') as float64."""
    lo = 0 if variant == 'whole_arena' else split
    p1, m1, v1 = (x.detach().double().clone() for x in (p, m, v))
    a, b, c = adam_ref.adam_f64(p[lo:], g[lo:], m[lo:], v[lo:], lr=lr, beta1=beta1, beta2=beta2, eps=eps, t=t, grad_scale=grad_scale)
    p1[lo:], m1[lo:], v1[lo:] = a, b, c
    return p1, m1, v1


def train_decoder_f64(kind, P, hp, codes, emb, target, steps, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
    """`steps` steps of float64 torch Adam on the decoder + head parameters alone, loss = mean((decode(codes, emb) - target)^2), the
    codes and rows fixed: ([loss per step], {name: parameter after the last step}).  The other parameters never move."""
    Pd = dec_params(P)
    opt = torch.optim.Adam(list(Pd.values()), lr=lr, betas=betas, eps=eps)
    cs = [c.detach().double() for c in codes]
    e = emb.detach().double() if emb is not None else None
    losses = []
    for _ in range(steps):
        out = ref_model.decoder(dec_input(kind, hp, cs, e), Pd, 3 if kind == 'G3' else 2)
        loss = ((out - target.double()) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in Pd.items()}


def flat_like(table, n, tensors, dtype=torch.float64):
    """{name: tensor} -> flat arena of n elements by an Engine.table [(name, offset, shape)]; names not given stay zero"""
    out = torch.zeros(n, dtype=dtype)
    for name, off, shape in table:
        if name in tensors:
            out[off:off + int(np.prod(shape))] = tensors[name].detach().reshape(-1).to(dtype)
    return out
