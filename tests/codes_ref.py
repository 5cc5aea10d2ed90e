"""Float64 reference of encode-to-codes and decode-from-codes, built from the oracle's own pieces (oracle/ref_model.py: encoder_7,
encoder_t, encoder_6, decoder): a code is what the encoders return (codes_from), decode is repeat_interleave by each code's factor,
concatenate with the speaker rows, ref_model.decoder.  tests/test_codes_ref_selftest.py checks it against ref_model.generator_3 /
generator_6 and shows that the mistakes a decode-from-codes kernel can make are far outside the bar on the inputs the GPU tests use."""
import numpy as np
import torch

from oracle import ref_model, weights as W
from speechsplit_amd._capi import HP_FIELDS

HP = W.default_hparams()
SEED_G3, SEED_G6 = 3, 4            # weight seeds of the suite's eval tests (tests/test_gpu_ragged.py)
SEED_IN = 11                       # input generator seed of the mixing / variant cases
_P64 = {}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def p64(kind, hp=HP, seed=None):
    key = (kind, tuple(int(getattr(hp, n)) for n in HP_FIELDS), seed)
    if key not in _P64:
        w = W.make_weights(kind, hp, seed if seed is not None else (SEED_G3 if kind == 'G3' else SEED_G6))
        _P64[key] = {k: torch.from_numpy(np.array(v, dtype=np.float64)) for k, v in w.items()}
    return _P64[key]


def inputs(seed, B, T, hp=HP):
    """mel [B,T,80] in [0,1), one-hot F0 [B,T,257], one-hot speaker rows [B,82] (the generator of tests/test_gpu_ragged.py)"""
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, hp.dim_freq, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (B, T), generator=g), hp.dim_f0).float()
    emb = torch.nn.functional.one_hot(torch.randint(0, hp.dim_spk_emb, (B,), generator=g), hp.dim_spk_emb).float()
    return mel, onehot, emb


def encode_g3(P, hp, x_f0, x_org):
    """(codes_x, codes_2, codes_f0) of an eval-mode Generator_3 forward (model.py:299-300)"""
    with torch.no_grad():
        cx, cf = ref_model.encoder_7(x_f0.double().transpose(2, 1), P, hp, None, False)
        c2 = ref_model.encoder_t(x_org.double().transpose(2, 1), P, hp)
    return cx, c2, cf


def decode_g3(P, hp, cx, c2, cf, c_trg):
    """model.py:301-312 on given codes"""
    T = c2.shape[1] * hp.freq_2
    with torch.no_grad():
        enc = torch.cat((cx.double().repeat_interleave(hp.freq, 1), c2.double().repeat_interleave(hp.freq_2, 1),
                         cf.double().repeat_interleave(hp.freq_3, 1), c_trg.double()[:, None, :].expand(-1, T, -1)), -1)
        return ref_model.decoder(enc, P, 3)


def encode_g6(P, hp, x_org, f0_trg):
    with torch.no_grad():
        c2 = ref_model.encoder_t(x_org.double().transpose(2, 1), P, hp)
        c3 = ref_model.encoder_6(f0_trg.double().transpose(2, 1), P, hp, None, False)
    return c2, c3


def decode_g6(P, hp, c2, c3):
    with torch.no_grad():
        enc = torch.cat((c2.double().repeat_interleave(hp.freq_2, 1), c3.double().repeat_interleave(hp.freq_3, 1)), -1)
        return ref_model.decoder(enc, P, 2)


def swap_halves(c):
    """forward and backward halves of a code exchanged"""
    H = c.shape[-1] // 2
    return torch.cat((c[..., H:], c[..., :H]), -1)


def wrong_variants(cx, c2, cf, emb):
    """{name: (cx, c2, cf, emb)}: what a decode-from-codes that indexes wrongly would compute.  Another row's code (each code), another row's
    speaker, halves swapped (each code), a code shifted by one block (each code), a zeroed rhythm code."""
    base = {'x': cx, '2': c2, 'f0': cf}
    out = {}

    def put(name, **kw):
        a = dict(base, **kw)
        out[name] = (a['x'], a['2'], a['f0'], kw.get('emb', emb))
    for k, c in base.items():
        put(f'row_{k}', **{k: c.roll(1, 0)})
        put(f'halves_{k}', **{k: swap_halves(c)})
        put(f'shift_{k}', **{k: c.roll(1, 1)})
    put('row_emb', emb=emb.roll(1, 0))
    put('zero_2', **{'2': torch.zeros_like(c2)})
    return out


def check_against(out, ref, bar, tag):
    """print the figure, then assert it"""
    r = rel(out, ref)
    print(f'[{tag}] rel {r:.2e} (bar {bar:.0e})')
    assert r < bar, (tag, r)
    return r
