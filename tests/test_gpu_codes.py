"""Encode to codes and decode from codes on the device (ss_g3_encode / ss_g3_decode / ss_g6_encode / ss_g6_decode and the Python layers above
them).  Runs on the GPU box: pytest -m gpu.

References: the float64 oracle pieces (tests/codes_ref.py: ref_model.encoder_7 / encoder_t / encoder_6 / decoder with W.make_weights),
never a second engine call -- except where the statement under test IS an identity between two engine calls (decode(encode(x)) is
forward(x) bit for bit; codes_r is g3_rhythm's result bit for bit; all-full lengths are the dense call bit for bit).
Bars: relative max-norm 1e-4 in f32 mode (TOL of tests/test_gpu_ragged.py and tests/test_gpu_parity.py), 4e-2 in the 16-bit mode (BF16_OUT of
tests/test_gpu_ragged.py).  tests/test_codes_ref_selftest.py shows that on the 3 x 24 inputs used here every indexing mistake of a
decode-from-codes is at least 1e-2 away, and a padded row 0.37 away from the row run alone."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import codes_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-4
BF16_OUT = 4e-2
DEV = 'cuda:0'
HP = R.HP
NAN = float('nan')
MIXED17 = [16 if b % 2 == 0 else 8 for b in range(16)] + [8]        # tests/test_gpu_ragged.py: two batch tiles, lengths differing inside and across
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FACTORS = {'x': 'freq', 'r': 'freq_2', 'f0': 'freq_3'}

_ENG = {}


def engine(kind, precision='f32', hp=HP, tag='default'):
    """one engine per (kind, precision, hyper-parameters), 17 x 192: the long shape grows its workspace (Engine.reserve)"""
    key = (kind, precision, tag)
    if key not in _ENG:
        from speechsplit_amd.engine import Engine
        e = Engine(kind, hp, 17, 192)
        e.set_precision(precision)
        e.load_weights(W.make_weights(kind, hp, R.SEED_G3 if kind == 'G3' else R.SEED_G6))
        _ENG[key] = e
    return _ENG[key]


def g3_inputs(seed, B, T, hp=HP):
    """x_f0 [B,T,337], x_org [B,T,80] (an utterance of its own: the rhythm code must not follow the content input), emb [B,82]"""
    mel, onehot, emb = R.inputs(seed, B, T, hp)
    return torch.cat((mel, onehot), -1), R.inputs(seed + 1, B, T, hp)[0], emb


def padded(x, lens, value, step=1):
    """copy of x [B, T, C] with rows t >= lens[b] / step of row b set to `value`"""
    y = x.clone()
    for b, n in enumerate(lens):
        y[b, n // step:] = value
    return y


def dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# --------------------------------------------------------------------------------------------- 1. codes against the oracle
@pytest.mark.parametrize('B,T', [(3, 24), (17, 16)], ids=['3x24', '17x16_two_tiles'])
def test_g3_codes_against_the_oracle(B, T):
    eng = engine('G3')
    x_f0, x_org, _ = g3_inputs(R.SEED_IN, B, T)
    ref = R.encode_g3(R.p64('G3'), HP, x_f0, x_org)
    xd, od = dev(x_f0, x_org)
    got = eng.g3_encode(xd, od)
    for name, g, r in zip(('x', 'r', 'f0'), got, ref):
        assert tuple(g.shape) == tuple(r.shape) == eng.code_shapes(B, T)[name]
        R.check_against(g, r, TOL, f'g3 codes_{name} {B}x{T}')
    assert bits(got[1], eng.g3_rhythm(od))                                   # the rhythm code is G.rhythm's, bit for bit
    # a NULL output pointer: that code is not computed for the caller, the others are the same bits
    cx, cr, cf = eng.g3_encode(xd, od, want=('x', 'f0'))
    assert cr is None and bits(cx, got[0]) and bits(cf, got[2])
    cx, cr, cf = eng.g3_encode(xd, od, want=('r',))
    assert cx is None and cf is None and bits(cr, got[1])


def test_g6_codes_against_the_oracle():
    B, T = 3, 24
    eng = engine('G6')
    mel, onehot, _ = R.inputs(R.SEED_IN, B, T)
    ref = R.encode_g6(R.p64('G6'), HP, mel, onehot)
    md, hd = dev(mel, onehot)
    got = eng.g6_encode(md, hd)
    for name, g, r in zip(('r', 'f0'), got, ref):
        assert tuple(g.shape) == tuple(r.shape)
        R.check_against(g, r, TOL, f'g6 codes_{name}')
    cr, cf = eng.g6_encode(md, hd, want=('f0',))
    assert cr is None and bits(cf, got[1])
    R.check_against(eng.g6_decode(*got), R.decode_g6(R.p64('G6'), HP, *ref), TOL, 'g6 decode')


# --------------------------------------------------------------------------------------------- 2. round trip
def _round_trip(eng, kind, B, T, hp, lengths, tag):
    x_f0, x_org, emb = g3_inputs(R.SEED_IN, B, T, hp)
    if kind == 'G3':
        args = dev(x_f0, x_org, emb)
        fwd = lambda: eng.g3_forward(*args, lengths=lengths)
        trip = lambda: eng.g3_decode(*eng.g3_encode(args[0], args[1], lengths=lengths), args[2], lengths=lengths)
    else:
        args = dev(x_org, x_f0[..., hp.dim_freq:])
        fwd = lambda: eng.g6_forward(*args, lengths=lengths)
        trip = lambda: eng.g6_decode(*eng.g6_encode(*args, lengths=lengths), lengths=lengths)
    a, b = fwd(), fwd()
    assert bits(a, b), (tag, 'the eval forward itself is not bit-stable')            # tests/test_gpu_same_shape_history.py establishes this
    c = trip()
    assert bool(torch.isfinite(c).all()), tag
    assert bits(c, a), (tag, 'decode(encode(x)) differs from forward(x)', R.rel(c, a))
    assert bits(fwd(), a), (tag, 'a forward after the code calls differs')
    return a


@pytest.mark.parametrize('lengths', [None, [24, 8, 16]], ids=['dense', 'ragged'])
@pytest.mark.parametrize('compact0', [1, 0])
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_round_trip_is_the_forward_bit_for_bit(kind, precision, compact0, lengths):
    from speechsplit_amd.engine import tune
    tune('compact0', compact0)
    try:
        _round_trip(engine(kind, precision), kind, 3, 24, HP, lengths, (kind, precision, compact0, lengths))
    finally:
        tune('compact0', 1)


UNEQUAL = dict(freq=4, freq_2=8, freq_3=2)                               # the full-slab form of the decoder input runs
ODD = dict(dim_neck=1, dim_neck_2=32, dim_neck_3=5, dim_spk_emb=81)      # 2H = 2 (scalar path), 10 (no float4), an odd row length


@pytest.mark.parametrize('over,T,lengths', [(UNEQUAL, 16, None), (UNEQUAL, 16, [16, 8, 8]), (ODD, 24, None), (ODD, 24, [24, 8, 16])],
                         ids=['unequal_factors', 'unequal_factors_ragged', 'odd_widths', 'odd_widths_ragged'])
def test_round_trip_at_other_hyper_parameters(over, T, lengths):
    hp = W.default_hparams(**over)
    tag = 'unequal' if over is UNEQUAL else 'odd'
    eng = engine('G3', 'f32', hp, tag)
    out = _round_trip(eng, 'G3', 3, T, hp, lengths, (tag, lengths))
    # and the round trip is the right answer: the oracle at these hyper-parameters
    x_f0, x_org, emb = g3_inputs(R.SEED_IN, 3, T, hp)
    P = R.p64('G3', hp)
    for b, n in enumerate(lengths or [T] * 3):
        ref = R.decode_g3(P, hp, *R.encode_g3(P, hp, x_f0[b:b + 1, :n], x_org[b:b + 1, :n]), emb[b:b + 1])
        R.check_against(out[b:b + 1, :n], ref, TOL, f'{tag} row {b}')


# --------------------------------------------------------------------------------------------- 3. mixing
@pytest.mark.parametrize('precision,bar', [('f32', TOL), ('bf16', BF16_OUT)])
def test_mixed_codes_against_the_float64_reference(precision, bar):
    """row b: content of b, rhythm of perm(b), pitch of perm2(b), speaker of perm3(b)"""
    B, T = 3, 24
    eng = engine('G3', precision)
    x_f0, x_org, emb = g3_inputs(R.SEED_IN, B, T)
    p1, p2, p3 = [1, 2, 0], [2, 0, 1], [0, 2, 1]
    rx, r2, rf = R.encode_g3(R.p64('G3'), HP, x_f0, x_org)
    ref = R.decode_g3(R.p64('G3'), HP, rx, r2[p1], rf[p2], emb[p3])
    plain = R.decode_g3(R.p64('G3'), HP, rx, r2, rf, emb)
    assert R.rel(plain, ref) > 1e-2                                          # the mix is not the unmixed forward by a wide margin
    cx, cr, cf = eng.g3_encode(*dev(x_f0, x_org))
    out = eng.g3_decode(cx, cr[p1].contiguous(), cf[p2].contiguous(), emb[p3].to(DEV))
    R.check_against(out, ref, bar, f'mixed decode {precision}')
    if precision == 'f32':      # decode alone, on the oracle's codes: nothing of the engine's encoders in the result
        R.check_against(eng.g3_decode(*dev(rx.float(), r2[p1].float(), rf[p2].float(), emb[p3])), ref, TOL, 'mixed decode of oracle codes')


# --------------------------------------------------------------------------------------------- 4. ragged
def _check_code_rows(codes, lens, refs, hp, tag):
    """every row of every code: exact zeros at and behind lens[b] / factor, its own rows within TOL of the oracle's run of that row alone"""
    worst = 0.0
    for name, c in codes.items():
        f = getattr(hp, FACTORS[name])
        c = c.detach().cpu()
        for b, n in enumerate(lens):
            assert bool((c[b, n // f:] == 0).all()), (tag, name, b, 'code rows behind the end are not zero')
            assert bool(torch.isfinite(c[b, :n // f]).all()), (tag, name, b)
            worst = max(worst, R.rel(c[b, :n // f], refs[b][name][0]))
    print(f'[{tag}] worst code row rel {worst:.2e}')
    assert worst < TOL, (tag, worst)


@pytest.mark.parametrize('B,T,lens', [(3, 24, [24, 8, 16]), (17, 16, MIXED17)], ids=['3x24', '17x16_mixed'])
def test_g3_ragged_encode_and_decode(B, T, lens):
    eng = engine('G3')
    P = R.p64('G3')
    x_f0, x_org, emb = g3_inputs(R.SEED_IN + 5, B, T)
    refs, outs = [], []
    for b, n in enumerate(lens):                                            # the oracle on every row ALONE at its own length
        cx, c2, cf = R.encode_g3(P, HP, x_f0[b:b + 1, :n], x_org[b:b + 1, :n])
        refs.append({'x': cx, 'r': c2, 'f0': cf})
        outs.append(R.decode_g3(P, HP, cx, c2, cf, emb[b:b + 1])[0])
    xd, od, ed = dev(padded(x_f0, lens, NAN), padded(x_org, lens, NAN), emb)
    cx, cr, cf = eng.g3_encode(xd, od, lengths=lens)
    _check_code_rows({'x': cx, 'r': cr, 'f0': cf}, lens, refs, HP, f'ragged encode {B}x{T}')
    # decode never reads the code rows behind a row's end: NaN there
    nx, nr, nf = (padded(c, lens, NAN, getattr(HP, FACTORS[k])) for k, c in (('x', cx), ('r', cr), ('f0', cf)))
    out = eng.g3_decode(nx, nr, nf, ed, lengths=lens).cpu()
    worst = 0.0
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == 0).all()), (b, 'output frames behind the end are not zero')
        assert bool(torch.isfinite(out[b, :n]).all()), b
        worst = max(worst, R.rel(out[b, :n], outs[b]))
    print(f'[ragged decode {B}x{T}] worst row rel {worst:.2e}')
    assert worst < TOL
    # all-full lengths: the dense call, bit for bit (on inputs without NaN)
    xd, od = dev(x_f0, x_org)
    full = [T] * B
    dense, rag = eng.g3_encode(xd, od), eng.g3_encode(xd, od, lengths=full)
    assert all(bits(a, b) for a, b in zip(dense, rag))
    assert bits(eng.g3_decode(*dense, ed), eng.g3_decode(*dense, ed, lengths=full))


def test_g6_ragged_encode_and_decode():
    B, T, lens = 3, 24, [24, 8, 16]
    eng = engine('G6')
    P = R.p64('G6')
    mel, onehot, _ = R.inputs(R.SEED_IN + 6, B, T)
    refs, outs = [], []
    for b, n in enumerate(lens):
        c2, c3 = R.encode_g6(P, HP, mel[b:b + 1, :n], onehot[b:b + 1, :n])
        refs.append({'r': c2, 'f0': c3})
        outs.append(R.decode_g6(P, HP, c2, c3)[0])
    cr, cf = eng.g6_encode(*dev(padded(mel, lens, NAN), padded(onehot, lens, NAN)), lengths=lens)
    _check_code_rows({'r': cr, 'f0': cf}, lens, refs, HP, 'g6 ragged encode')
    out = eng.g6_decode(padded(cr, lens, NAN, HP.freq_2), padded(cf, lens, NAN, HP.freq_3), lengths=lens).cpu()
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == 0).all()), b
        R.check_against(out[b, :n], outs[b], TOL, f'g6 ragged decode row {b}')
    md, hd = dev(mel, onehot)
    dense, rag = eng.g6_encode(md, hd), eng.g6_encode(md, hd, lengths=[T] * B)
    assert all(bits(a, b) for a, b in zip(dense, rag))
    assert bits(eng.g6_decode(*dense), eng.g6_decode(*dense, lengths=[T] * B))


# --------------------------------------------------------------------------------------------- 5. long
def test_long_utterance_above_max_frames():
    """1 x 264: above max_frames (192) -- the chunked GroupNorm kernels and a workspace grown through Engine.reserve"""
    B, T = 1, 264
    eng = engine('G3')
    x_f0, x_org, emb = g3_inputs(R.SEED_IN + 7, B, T)
    P = R.p64('G3')
    ref_codes = R.encode_g3(P, HP, x_f0, x_org)
    codes = eng.g3_encode(*dev(x_f0, x_org))
    for name, g, r in zip(('x', 'r', 'f0'), codes, ref_codes):
        R.check_against(g, r, TOL, f'long codes_{name}')
    R.check_against(eng.g3_decode(*codes, emb.to(DEV)), R.decode_g3(P, HP, *ref_codes, emb), TOL, 'long decode')


# --------------------------------------------------------------------------------------------- 6. launch classes, state, refusals
ENCODE_NEVER = {'rec_fwd', 'dec_proj', 'dec_proj0', 'head'}
DECODE_NEVER = {'conv_fwd', 'gn', 'enc_rec'}


def _classes(eng, call):
    eng.profile('timeline')
    try:
        res = call()
        torch.cuda.synchronize()
        names = [t[0] for t in eng.profile_timeline()]
    finally:
        eng.profile(False)
    return res, {n: names.count(n) for n in set(names)}


@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_launch_classes_and_state_afterwards(kind):
    B, T = 3, 24
    eng = engine(kind)
    x_f0, x_org, emb = g3_inputs(R.SEED_IN, B, T)
    if kind == 'G3':
        xd, od, ed = dev(x_f0, x_org, emb)
        fwd, enc, bwd = (lambda: eng.g3_forward(xd, od, ed)), (lambda: eng.g3_encode(xd, od)), eng.g3_backward
        dec = lambda c: eng.g3_decode(*c, ed)
        d_out = torch.zeros(B, T, HP.dim_freq, device=DEV)
    else:
        od, hd = dev(x_org, x_f0[..., HP.dim_freq:])
        fwd, enc, bwd = (lambda: eng.g6_forward(od, hd)), (lambda: eng.g6_encode(od, hd)), eng.g6_backward
        dec = lambda c: eng.g6_decode(*c)
        d_out = torch.zeros(B, T, HP.dim_f0, device=DEV)
    before, all_classes = _classes(eng, fwd)
    assert (ENCODE_NEVER | DECODE_NEVER) <= set(all_classes), all_classes      # the forward launches every one of them: the sets below mean something
    codes, counts = _classes(eng, enc)
    print(f'[{kind} encode launches] {counts}')
    assert not ENCODE_NEVER & set(counts), counts
    assert {k: counts.get(k) for k in DECODE_NEVER} == {k: all_classes[k] for k in DECODE_NEVER}      # and all of the forward's encoder launches
    with pytest.raises(RuntimeError, match='without a preceding forward'):
        bwd(d_out)
    out, counts = _classes(eng, lambda: dec(codes))
    print(f'[{kind} decode launches] {counts}')
    assert not DECODE_NEVER & set(counts), counts
    assert {k: counts.get(k) for k in ENCODE_NEVER} == {k: all_classes[k] for k in ENCODE_NEVER}
    with pytest.raises(RuntimeError, match='without a preceding forward'):
        bwd(d_out)
    assert bits(out, before)
    assert bits(fwd(), before)                                               # the engine stays usable: a normal forward, the same bits
    bwd(d_out)                                                               # ... and that one can be differentiated
    eng.check()


def test_refusals_on_a_bound_engine_enqueue_nothing_and_name_the_call():
    eng = engine('G3')
    e6 = engine('G6')
    lib, h = eng.lib, eng.h
    B, T = 2, 16
    buf = torch.full((B * T * 512,), NAN, device=DEV)
    p, z = C.c_void_p(buf.data_ptr()), C.c_void_p(0)
    torch.cuda.synchronize()

    def refused(rc, name, word):
        msg = lib.ss_last_error().decode()
        assert rc != 0 and name in msg and word in msg, (name, word, msg)

    # NULL required pointers
    refused(lib.ss_g3_encode(h, z, p, z, B, T, p, p, p, z), 'ss_g3_encode', 'null pointer')
    refused(lib.ss_g3_encode(h, p, z, z, B, T, p, p, p, z), 'ss_g3_encode', 'null pointer')
    refused(lib.ss_g3_encode(h, p, p, z, B, T, z, z, z, z), 'ss_g3_encode', 'null pointer')          # all outputs NULL
    for k in range(4):
        a = [p, p, p, p]
        a[k] = z
        refused(lib.ss_g3_decode(h, *a, z, B, T, p, z), 'ss_g3_decode', 'null pointer')
    refused(lib.ss_g3_decode(h, p, p, p, p, z, B, T, z, z), 'ss_g3_decode', 'null pointer')
    refused(lib.ss_g6_encode(e6.h, p, p, z, B, T, z, z, z), 'ss_g6_encode', 'null pointer')
    refused(lib.ss_g6_decode(e6.h, p, z, z, B, T, p, z), 'ss_g6_decode', 'null pointer')
    # B and T outside the rules
    for b, t, word in ((0, T, 'batch'), (18, T, 'batch'), (B, 0, 'T outside'), (B, 8200, 'T outside'), (B, 12, 'multiple'),
                       (17, 8192, 'workspace too small')):
        refused(lib.ss_g3_encode(h, p, p, z, b, t, p, p, p, z), 'ss_g3_encode', word)
        refused(lib.ss_g3_decode(h, p, p, p, p, z, b, t, p, z), 'ss_g3_decode', word)
        refused(lib.ss_g6_encode(e6.h, p, p, z, b, t, p, p, z), 'ss_g6_encode', word)
        refused(lib.ss_g6_decode(e6.h, p, p, z, b, t, p, z), 'ss_g6_decode', word)
    # the wrong kind of engine
    refused(lib.ss_g3_encode(e6.h, p, p, z, B, T, p, p, p, z), 'ss_g3_encode', 'Generator_3')
    refused(lib.ss_g6_decode(h, p, p, z, B, T, p, z), 'ss_g6_decode', 'Generator_6')
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                                      # nothing was enqueued: the output buffer is untouched
    eng.check()
    e6.check()


# --------------------------------------------------------------------------------------------- 7. containment
@pytest.mark.parametrize('lengths', [None, [24, 8, 16]], ids=['dense', 'ragged'])
def test_guarded_encode_and_decode(lengths):
    """Both calls on an engine whose every buffer is a guarded allocation (tests/test_gpu_engine_containment.py): inputs surrounded by NaN,
    outputs banded -- nothing outside the tensors is read into a result or written."""
    from speechsplit_amd import engine as E
    from tests.test_gpu_engine_containment import Bound
    B, T = 3, 24
    b = Bound(E, 'G3', HP, B, T)
    x_f0, x_org, emb = g3_inputs(R.SEED_IN, B, T)
    lens = lengths or [T] * B
    codes = b.eng.g3_encode(b.inp(padded(x_f0, lens, NAN), 'x_f0'), b.inp(padded(x_org, lens, NAN), 'x_org'), lengths=lengths)
    torch.cuda.synchronize()
    keep = [c.clone() for c in codes]
    b.check(('encode', lengths))
    ins = [b.inp(padded(c, lens, NAN, getattr(HP, FACTORS[k])), 'codes_' + k) for k, c in zip(('x', 'r', 'f0'), keep)]
    out = b.eng.g3_decode(*ins, b.inp(emb, 'c_trg'), lengths=lengths)
    torch.cuda.synchronize()
    got = out.clone()
    b.check(('decode', lengths))
    P = R.p64('G3')
    for r, n in enumerate(lens):
        ref = R.decode_g3(P, HP, *R.encode_g3(P, HP, x_f0[r:r + 1, :n], x_org[r:r + 1, :n]), emb[r:r + 1])
        R.check_against(got[r:r + 1, :n], ref, TOL, f'guarded row {r}')


def test_guarded_g6_encode_and_decode():
    from speechsplit_amd import engine as E
    from tests.test_gpu_engine_containment import Bound
    B, T = 3, 24
    b = Bound(E, 'G6', HP, B, T)
    mel, onehot, _ = R.inputs(R.SEED_IN, B, T)
    codes = b.eng.g6_encode(b.inp(mel, 'x_org'), b.inp(onehot, 'f0_trg'))
    torch.cuda.synchronize()
    keep = [c.clone() for c in codes]
    b.check('g6 encode')
    out = b.eng.g6_decode(b.inp(keep[0], 'codes_r'), b.inp(keep[1], 'codes_f0'))
    torch.cuda.synchronize()
    got = out.clone()
    b.check('g6 decode')
    P = R.p64('G6')
    R.check_against(got, R.decode_g6(P, HP, *R.encode_g6(P, HP, mel, onehot)), TOL, 'guarded g6')


# --------------------------------------------------------------------------------------------- 8. conversion
def _demo_modules():
    from speechsplit_amd import model
    z = np.load(os.path.join(GOLD, 'demo_config1.npz'))
    hp = W.default_hparams()
    G, P = model.Generator_3(hp).eval(), model.Generator_6(hp).eval()
    G.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_weights('G3', hp, int(z['seed_g3'])).items()}, strict=False)
    P.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_weights('G6', hp, int(z['seed_g6'])).items()}, strict=False)
    ent = []
    for n in range(2):
        L = int(z[f'u{n}_len'])
        ent.append([f'p{n}', z[f'u{n}_emb'], (z[f'u{n}_mel_pad'][0, :L], z[f'u{n}_f0_pad'][:L], L, f'utt{n}')])
    return G.to(DEV), P.to(DEV), ent


def test_demo_conversion_codes_seven_conditions():
    """setup as tests/test_gpu_parity.py::test_demo_conversion_seven_conditions; the reference's seven batch-1 outputs"""
    from speechsplit_amd import convert
    c = np.load(os.path.join(GOLD, 'demo_conversion.npz'))
    G, P, ent = _demo_modules()
    res = convert.demo_conversion_codes(G, P, ent[0], ent[1])
    assert [r[0] for r in res] == [f'p0_p1_utt0_{cond}' for cond in convert.CONDITIONS]
    for (name, mel), cond in zip(res, convert.CONDITIONS):
        assert mel.shape == c[f'out_{cond}'].shape
        R.check_against(mel, c[f'out_{cond}'], TOL, f'demo_conversion_codes {cond}')


def test_convert_speakers_against_batch_one_forwards():
    from speechsplit_amd import convert
    G, _, ent = _demo_modules()
    hp = W.default_hparams()
    g = torch.Generator().manual_seed(17)
    embs = torch.nn.functional.one_hot(torch.randperm(hp.dim_spk_emb, generator=g)[:5], hp.dim_spk_emb).float()
    out = convert.convert_speakers(G, ent[0], embs)
    L = ent[0][2][2]
    assert tuple(out.shape) == (5, L, hp.dim_freq)
    x_org, oh_org, _, _, _ = convert._prepare(ent[0], convert.conversion_frames((L,)), DEV)
    x_f0 = torch.cat((x_org, oh_org), -1)
    with torch.no_grad():
        for n in range(5):
            ref = G(x_f0, x_org, embs[n:n + 1].to(DEV))[0, :L]
            R.check_against(out[n], ref, TOL, f'convert_speakers row {n}')
    assert R.rel(out[0], out[1]) > 1e-2                                      # the speakers differ: the rows are not one result five times
