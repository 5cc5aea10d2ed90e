"""The persistent recurrences (csrc/lstm_seq.hip) launched the way the engine launches them (pytest -m gpu): engine.seq_recurrence passes
every option of SeqFwd / SeqBwd through ss_op_lstm_seq_fwd / _bwd, and each side output and arithmetic variant is compared with a reference
computed from the run's OWN out / dgates (lstm_ref.py: block_sums, bias_sums, bf16_bits, amax_bits, F4 / B3 with the f16hi operand rounding,
check_b2_hi) -- bit for bit wherever the kernel's arithmetic is fixed.  Shapes: the smallest that select each path, (H, B, T) = (256, 5, 40)
a partial batch tile, (256, 17, 40) a second tile, (512, 16, 24); H = 256 under the tagged hand-off and the flag line.  Inputs are
lstm_ref.trained(B, T, H, ws).  Every test prints what it measured before it asserts (ratios: a pass is <= 1).

Every per-utterance side output (out_img, dimg, dgs) comes back with room for the 16 ceil(B / 16) - B padded utterances of the last batch
tile behind it, pre-filled like the guard: a storing wave that lost its b < B test would write there, and `untouched` says that nobody did.

The bias sums meet through one fp32 atomic add per batch tile and element.  With one tile (B = 5, B = 16) the result does not depend on any
order and is compared bit for bit -- between the b_ih and b_hh halves and between runs; with two tiles (B = 17) fl(fl(g0 + S0) + S1) and
fl(fl(g0 + S1) + S0) may differ in the last bit and the arrival order is not fixed, so there every half of every run is held to check_gbias's bar."""
import functools

import numpy as np
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [('h256_b5_tagged', 256, 5, 40, dict(seq_tag=1)), ('h256_b5_flag_line', 256, 5, 40, dict(seq_tag=0)),
          ('h256_b17_tagged', 256, 17, 40, dict(seq_tag=1)), ('h256_b17_flag_line', 256, 17, 40, dict(seq_tag=0)),
          ('h512_b16', 512, 16, 24, {})]
BY_ID = {s[0]: s for s in SHAPES}
IDS = list(BY_ID)
shapes = pytest.mark.parametrize('sid', IDS)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def seq(sid, pre, w, d=None, **opt):
    """engine.seq_recurrence under the shape's knobs, everything as numpy (side outputs: raw uint8, guard included)."""
    from speechsplit_amd import engine as E
    knobs = BY_ID[sid][4]
    for k, v in knobs.items():
        E.tune(k, v)
    try:
        res = E.seq_recurrence(dev(pre), tuple(dev(x) for x in w), None if d is None else dev(d), **opt)
        torch.cuda.synchronize()
    finally:
        for k in knobs:
            E.tune(k, 1)
    return {k: None if v is None else v.cpu().numpy() for k, v in res.items()}


@functools.lru_cache(None)
def inputs(sid, ws=3, expand=0):
    """trained(B, T, H, ws); expand = xf: the pre-activations repeat in blocks of xf frames (what a compact run computes on)."""
    _, H, B, T, _ = BY_ID[sid]
    pre, w, d = R.trained(B, T, H, ws)
    if expand:
        pre = np.repeat(pre[:, ::expand], expand, axis=1)
    return pre, w, d


@functools.lru_cache(None)
def plain(sid, ws=3, hi_only=False, expand=0, backward=True):
    """The run without any option (but hi_only), shared by the tests that compare with it; never modified."""
    pre, w, d = inputs(sid, ws, expand)
    return seq(sid, pre, w, d if backward else None, hi_only=hi_only)


@functools.lru_cache(None)
def refs(H, B, T, ws):
    """(layer64, layer16 untagged) of trained(B, T, H, ws), computed once per shape."""
    pre, w, d = R.trained(B, T, H, ws)
    return R.layer64(pre, w, d), R.layer16(pre, w, d, False)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def body(raw, nbytes, pad_bytes=0):
    """(the first nbytes of a raw side output, True if everything behind them -- pad_bytes of room for the padded utterances, then the guard
    -- still holds the fill byte)."""
    from speechsplit_amd import engine as E
    assert raw.dtype == np.uint8 and raw.size == nbytes + pad_bytes + E.SEQ_GUARD
    return raw[:nbytes], bool((raw[nbytes:] == E.SEQ_FILL).all())


def padded(B):
    """Utterances between B and the end of its last batch tile."""
    return (B + 15) // 16 * 16 - B


def image_rows(raw, B, T, row_bytes):
    """A haloed image [B, T + 4, row_bytes] -> (real rows [B, T, row_bytes], halo rows, the padded utterances' rows and guard untouched)."""
    from speechsplit_amd import engine as E
    img, guard = body(raw, B * (T + 4) * row_bytes, padded(B) * (T + 4) * row_bytes)
    img = img.reshape(B, T + 4, row_bytes)
    return img[:, 2:2 + T], guard and bool((img[:, :2] == E.SEQ_FILL).all() and (img[:, T + 2:] == E.SEQ_FILL).all())


def split_bytes(out):
    """ss_op_split_image(out, scale 16) of the real rows [B, T, 2H], as bytes [B, T, 8H]."""
    from speechsplit_amd import engine as E
    B, T, C = out.shape
    img = E.split_image(dev(out.reshape(B * T, C)), 16.0)
    torch.cuda.synchronize()
    return img.cpu().numpy().view(np.uint8).reshape(B, T, 4 * C)


def u16(x):
    return np.ascontiguousarray(x).view(np.uint16)


def forward_identical(a, b):
    return {k: bool(np.array_equal(bits(a[k]), bits(b[k]))) for k in ('out', 'csave', 'act')}


# ------------------------------------------------------------------------------------------------ forward options
@pytest.mark.parametrize('hi_only', [False, True], ids=['f16x2', 'hi_only'])
@pytest.mark.parametrize('xf', [1, 8, 0], ids=['xf1', 'xf8', 'xfT'])
@shapes
def test_compact_input(sid, xf, hi_only):
    """xc = pre[:, ::xf] with the gates slab full of NaN against the plain run on repeat(xc, xf): out, csave and act bit for bit."""
    _, H, B, T, _ = BY_ID[sid]
    xf = xf or T
    pre, w, _ = inputs(sid, 3, xf)
    ref = plain(sid, 3, hi_only, xf, False) if xf == 8 else seq(sid, pre, w, hi_only=hi_only)
    got = seq(sid, pre[:, ::xf], w, xf=xf, hi_only=hi_only)
    same = forward_identical(got, ref)
    print(f'seq_options {sid} compact xf {xf} hi_only {hi_only}: identical {same} finite {bool(np.isfinite(got["act"]).all())}')
    assert got['act'].shape == (B, T, 8 * H) and np.isfinite(got['act']).all()          # every real row of the NaN slab was written
    assert all(same.values()), same


@shapes
def test_out_img_v2(sid):
    """The real rows of the v2 image are ss_op_split_image(out, 16) byte for byte; halo rows, the rows of padded utterances and the
    guard keep their fill.  Then ragged:
    rows behind each length are zero bytes."""
    _, H, B, T, _ = BY_ID[sid]
    pre, w, _ = inputs(sid)
    got = seq(sid, pre, w, out_img='v2')
    rows, untouched = image_rows(got['out_img'], B, T, 8 * H)
    eq = np.array_equal(rows, split_bytes(got['out']))
    lens = [(T, T // 2, 1)[b % 3] for b in range(B)]
    rag = seq(sid, pre, w, out_img='v2', lengths=lens)
    rrows, runtouched = image_rows(rag['out_img'], B, T, 8 * H)
    tail_zero = all(not rrows[b, n:].any() for b, n in enumerate(lens))
    req = np.array_equal(rrows, split_bytes(rag['out']))
    print(f'seq_options {sid} out_img v2: equal {eq} untouched {untouched} same forward {forward_identical(got, plain(sid))} | ragged: equal {req} '
          f'tail zero {tail_zero} untouched {runtouched}')
    assert eq and untouched and all(forward_identical(got, plain(sid)).values())
    assert req and tail_zero and runtouched and R.tail_is_zero(rag['out'], lens)
    assert all(rrows[b, :n].any() for b, n in enumerate(lens))


@shapes
def test_out_img_bf16(sid):
    _, H, B, T, _ = BY_ID[sid]
    pre, w, _ = inputs(sid)
    got = seq(sid, pre, w, out_img='bf16')
    rows, untouched = image_rows(got['out_img'], B, T, 4 * H)
    eq = np.array_equal(u16(rows).reshape(B, T, 2 * H), R.bf16_bits(got['out']))
    print(f'seq_options {sid} out_img bf16: equal {eq} untouched {untouched}')
    assert eq and untouched and all(forward_identical(got, plain(sid)).values())


@pytest.mark.parametrize('ws', [3, 6])
@shapes
def test_hi_only_forward(sid, ws):
    """The 16-bit data path's forward: F1, F2, F4 with the f16hi operand rounding (the tag emulated exactly) and the coarse chain check."""
    _, H, B, T, knobs = BY_ID[sid]
    pre, w, _ = inputs(sid, ws)
    r = plain(sid, ws, True)
    ops = R.operands_of(H, knobs, hi_only=True, B=B)
    f1, f2, f4 = R.check_f1(r['act'], r['csave']), R.check_f2(r['act'], r['csave'], r['out']), R.check_f4(pre, r['act'], r['out'], w, ops)
    wrong = R.check_f4(pre, r['act'], r['out'], w, R.operands_of(H, knobs, hi_only=False, B=B))      # what the check says of the other family
    b2 = R.check_b2_hi(dict(out=r['out']), *refs(H, B, T, ws))['out']
    print(f'seq_options {sid} hi_only forward ws {ws}: F1 {f1:.3f} F2 {f2:.3f} F4 {f4:.3f} (judged as f16x2: {wrong:.1f}) '
          f'b2_hi out {b2[0]:.2e}/{b2[1]:.2e} {b2[2]:.3f}')
    assert np.isfinite(r['out']).all()
    assert f1 <= 1.0 and f2 <= 1.0 and f4 <= 1.0 and b2[2] <= 1.0, (f1, f2, f4, b2)
    assert wrong > 1.0                                      # F4 tells the two operand roundings apart on this very run


# ------------------------------------------------------------------------------------------------ backward options
@shapes
def test_backward_repeats_bit_identically(sid):
    """Two plain runs at trained-scale W_hh: what the img_only comparison below rests on."""
    pre, w, d = inputs(sid)
    a, b = plain(sid), seq(sid, pre, w, d)
    same = {k: bool(np.array_equal(bits(a[k]), bits(b[k]))) for k in ('out', 'csave', 'act', 'dgates')}
    print(f'seq_options {sid} repeat: {same}')
    assert all(same.values()), same


@shapes
def test_amax(sid):
    pre, w, d = inputs(sid)
    base = plain(sid)
    got = seq(sid, pre, w, d, amax0=0.0)
    word, guard = body(got['amax'], 4)
    big = seq(sid, pre, w, d, amax0=1e30)
    zero = seq(sid, pre, w, np.zeros_like(d), amax0=0.0)
    res = dict(bits=int(word.view(np.uint32)[0]), want=R.amax_bits(got['dgates']), big=float(big['amax'][:4].view(R.F32)[0]),
               zero=int(zero['amax'][:4].view(np.uint32)[0]), guard=guard, dgates=bool(np.array_equal(bits(got['dgates']), bits(base['dgates']))))
    print(f'seq_options {sid} amax: {res}')
    assert res['bits'] == res['want'] != 0 and res['big'] == np.float32(1e30) and res['zero'] == 0 and guard and res['dgates']
    assert not zero['dgates'].any()


@shapes
def test_gbias(sid):
    _, H, B, T, _ = BY_ID[sid]
    pre, w, d = inputs(sid)
    g0 = np.random.default_rng(3).standard_normal(8 * H).astype(R.F32)
    got = seq(sid, pre, w, d, gbias0=g0)
    raw, guard = body(got['gbias'], 64 * H)
    g = raw.view(R.F32).reshape(2, 2, 4 * H)
    nbt = (B + 15) // 16
    halves = bool(np.array_equal(bits(g[:, 0]), bits(g[:, 1])))
    ratio = max(R.check_gbias(g[:, k].reshape(-1), g0, got['dgates'], nbt) for k in range(2))
    same = bool(np.array_equal(bits(got['dgates']), bits(plain(sid)['dgates'])))
    print(f'seq_options {sid} gbias: ratio (both halves) {ratio:.3f} halves identical {halves} guard {guard} dgates identical {same}')
    assert ratio <= 1.0 and guard and same
    assert halves or nbt > 1                                # one tile: one add per element, no order to depend on (module docstring)


@pytest.mark.parametrize('xf', [1, 8, 0], ids=['xf1', 'xf8', 'xfT'])
@shapes
def test_dgs(sid, xf):
    _, H, B, T, _ = BY_ID[sid]
    xf = xf or T
    pre, w, d = inputs(sid, 3, 0 if xf == 1 else xf)
    # seq_recurrence ties xf > 0 to a compact forward, as the engine does; without it the blocks are single frames
    got = seq(sid, pre, w, d, dgs=True) if xf == 1 else seq(sid, pre[:, ::xf], w, d, dgs=True, xf=xf)
    n = B * (T // xf) * 8 * H
    raw, guard = body(got['dgs'], 4 * n, padded(B) * 4 * (T // xf) * 8 * H)
    sums = raw.view(R.F32).reshape(B, T // xf, 8 * H)
    want = R.block_sums(got['dgates'], xf)
    res = dict(written=bool(np.isfinite(sums).all()), equal=bool(np.array_equal(bits(sums), bits(want))), guard=guard)
    if xf == 1:
        res['is_dgates'] = bool(np.array_equal(bits(sums), bits(np.float32(0) + got['dgates'])))      # the sum of one frame, started from +0
    base = plain(sid, 3, False, 8) if xf == 8 else seq(sid, pre, w, d)
    res['dgates'] = bool(np.array_equal(bits(got['dgates']), bits(base['dgates'])))
    print(f'seq_options {sid} dgs xf {xf}: {res}')
    assert all(res.values()), res


@shapes
def test_dimg(sid):
    """dimg beside the fp32 slab, then img_only: the slab keeps the forward's gates and every other output is that of the img_only = 0 run."""
    _, H, B, T, _ = BY_ID[sid]
    pre, w, d = inputs(sid)
    g0 = np.random.default_rng(4).standard_normal(8 * H).astype(R.F32)
    opts = dict(amax0=0.0, gbias0=g0, dgs=True, dimg=True)
    both = seq(sid, pre, w, d, **opts)
    rows, untouched = image_rows(both['dimg'], B, T, 16 * H)
    res = dict(equal=bool(np.array_equal(u16(rows).reshape(B, T, 8 * H), R.bf16_bits(both['dgates']))), untouched=untouched,
               dgates=bool(np.array_equal(bits(both['dgates']), bits(plain(sid)['dgates']))))
    only = seq(sid, pre, w, d, img_only=True, **opts)
    res['slab_keeps_gates'] = bool(np.array_equal(bits(only['dgates']), bits(only['act'])))
    res['act'] = bool(np.array_equal(bits(only['act']), bits(both['act'])))
    for k in ('amax', 'dgs', 'dimg'):
        res[k] = bool(np.array_equal(only[k], both[k]))
    nbt = (B + 15) // 16
    gb = [body(r['gbias'], 64 * H) for r in (both, only)]
    res['gbias_guard'] = gb[0][1] and gb[1][1]
    if nbt == 1:                                            # one add per element: the same bits; two tiles: each run within the bar
        res['gbias'] = bool(np.array_equal(only['gbias'], both['gbias']))
    gratio = max(R.check_gbias(g.view(R.F32).reshape(2, 2, 4 * H)[:, k].reshape(-1), g0, both['dgates'], nbt) for g, _ in gb for k in range(2))
    print(f'seq_options {sid} dimg: gbias ratio (both runs, both halves) {gratio:.3f} {res}')
    assert all(res.values()), res
    assert gratio <= 1.0


@pytest.mark.parametrize('ws', [3, 6])
@shapes
def test_hi_only_backward(sid, ws):
    """The 16-bit data path's backward on the state its own hi_only forward saved: B3 with the f16hi operand rounding, and the coarse chain
    check for dgates and dW_hh."""
    _, H, B, T, knobs = BY_ID[sid]
    pre, w, d = inputs(sid, ws)
    r = plain(sid, ws, True)
    ops = R.operands_of(H, knobs, hi_only=True, B=B)
    b3 = R.check_b3(r['act'], r['csave'], d, r['dgates'], w, ops)
    wrong = R.check_b3(r['act'], r['csave'], d, r['dgates'], w, R.operands_of(H, knobs, hi_only=False, B=B))
    b2 = R.check_b2_hi(dict(dgates=r['dgates'], dw_hh=R.dw_hh(r['dgates'], r['out'])), *refs(H, B, T, ws))
    print(f'seq_options {sid} hi_only backward ws {ws}: B3 {b3:.3f} (judged as f16x2: {wrong:.1f}) ' +
          ' '.join(f'b2_hi {k} {e:.2e}/{e16:.2e} {q:.3f}' for k, (e, e16, q) in sorted(b2.items())))
    assert np.isfinite(r['dgates']).all()
    assert b3 <= 1.0 and all(q <= 1.0 for _, _, q in b2.values()), (b3, b2)
    assert wrong > 1.0


# ------------------------------------------------------------------------------------------------ what the engine runs
@pytest.mark.parametrize('path', ['fp32', '16bit'])
@shapes
def test_engine_combinations(sid, path):
    """fp32 decoder layer 0: xc with xf = 8 and a v2 out_img forward; amax, gbias, dgs backward.  16-bit path: xc, a bf16 out_img and hi_only
    forward; amax, gbias, dgs, dimg, img_only and hi_only backward.  Every side output against the option-free run on the same input."""
    _, H, B, T, knobs = BY_ID[sid]
    hi = path == '16bit'
    pre, w, d = inputs(sid, 3, 8)
    base = plain(sid, 3, hi, 8)
    g0 = np.random.default_rng(5).standard_normal(8 * H).astype(R.F32)
    got = seq(sid, pre[:, ::8], w, d, xf=8, out_img='bf16' if hi else 'v2', hi_only=hi, amax0=0.0, gbias0=g0, dgs=True, dimg=hi, img_only=hi)
    dg = base['dgates']                                     # under img_only the run leaves no fp32 gradients of its own: the repeat's
    res = dict(forward=all(forward_identical(got, base).values()))
    rows, res['out_img_untouched'] = image_rows(got['out_img'], B, T, (4 if hi else 8) * H)
    res['out_img'] = bool(np.array_equal(u16(rows).reshape(B, T, 2 * H), R.bf16_bits(got['out']))) if hi else bool(np.array_equal(rows, split_bytes(got['out'])))
    res['dgates'] = bool(np.array_equal(bits(got['dgates']), bits(got['act'] if hi else dg)))
    res['amax'] = int(got['amax'][:4].view(np.uint32)[0]) == R.amax_bits(dg)
    gb, res['gbias_guard'] = body(got['gbias'], 64 * H)
    gb = gb.view(R.F32).reshape(2, 2, 4 * H)
    nbt = (B + 15) // 16
    if nbt == 1:
        res['gbias_halves'] = bool(np.array_equal(bits(gb[:, 0]), bits(gb[:, 1])))
    gratio = max(R.check_gbias(gb[:, k].reshape(-1), g0, dg, nbt) for k in range(2))
    sums, res['dgs_guard'] = body(got['dgs'], 4 * B * (T // 8) * 8 * H, padded(B) * 4 * (T // 8) * 8 * H)
    res['dgs'] = bool(np.array_equal(bits(sums.view(R.F32).reshape(B, T // 8, 8 * H)), bits(R.block_sums(dg, 8))))
    if hi:
        rows, res['dimg_untouched'] = image_rows(got['dimg'], B, T, 16 * H)
        res['dimg'] = bool(np.array_equal(u16(rows).reshape(B, T, 8 * H), R.bf16_bits(dg)))
    ops = R.operands_of(H, knobs, hi_only=hi, B=B)
    ratios = dict(F1=R.check_f1(got['act'], got['csave']), F2=R.check_f2(got['act'], got['csave'], got['out']),
                  F4=R.check_f4(pre, got['act'], got['out'], w, ops), B3=R.check_b3(got['act'], got['csave'], d, dg, w, ops), gbias=gratio)
    print(f'seq_options {sid} engine {path}: ' + ' '.join(f'{k} {v:.3f}' for k, v in ratios.items()) + f' {res}')
    assert all(res.values()), res
    assert all(v <= 1.0 for v in ratios.values()), ratios
