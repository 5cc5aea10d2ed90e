"""The F0-guided harmonic mel inversion and the harmonic start phases on the GPU (ss_mel_to_linear_harmonic, ss_harmonic_phase;
csrc/vocoder.hip) against their float64 numpy restatement (harmonic_ref.py, proven on wrong stand-ins by test_harmonic_ref_selftest.py):
pytest -m gpu.  Shapes: harmonic_ref.parity_inputs -- 4, 5, 9 and 41 frames of features.npz's u1_wav and the 49 of u0_wav through
features.npz's own basis, F0 from pitch_ref.track -- the ragged batch [4, 9, 41], two synthetic tracks at the edges of the voiced range and
one that alternates; seconds in total.

Conditions, asserted on the reference when the module is set up (harmonic_ref.conditions): no k / p_1 within 1e-9 of a half-integer, no
voiced f within 1e-9 (relative) of 40, 1000 or a step of floor(f_top / f); every input has voiced and unvoiced frames.  The recorded
tracks hold them as they are.  The low edge is 40.5003 Hz, not 40.5: at 40.5 exactly, 162 / p_1 is 62.5 to the bit.

Bound.  Per input and round count, harmonic_ref.gpu_bound of the restatement's own two-order disagreement (numpy matmuls with A formed
against the kernel's order), measured when the module is set up: 100 x it, capped at 1e-9 -- one factor of 10 for a third way of rounding
the same sums (fused multiply-adds in a fixed order), one for the device's pow, sqrt, sincos and atan2.  A disagreement below 2^-52 (at
n_iter 0 the two orders take the same sums) counts as 2^-52.  S is relative to max |S|, the share absolute, phases |e^{ia} - e^{ib}|, per
element, nothing left out; u is compared to the bit.

phase0 is the SECOND call's output, and it is compared on one and the same share: ss_harmonic_phase on the restatement's share against
the restatement's phase0, and chained on the GPU's own share against the restatement applied to that share.  The share reaches the call
rounded to a double, and the definition's sqrt(1 - w^2) turns one unit in the last place of a share next to 1 into 1.5e-8 of phase -- the
restatement's own two orders end 9.3e-9 apart on u1 at 50 rounds, above the cap -- so two computations of the share cannot be held to
1e-9 of phase through it; that conditioning is the definition's, recorded in test_harmonic_ref_selftest.py.  The difference the chain makes
is printed.

Measured (MI355X), GPU against the kernel-order restatement, the two-order disagreement of the same input and count in brackets:

    input    n_iter 50: S of max |S|     share                 phase0, one share    chained GPU phase0 vs the restatement's
    u1_4     6.8e-16 (3.4e-16)           2.8e-15 (1.6e-15)     9.2e-16              1.0e-8   (two orders 8.9e-9)
    u1_5     4.3e-16 (4.5e-16)           1.7e-14 (1.7e-14)     9.6e-16              3.7e-9   (3.4e-9)
    u1_9     4.2e-16 (4.6e-16)           6.3e-14 (4.7e-15)     2.5e-15              9.2e-9   (7.7e-9)
    u1_41    3.8e-16 (4.2e-16)           5.7e-13 (9.5e-14)     1.5e-15              4.2e-9   (1.2e-8)
    u0       2.7e-16 (2.7e-16)           5.5e-14 (8.8e-14)     1.8e-15              2.5e-12  (9.8e-13)
    40.5003  2.1e-15 (1.4e-15)           2.3e-14 (2.1e-14)     9.6e-16              2.1e-8   (2.1e-8)
    999      2.5e-16 (5.0e-16)           2.2e-15 (4.4e-16)     7.5e-16              1.1e-14  (8.7e-16)

at n_iter 0 and 1 every figure is below 2.1e-14 (S, share) and 8.3e-15 (phase0 on one share); u equals numpy's to the bit everywhere.
End to end on u1's 41 frames: waveform 6.0e-12 (0 rounds) and 8.3e-12 (8 rounds) of max |x| against a bound of 3.7e-10; the claim's
ratios 0.3987 (u0) and 0.2888 (u1) against bars of 0.6995 and 0.6445.

Every test prints its figures before it asserts; those of one run (pytest -s) are kept in profiles/r05/harmonic/test_figures.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import griffinlim_ref as R
from tests import guarded as G
from tests import harmonic_ref as H
from tests import nnls_ref as N

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
NAMES = ('u1_4', 'u1_5', 'u1_9', 'u1_41', 'u0')
RAGGED = ('u1_4', 'u1_9', 'u1_41')
NAN = float('nan')
FLOOR, F_TOP = 1e-10, 7600.0
EDGE_LOW, EDGE_HIGH = 40.5003, 999.0                                     # H = 187 and H = 7
CLAIM_BAR = {'u0': 0.6995, 'u1_41': 0.6445}                              # test_harmonic_ref_selftest.py: midway between the measured ratio and 1


@pytest.fixture(scope='module')
def V():
    from speechsplit_amd import vocoder
    return vocoder


@pytest.fixture(scope='module')
def lib():
    from speechsplit_amd import _capi
    return _capi.lib()


@pytest.fixture(scope='module')
def feats():
    return np.load(os.path.join(GOLD, 'features.npz'))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _frames(fr):
    return torch.tensor(fr, dtype=torch.int32, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


class Basis:
    def __init__(self, B):
        self.B = np.ascontiguousarray(B, dtype=np.float64)
        self.n = self.B.shape[1]
        self.P = np.linalg.pinv(self.B)
        self.step = N.step_of(self.B)
        self.packed = N.pack(self.B)
        self.P_dev, self.packed_dev = _dev(self.P), _dev(self.packed)


@pytest.fixture(scope='module')
def bank(feats):
    return Basis(feats['mel_basis'])


def _reference(bank, mel, hz, seed):
    """per round count the kernel-order (S, share, phase0), the two-order disagreements and the bounds; computed once"""
    H.conditions(hz)
    rand = np.random.default_rng(seed).uniform(-np.pi, np.pi, (mel.shape[0], 513))
    ref = {}
    for it in H.ITERS:
        (S, w, ph), d = H.disagreement(mel, hz, bank.B, bank.P, rand, it)
        assert d[0] <= H.DISAGREEMENT_CAP and d[1] <= H.DISAGREEMENT_CAP
        ref[it] = dict(S=S, share=w, phase0=ph, div=d, bound=tuple(H.gpu_bound(x) for x in d))
    return dict(mel=mel, hz=hz, rand=rand, ref=ref, u=H.phase_u(hz))


@pytest.fixture(scope='module')
def inputs(feats, bank):
    out = {}
    for n, (name, (mel, hz)) in enumerate(H.parity_inputs(feats).items()):
        v = H.voiced(hz)
        assert v.any() and not v.all(), name
        out[name] = _reference(bank, mel, hz, 100 + n)
    return out


def route(lib, basis, mel, frames=None, which='pinv'):
    """the magnitude either existing route fills, as a device tensor [B, T, 513]"""
    B, T, n = mel.shape
    mag = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    if which == 'pinv':
        rc = lib.ss_mel_to_linear(_p(mel), _p(basis.P_dev), _p(frames), B, T, n, FLOOR, _p(mag), _s())
    else:
        rc = lib.ss_mel_to_linear_nnls(_p(mel), _p(basis.P_dev), _p(basis.packed_dev), basis.packed_dev.numel(), _p(frames), B, T, n, 50,
                                       basis.step, FLOOR, _p(mag), _s())
    assert rc == 0, lib.ss_last_error()
    return mag


def fit(lib, basis, mel, hz, n_iter, frames=None, which='pinv', f_top=F_TOP):
    """mel float32 [B, T, n] and hz float64 [B, T] on the device -> (mag, share) float64 numpy [B, T, 513]"""
    B, T, n = mel.shape
    assert mel.dtype == torch.float32 and hz.dtype == torch.float64 and hz.shape == (B, T) and mel.is_contiguous() and hz.is_contiguous()
    mag = route(lib, basis, mel, frames, which)
    share = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    rc = lib.ss_mel_to_linear_harmonic(_p(mel), _p(hz), _p(basis.P_dev), _p(basis.packed_dev), basis.packed_dev.numel(), _p(frames), B, T, n,
                                       f_top, n_iter, FLOOR, _p(mag), _p(share), _s())
    assert rc == 0, lib.ss_last_error()
    return mag.cpu().numpy(), share.cpu().numpy()


def phase(lib, hz, share, rand, frames=None, f_top=F_TOP):
    """hz [B, T], share and rand [B, T, 513] on the device -> phase0 float64 numpy"""
    B, T = hz.shape
    nb = lib.ss_harmonic_phase_scratch_bytes(B, T)
    assert nb >= B * T * 8
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    rc = lib.ss_harmonic_phase(_p(hz), _p(share), _p(rand), _p(frames), B, T, f_top, _p(out), _p(scratch), nb, _s())
    assert rc == 0, lib.ss_last_error()
    return out.cpu().numpy()


def u_of(lib, hz, frames=None):
    B, T = hz.shape
    u = torch.full((B, T), NAN, dtype=torch.float64, device=DEV)
    assert lib.ss_op_harmonic_u(_p(hz), _p(frames), B, T, _p(u), _s()) == 0, lib.ss_last_error()
    return u.cpu().numpy()


def _check(tag, lib, bank, inp, its=H.ITERS):
    """the parity of one input at every round count: S, share, phase0 (on one and the same share) and u"""
    mel, hz, rand = _dev(inp['mel'], torch.float32)[None], _dev(inp['hz'])[None], _dev(inp['rand'])[None]
    assert np.array_equal(_bits(u_of(lib, hz)[0]), _bits(inp['u'])), tag
    for it in its:
        ref = inp['ref'][it]
        S, w = fit(lib, bank, mel, hz, it)
        assert np.isfinite(S).all() and np.isfinite(w).all() and w.min() >= 0.0 and w.max() <= 1.0 and S.min() >= FLOOR
        dS, dw = H.rel_diff(S[0], ref['S']), H.abs_diff(w[0], ref['share'])
        on_ref = H.phase_diff(phase(lib, hz, _dev(ref['share'])[None], rand)[0], ref['phase0'])
        chained = phase(lib, hz, _dev(w), rand)[0]
        on_own = H.phase_diff(chained, H.harmonic_phase(inp['hz'], w[0], inp['rand']))
        print(f'{tag}, n_iter {it}: S {dS:.3g} of max |S| (two orders {ref["div"][0]:.3g}, bound {ref["bound"][0]:.3g}); '
              f'share {dw:.3g} ({ref["div"][1]:.3g}, {ref["bound"][1]:.3g}); phase0 on the reference\'s share {on_ref:.3g}, on its own '
              f'{on_own:.3g} ({ref["div"][2]:.3g}, {ref["bound"][2]:.3g}); chained against the reference\'s phase0 '
              f'{H.phase_diff(chained, ref["phase0"]):.3g}')
        assert dS <= ref['bound'][0]
        assert dw <= ref['bound'][1]
        assert on_ref <= ref['bound'][2] and on_own <= ref['bound'][2]


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize('name', NAMES)
def test_parity(lib, bank, inputs, name):
    _check(name, lib, bank, inputs[name])


def _edge_track(kind, F):
    if kind == 'low':
        return np.full(F, EDGE_LOW)
    if kind == 'high':
        return np.full(F, EDGE_HIGH)
    hz = np.where(np.arange(F) % 2 == 0, 0.0, 110.37 + 3.1307 * np.arange(F))   # alternating: every voiced frame restarts at u = 0
    hz[-3:] = 131.21, 133.57, 0.0                                            # and one pair that chains (whole Hz would put k / p_1 on halves)
    return hz


@pytest.mark.parametrize('kind', ['low', 'high', 'alternating'])
def test_edges_of_the_voiced_range_and_alternating_frames(lib, bank, inputs, kind):
    mel = inputs['u1_9']['mel']
    hz = _edge_track(kind, 9)
    assert kind == 'alternating' or H.count(hz[0]) == {'low': 187, 'high': 7}[kind]
    inp = _reference(bank, mel, hz, 31)
    if kind == 'alternating':
        assert H.voiced(hz).tolist() == [False, True] * 3 + [True, True, False]
        assert not inp['u'][:6].any() and inp['u'][6] > 0.0 and inp['u'][7] > 0.0 and inp['u'][8] == 0.0
    _check(kind, lib, bank, inp, its=(1, 50))


def test_two_runs_give_the_same_bits(lib, bank, inputs):
    inp = inputs['u1_41']
    mel, hz = _dev(inp['mel'], torch.float32)[None], _dev(inp['hz'])[None]
    a, b = fit(lib, bank, mel, hz, 50), fit(lib, bank, mel, hz, 50)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


# ---------------------------------------------------------------------------------------------- unvoiced
@pytest.mark.parametrize('which', ['pinv', 'nnls'])
def test_an_all_unvoiced_track_is_the_filled_route_bit_for_bit(lib, bank, inputs, which):
    inp = inputs['u1_9']
    mel, rand = _dev(inp['mel'], torch.float32)[None], _dev(inp['rand'])[None]
    hz = _dev(np.array([NAN, 0.0, 39.9, 1000.1, -1.0, np.inf, -np.inf, -0.0, 1e300]))[None]
    want = route(lib, bank, mel, None, which).cpu().numpy()
    for it in (0, 50):
        S, w = fit(lib, bank, mel, hz, it, which=which)
        assert np.array_equal(_bits(S), _bits(want)) and not w.any() and not np.signbit(w).any()
    assert np.array_equal(_bits(phase(lib, hz, _dev(w), rand)), _bits(inp['rand'][None]))
    assert not phase(lib, hz, _dev(w), None).any()                                        # NULL rand_phase_dev: zeros
    assert not u_of(lib, hz).any()
    # and on a voiced track the unvoiced frames keep the route's bits while the voiced ones leave them
    S, w = fit(lib, bank, mel, _dev(inp['hz'])[None], 50, which=which)
    v = H.voiced(inp['hz'])
    assert np.array_equal(_bits(S[0, ~v]), _bits(want[0, ~v])) and not w[0, ~v].any() and (S[0, v] != want[0, v]).any()


# ---------------------------------------------------------------------------------------------- ragged batches
def _batch(rows, T, fill):
    out = np.full((len(rows), T) + rows[0].shape[1:], fill, rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


def test_ragged_batch_rows_are_the_utterances_alone(lib, bank, inputs):
    rows = [inputs[n] for n in RAGGED]
    lens = [r['mel'].shape[0] for r in rows]
    assert lens == [4, 9, 41]
    T, fr = 41, _frames(lens)
    # beyond a row's frames: NaN in mel, a VOICED value in f0 (a kernel that read it would fit NaN there), NaN in the phases
    mel = _dev(_batch([r['mel'] for r in rows], T, NAN), torch.float32)
    hz = _dev(_batch([r['hz'] for r in rows], T, 100.0))
    rand = _dev(_batch([r['rand'] for r in rows], T, NAN))
    S, w = fit(lib, bank, mel, hz, 50, fr)
    share = _dev(w)
    share[0, 4:], share[1, 9:] = NAN, NAN
    ph, u = phase(lib, hz, share, rand, fr), u_of(lib, hz, fr)
    clean = fit(lib, bank, _dev(_batch([r['mel'] for r in rows], T, 0.0), torch.float32), _dev(_batch([r['hz'] for r in rows], T, NAN)), 50, fr)
    assert np.array_equal(_bits(S), _bits(clean[0])) and np.array_equal(_bits(w), _bits(clean[1]))
    for b, (r, F) in enumerate(zip(rows, lens)):
        m1, h1, r1 = _dev(r['mel'], torch.float32)[None], _dev(r['hz'])[None], _dev(r['rand'])[None]
        S1, w1 = fit(lib, bank, m1, h1, 50)
        assert np.array_equal(_bits(S[b, :F]), _bits(S1[0])) and np.array_equal(_bits(w[b, :F]), _bits(w1[0])), b    # bit for bit
        assert np.array_equal(_bits(ph[b, :F]), _bits(phase(lib, h1, _dev(w1), r1)[0])), b
        assert np.array_equal(_bits(u[b, :F]), _bits(r['u'])), b
        for tail in (S[b, F:], w[b, F:], ph[b, F:], u[b, F:]):                              # the route's zeros, and zeros
            assert not tail.any() and not np.signbit(tail).any(), b
        assert H.rel_diff(S[b, :F], r['ref'][50]['S']) <= r['ref'][50]['bound'][0]


def test_frame_counts_outside_the_contract_spoil_their_row_only(lib, bank, inputs):
    inp = inputs['u1_9']
    mel, hz = _dev(np.stack([inp['mel']] * 4), torch.float32), _dev(np.stack([inp['hz']] * 4))
    S, w = fit(lib, bank, mel, hz, 5, _frames([-3, 9, 5, 1 << 30]))
    full = fit(lib, bank, mel[:1], hz[:1], 5)
    for b, F in ((0, 4), (1, 9), (2, 5), (3, 9)):
        assert np.array_equal(_bits(S[b, :F]), _bits(full[0][0, :F])) and np.array_equal(_bits(w[b, :F]), _bits(full[1][0, :F]))
        assert not S[b, F:].any() and not w[b, F:].any()


# ---------------------------------------------------------------------------------------------- containment
CB, CT, CFR = 4, 8, [8, 4, 6, 5]                                          # 32 doubles of u: exactly the 256 bytes of scratch


def _guarded_call(lib, bank, inputs, packed):
    inp = inputs['u1_9']
    rows = [inp['mel'][:F] for F in CFR]
    hzs = [inp['hz'][:F] for F in CFR]
    fr = torch.tensor(CFR, dtype=torch.int32)
    filled = route(lib, bank, _dev(_batch(rows, CT, 0.0), torch.float32), fr.to(DEV))
    gm, gh = G.inp(_batch(rows, CT, NAN), DEV, name='mel'), G.inp(_batch(hzs, CT, 100.0), DEV, name='f0_hz')
    gi, gp, gf = G.inp(bank.P, DEV, name='inv_basis'), G.inp(packed, DEV, name='packed'), G.inp(fr, DEV, name='frames')
    gr = G.inp(_batch([inp['rand'][:F] for F in CFR], CT, NAN), DEV, name='rand_phase')
    gmag = G.out((CB, CT, 513), DEV, dtype=torch.float64, fill=filled, name='mag')
    gw = G.out((CB, CT, 513), DEV, dtype=torch.float64, name='share')
    gph = G.out((CB, CT, 513), DEV, dtype=torch.float64, name='phase0')
    gu = G.out((CB * CT,), DEV, dtype=torch.float64, name='scratch')
    assert lib.ss_harmonic_phase_scratch_bytes(CB, CT) == 256 and gu.t.data_ptr() % 256 == 0
    rc = lib.ss_mel_to_linear_harmonic(_p(gm.t), _p(gh.t), _p(gi.t), _p(gp.t), packed.shape[0], _p(gf.t), CB, CT, 80, F_TOP, 50, FLOOR,
                                       _p(gmag.t), _p(gw.t), _s())
    assert rc == 0, lib.ss_last_error()
    rc = lib.ss_harmonic_phase(_p(gh.t), _p(gw.t), _p(gr.t), _p(gf.t), CB, CT, F_TOP, _p(gph.t), _p(gu.t), 256, _s())
    assert rc == 0, lib.ss_last_error()
    torch.cuda.synchronize()
    G.check_all([gm, gh, gi, gp, gf, gr, gmag, gw, gph, gu])
    return rows, hzs, filled.cpu().numpy(), gmag.t.cpu().numpy(), gw.t.cpu().numpy(), gph.t.cpu().numpy()


def test_containment(lib, bank, inputs):
    rows, hzs, filled, S, w, ph = _guarded_call(lib, bank, inputs, bank.packed)
    for b, F in enumerate(CFR):
        ref_S, ref_w = H.mel_to_linear_harmonic(rows[b], hzs[b], bank.B, filled[b, :F], 50, order='kernel', inv_basis=bank.P)
        assert H.rel_diff(S[b, :F], ref_S) <= 100.0 * H.DISAGREEMENT_CAP and H.abs_diff(w[b, :F], ref_w) <= 100.0 * H.DISAGREEMENT_CAP
        assert np.isfinite(ph[b, :F]).all()
        assert not S[b, F:].any() and not w[b, F:].any() and not ph[b, F:].any()


def test_a_corrupt_packed_buffer_stays_inside_its_outputs(lib, bank, inputs):
    """first bins and run lengths far outside the 513 bins and the packed weights, NaN and infinities among them: every index is clamped, so
    the numbers are wrong and nothing else is -- the guards around mag, share, phase0, the scratch and every input are untouched"""
    bad = bank.packed.copy()
    bad[0:160:2] = np.resize([-5.0, 1e18, 700.0, NAN, 512.0, -np.inf, 300.5], 80)
    bad[1:160:2] = np.resize([1e18, 600.0, -4.0, 513.0, NAN, np.inf, 941.0], 80)
    _guarded_call(lib, bank, inputs, bad)


# ---------------------------------------------------------------------------------------------- the Python layer, end to end
def test_python_mel_to_linear_with_f0(V, lib, bank, inputs):
    inp = inputs['u1_41']
    ln = np.where(H.voiced(inp['hz']), np.log(np.where(inp['hz'] > 0.0, inp['hz'], 1.0)), -1e10)
    assert np.array_equal(V.f0_hz(ln) > 0.0, H.voiced(inp['hz']))
    mel, hz = _dev(inp['mel'], torch.float32)[None], _dev(V.f0_hz(ln))[None]
    for which in ('pinv', 'nnls'):
        got, share = V.mel_to_linear(inp['mel'], bank.B, inversion=which, nnls_iter=50, f0=ln, return_share=True)
        S, w = fit(lib, bank, mel, hz, 50, which=which)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(S[0])) and np.array_equal(_bits(share.cpu().numpy()), _bits(w[0]))
    assert np.array_equal(V.mel_to_linear(inp['mel'], bank.B).cpu().numpy(), route(lib, bank, mel)[0].cpu().numpy())   # without f0: the route


def test_end_to_end_griffin_lim_with_f0_agrees_with_numpy_and_holds_the_claim(V, lib, bank, inputs, feats):
    """griffin_lim(mel_u1, f0=...) at 0 and 8 rounds against harmonic_ref then griffinlim_ref.griffin_lim, within the vocoder tests' own
    41-frame bound (100 x the fft / dft divergence of Griffin-Lim on u1's 41 frames, capped at 1e-9 of max |x|: 3.7e-10).  Then the claim:
    the GPU's S is closer to the recording's |stft| than the pseudo-inverse route's by the self-test's bar, on u0 and u1."""
    inp = inputs['u1_41']
    ln = np.where(H.voiced(inp['hz']), np.log(np.where(inp['hz'] > 0.0, inp['hz'], 1.0)), -1e10)
    hz = V.f0_hz(ln)
    ph = np.random.default_rng(5).uniform(-np.pi, np.pi, (41, 513))
    S_ref, w_ref, ph_ref = H.full(inp['mel'], hz, bank.B, bank.P, ph, 50)
    S41, ph41 = R.parity_input(feats['u1_wav'], 41)
    bound = min(1e-9, 100.0 * R.divergence(S41, ph41))
    for rounds in (0, 8):
        wav = V.griffin_lim(inp['mel'], n_iter=rounds, generator=np.random.default_rng(5), mel_basis=bank.B, f0=ln)
        ref = R.griffin_lim(S_ref, rounds, 0.99, ph_ref)
        d = R.rel_diff(wav, ref)
        print(f'end to end, {rounds} rounds: waveform {d:.3g} of max |x|, bound {bound:.3g}')
        assert wav.dtype == np.float64 and wav.shape == (256 * 40,)
        assert d <= bound
    # without f0 the waveform is the bits it was: the two existing routes, through the same call
    a = V.griffin_lim(inp['mel'], n_iter=2, generator=np.random.default_rng(5), mel_basis=bank.B)
    b = V.griffin_lim(inp['mel'], n_iter=2, generator=np.random.default_rng(5), mel_basis=bank.B, f0=np.full(41, -1e10))
    assert np.array_equal(_bits(a), _bits(b))
    # batching does not change a row: the list form, ragged, one and two rows a batch
    mels = [inputs[n]['mel'] for n in ('u1_9', 'u1_41', 'u1_5')]
    f0s = [np.where(H.voiced(inputs[n]['hz']), np.log(np.where(inputs[n]['hz'] > 0.0, inputs[n]['hz'], 1.0)), -1e10) for n in ('u1_9', 'u1_41', 'u1_5')]
    runs = [V.griffin_lim(mels, n_iter=2, generator=np.random.default_rng(2), max_rows=r, mel_basis=bank.B, f0=f0s) for r in (1, 2)]
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(*runs))
    # the claim, on the GPU's S
    for name, key in (('u0', 'u0_wav'), ('u1_41', 'u1_wav')):
        i = inputs[name]
        true = np.abs(R.stft(np.asarray(feats[key], np.float64)))
        err = lambda x: float(np.linalg.norm(x - true) / np.linalg.norm(true))
        mel, hzd = _dev(i['mel'], torch.float32)[None], _dev(i['hz'])[None]
        e_h, e_p = err(fit(lib, bank, mel, hzd, 50)[0][0]), err(route(lib, bank, mel)[0].cpu().numpy())
        print(f'{name}: S against the recording\'s |stft| {e_h:.4f}, the pseudo-inverse route {e_p:.4f}: ratio {e_h / e_p:.4f}, bar {CLAIM_BAR[name]}')
        assert e_h / e_p <= CLAIM_BAR[name]
