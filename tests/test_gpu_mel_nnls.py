"""The non-negative mel inversion on the GPU (ss_mel_to_linear_nnls, csrc/vocoder.hip) against its float64 numpy restatement (nnls_ref.py,
proven on wrong stand-ins by test_nnls_ref_selftest.py): pytest -m gpu.  Shapes: 4, 5, 9 and 41 frames of features.npz's u1_wav through the
project's own filter bank, the ragged batch [41, 9, 5]; seconds in total.

Bound.  Per input and iteration count, 100 x the disagreement of the reference's own two summation orders (numpy matmuls against the
kernel's band order), relative to max |x|, measured when the module is set up -- the rule test_gpu_vocoder.py uses for fft against dft: one
factor of 10 for a third way of rounding the same sums (fused multiply-adds in a fixed order), one for the device's pow, sqrt and the
starting product.  The self-test holds the disagreement under 1e-11 and the smallest wrong variant (6.6e-4) 100 x above any such bound.
Measured (MI355X; the dense-vs-band column on the host of that run), of max |x|:

    frames   n_iter 1: dense vs band / GPU    50: dense vs band / GPU    200: dense vs band / GPU
    4        1.9e-16 / 1.9e-16                8.3e-15 / 8.3e-15          2.0e-14 / 2.1e-14
    5        5.5e-17 / 2.2e-16                3.2e-15 / 2.8e-15          1.5e-14 / 3.3e-14
    9        1.0e-16 / 2.1e-16                3.6e-15 / 3.6e-15          2.5e-14 / 3.7e-14
    41       2.0e-16 / 2.0e-16                8.6e-15 / 6.9e-15          3.7e-14 / 4.4e-14

Every test prints its figures before it asserts; those of one run (pytest -s) are kept in profiles/r05/nnls/test_figures.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import griffinlim_ref as R
from tests import guarded as G
from tests import nnls_ref as N

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
FRAMES = (4, 5, 9, 41)
RAGGED = [41, 9, 5]
NAN = float('nan')
FLOOR = 1e-10


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


class Basis:
    """a [513, n_mels] basis with everything the call takes, on the host and on the device"""

    def __init__(self, B):
        self.B = np.ascontiguousarray(B, dtype=np.float64)
        self.n = self.B.shape[1]
        self.P = np.linalg.pinv(self.B)
        self.step = N.step_of(self.B)
        self.packed = N.pack(self.B)
        self.P_dev, self.packed_dev = _dev(self.P), _dev(self.packed)


@pytest.fixture(scope='module')
def bank():
    from speechsplit_amd import features
    return Basis(features.mel_filter_bank().T)


@pytest.fixture(scope='module')
def inputs(feats, bank):
    """frames -> the mel, and per iteration count the band-order reference with its bound"""
    out = {}
    for F in FRAMES:
        mel = N.parity_mel(feats['u1_wav'], F, bank.B)
        ref = {}
        for it in N.ITERS:
            band, d = N.disagreement(mel, bank.B, it, bank.P, bank.step)
            assert d <= N.DISAGREEMENT_CAP
            ref[it] = dict(x=band, div=d, bound=100.0 * d)
        out[F] = dict(mel=mel, ref=ref, pinv=R.mel_to_linear(mel, bank.P))
    return out


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _frames(fr):
    return torch.tensor(fr, dtype=torch.int32, device=DEV)


def nnls(lib, basis, mel, n_iter, frames=None, floor=FLOOR, mag=None, step=None):
    """mel float32 tensor [B, T, n_mels] on the device -> float64 numpy [B, T, 513]"""
    B, T, n = mel.shape
    assert n == basis.n and mel.dtype == torch.float32 and mel.is_contiguous()
    if mag is None:
        mag = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    rc = lib.ss_mel_to_linear_nnls(_p(mel), _p(basis.P_dev), _p(basis.packed_dev), basis.packed_dev.numel(), _p(frames), B, T, n, n_iter,
                                   basis.step if step is None else step, floor, _p(mag), _s())
    assert rc == 0, lib.ss_last_error()
    return mag.cpu().numpy()


def pinv_path(lib, basis, mel, frames=None, floor=FLOOR):
    B, T, n = mel.shape
    mag = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    assert lib.ss_mel_to_linear(_p(mel), _p(basis.P_dev), _p(frames), B, T, n, floor, _p(mag), _s()) == 0, lib.ss_last_error()
    return mag.cpu().numpy()


def _batch(rows, T, fill=NAN):
    out = np.full((len(rows), T, rows[0].shape[1]), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize('F', FRAMES)
def test_parity(lib, bank, inputs, F):
    mel = _dev(inputs[F]['mel'], torch.float32)[None]
    for it in N.ITERS:
        ref = inputs[F]['ref'][it]
        got = nnls(lib, bank, mel, it)[0]
        assert got.shape == (F, 513) and np.isfinite(got).all()
        d = N.rel_diff(got, ref['x'])
        print(f'{F} frames, n_iter {it}: GPU vs band-order reference {d:.3g} of max |x| (dense vs band {ref["div"]:.3g}, bound {ref["bound"]:.3g})')
        assert d <= ref['bound']


@pytest.mark.parametrize('F', FRAMES)
def test_zero_iterations_are_ss_mel_to_linear_bit_for_bit(lib, bank, inputs, F):
    mel = _dev(inputs[F]['mel'], torch.float32)[None]
    for floor in (FLOOR, 0.0, 0.5):
        a, b = nnls(lib, bank, mel, 0, floor=floor), pinv_path(lib, bank, mel, floor=floor)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), floor
    assert N.rel_diff(a[0], R.mel_to_linear(inputs[F]['mel'], bank.P, 0.5)) <= 1e-12


def test_two_runs_give_the_same_bits(lib, bank, inputs):
    T = max(RAGGED)
    mel, fr = _dev(_batch([inputs[F]['mel'] for F in RAGGED], T), torch.float32), _frames(RAGGED)
    a, b = nnls(lib, bank, mel, 200, fr), nnls(lib, bank, mel, 200, fr)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize('F', (5, 9, 41))
def test_residual_falls_a_thousandfold_and_nothing_is_below_the_floor(lib, bank, inputs, F):
    mel = inputs[F]['mel']
    got = nnls(lib, bank, _dev(mel, torch.float32)[None], 200)[0]
    res, res0 = N.residual(got, mel, bank.B), N.residual(inputs[F]['pinv'], mel, bank.B)
    print(f'{F} frames: residual {res:.3g} against the floored pseudo-inverse\'s {res0:.3g}')
    assert res * 1000.0 <= res0
    assert got.min() >= FLOOR
    dead = bank.B.sum(axis=1) == 0                                       # bins no band covers keep their start
    assert dead.sum() == 32 and np.array_equal(got[:, dead], pinv_path(lib, bank, _dev(mel, torch.float32)[None])[0][:, dead])


# ---------------------------------------------------------------------------------------------- ragged batches
def test_ragged_batch_rows_are_the_utterances_alone(lib, bank, inputs):
    T, fr = max(RAGGED), _frames(RAGGED)
    rows = [inputs[F]['mel'] for F in RAGGED]
    got = nnls(lib, bank, _dev(_batch(rows, T), torch.float32), 50, fr)      # NaN in every mel frame a row does not own
    clean = nnls(lib, bank, _dev(_batch(rows, T, 0.0), torch.float32), 50, fr)
    assert np.array_equal(got.view(np.int64), clean.view(np.int64))
    for b, F in enumerate(RAGGED):
        alone = nnls(lib, bank, _dev(rows[b], torch.float32)[None], 50)[0]
        assert np.array_equal(got[b, :F].view(np.int64), alone.view(np.int64)), (b, F)   # bit for bit
        assert not got[b, F:].any() and not np.signbit(got[b, F:]).any(), (b, F)
        assert N.rel_diff(got[b, :F], inputs[F]['ref'][50]['x']) <= inputs[F]['ref'][50]['bound']


def test_frame_counts_outside_the_contract_spoil_their_row_only(lib, bank, inputs):
    mel = _dev(np.stack([inputs[9]['mel']] * 4), torch.float32)
    got = nnls(lib, bank, mel, 5, _frames([-3, 9, 5, 1 << 30]))
    full = nnls(lib, bank, mel[:1], 5)[0]
    assert np.array_equal(got[1], full) and np.array_equal(got[3], full)
    assert np.array_equal(got[2, :5], full[:5]) and not got[2, 5:].any()
    assert np.array_equal(got[0, :4], full[:4]) and not got[0, 4:].any()


# ---------------------------------------------------------------------------------------------- containment
def test_containment(lib, bank, inputs):
    CB, CT, CFR = 3, 9, [9, 4, 6]
    rows = [inputs[9]['mel'][:F] for F in CFR]
    gm = G.inp(_batch(rows, CT), DEV, name='mel')
    gi, gp = G.inp(bank.P, DEV, name='inv_basis'), G.inp(bank.packed, DEV, name='packed')
    gf = G.inp(torch.tensor(CFR, dtype=torch.int32), DEV, name='frames')
    go = G.out((CB, CT, 513), DEV, dtype=torch.float64, name='mag')
    rc = lib.ss_mel_to_linear_nnls(_p(gm.t), _p(gi.t), _p(gp.t), bank.packed.shape[0], _p(gf.t), CB, CT, 80, 50, bank.step, FLOOR, _p(go.t), _s())
    assert rc == 0, lib.ss_last_error()
    torch.cuda.synchronize()
    G.check_all([gm, gi, gp, gf, go])
    got = go.t.cpu().numpy()
    for b, F in enumerate(CFR):
        ref = N.mel_to_linear_nnls(rows[b], bank.B, 50, bank.step, order='band', inv_basis=bank.P)
        assert N.rel_diff(got[b, :F], ref) <= 100.0 * N.DISAGREEMENT_CAP and not got[b, F:].any()


def test_a_corrupt_packed_buffer_stays_inside_mag(lib, bank, inputs):
    """first bins and run lengths far outside the 513 bins and the packed weights, NaN and infinities among them: every index is clamped, so
    the numbers are wrong and nothing else is -- the guard around mag and around every input is untouched"""
    bad = bank.packed.copy()
    bad[0:160:2] = np.resize([-5.0, 1e18, 700.0, NAN, 512.0, -np.inf, 300.5], 80)
    bad[1:160:2] = np.resize([1e18, 600.0, -4.0, 513.0, NAN, np.inf, 941.0], 80)
    rows = [inputs[9]['mel']]
    gm, gi, gp = G.inp(_batch(rows, 9), DEV, name='mel'), G.inp(bank.P, DEV, name='inv_basis'), G.inp(bad, DEV, name='packed')
    go = G.out((1, 9, 513), DEV, dtype=torch.float64, name='mag')
    rc = lib.ss_mel_to_linear_nnls(_p(gm.t), _p(gi.t), _p(gp.t), bad.shape[0], None, 1, 9, 80, 3, bank.step, FLOOR, _p(go.t), _s())
    assert rc == 0, lib.ss_last_error()
    torch.cuda.synchronize()
    G.check_all([gm, gi, gp, go])


# ---------------------------------------------------------------------------------------------- other bases
@pytest.mark.parametrize('which', ['golden', 'every_second', 'forty'])
def test_a_second_basis_with_other_supports(lib, bank, feats, which):
    """features.npz's own 80-band basis (1004 weights, other runs), every second band of the project's (uncovered bins between the bands), and
    40 bands by features.mel_filter_bank's formula"""
    from speechsplit_amd import features
    B = {'golden': lambda: feats['mel_basis'], 'every_second': lambda: bank.B[:, ::2], 'forty': lambda: features.mel_filter_bank(n_mels=40).T}[which]()
    bs = Basis(B)
    mel = R.melspec(feats['u1_wav'][:R.PARITY_SLICES[9]], bs.B).astype(np.float32)
    for it in (1, 50):
        ref, d = N.disagreement(mel, bs.B, it, bs.P, bs.step)
        got = nnls(lib, bs, _dev(mel, torch.float32)[None], it)[0]
        err = N.rel_diff(got, ref)
        print(f'{which} ({bs.n} bands, {bs.packed.shape[0] - 2 * bs.n} weights), n_iter {it}: {err:.3g} (dense vs band {d:.3g})')
        assert d <= N.DISAGREEMENT_CAP and err <= 100.0 * d
    assert np.array_equal(nnls(lib, bs, _dev(mel, torch.float32)[None], 0), pinv_path(lib, bs, _dev(mel, torch.float32)[None]))


# ---------------------------------------------------------------------------------------------- the Python layer, end to end
def test_python_mel_to_linear_nnls(V, lib, bank, inputs):
    mel = inputs[41]['mel']
    got = V.mel_to_linear(mel, inversion='nnls').cpu().numpy()
    assert np.array_equal(got, nnls(lib, bank, _dev(mel, torch.float32)[None], 200)[0])
    assert np.array_equal(V.mel_to_linear(mel, inversion='nnls', nnls_iter=0).cpu().numpy(), V.mel_to_linear(mel).cpu().numpy())
    assert np.array_equal(V.mel_to_linear(mel, bank.B, inversion='nnls', nnls_iter=50).cpu().numpy(), nnls(lib, bank, _dev(mel, torch.float32)[None], 50)[0])


def test_end_to_end_griffin_lim_nnls_agrees_with_numpy(V, bank, inputs, feats):
    """griffin_lim(inversion='nnls') on u1's 41 frames against nnls_ref then griffinlim_ref.griffin_lim, 32 rounds: within the vocoder tests'
    own 41-frame bound (100 x the fft / dft disagreement of Griffin-Lim on u1's 41 frames, capped at 1e-9 of max |x|: 3.7e-10) and within
    their end-to-end bound in mel units (1e-6); and the mel round trip is lower than the pseudo-inverse path's on the same run.  Measured:
    waveform 1.9e-12 (the reference's own fft and dft forms differ by 4.1e-12 on this magnitude), mel 3.0e-8, round trip 0.0142 against
    0.0185"""
    from speechsplit_amd import features
    mel = inputs[41]['mel']
    ph = np.random.default_rng(5).uniform(-np.pi, np.pi, (41, 513))
    mag_ref = inputs[41]['ref'][200]['x']
    div = max(R.rel_diff(R.griffin_lim(mag_ref, 32, 0.99, ph, 'dft'), R.griffin_lim(mag_ref, 32, 0.99, ph, 'fft')), 0.0)
    wav = V.griffin_lim(mel, n_iter=32, generator=np.random.default_rng(5), inversion='nnls')
    ref = R.griffin_lim(mag_ref, 32, 0.99, ph)
    d = R.rel_diff(wav, ref)
    assert wav.dtype == np.float64 and wav.shape == (256 * 40,)
    got_mel = features.melspectrogram(wav, bank.B).cpu().numpy()
    dmel = float(np.abs(got_mel - R.melspec(ref, bank.B)).max())
    trip = float(np.abs(got_mel - mel).mean())
    wav0 = V.griffin_lim(mel, n_iter=32, generator=np.random.default_rng(5))
    trip0 = float(np.abs(features.melspectrogram(wav0, bank.B).cpu().numpy() - mel).mean())
    print(f'end to end: waveform {d:.3g} of max |x| (the reference\'s own fft vs dft on this magnitude: {div:.3g}), mel {dmel:.3g}; '
          f'mel round trip {trip:.4f} against the pseudo-inverse path\'s {trip0:.4f}')
    S41, ph41 = R.parity_input(feats['u1_wav'], 41)                       # test_gpu_vocoder.py's own 41-frame bound, as it computes it
    bound = min(1e-9, 100.0 * R.divergence(S41, ph41))
    print(f'bounds: waveform {bound:.3g} of max |x|, mel 1e-6')
    assert d <= bound
    assert got_mel.shape == (41, 80) and dmel <= 1e-6                     # and its end-to-end test's, in mel units
    assert trip < trip0
    # batching does not change a row: the list form, ragged, two rows a batch
    mels = [inputs[F]['mel'] for F in (9, 41, 5)]
    runs = [V.griffin_lim(mels, n_iter=2, generator=np.random.default_rng(2), max_rows=r, inversion='nnls', nnls_iter=50) for r in (1, 2)]
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
