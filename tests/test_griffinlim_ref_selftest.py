"""The numpy restatement of the vocoder (griffinlim_ref.py) checked against itself, against the reference project's own feature fixture,
and on wrong stand-ins.  CPU only.

What is deliberately NOT asserted: a monotone decrease of the spectral error (with reflect padding and trimmed edges it is no theorem; the
4-frame input violates it around iteration 30) and the mel round trip (a quality figure, recorded in DESIGN.md, not a bar).

Measured when this was written (numpy 'fft' against 'dft', 32 iterations, relative to max |x|, worst of zero / seeded phases and momentum
0 / 0.99): 4 frames 1.3e-13, 5 frames 6.8e-13, 9 frames 1.7e-12, 41 frames 3.7e-12; round trip istft(stft(x)) 1.1e-15 / 2.2e-15."""
import os

import numpy as np
import pytest

from tests import griffinlim_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def feats():
    return np.load(os.path.join(GOLD, 'features.npz'))


@pytest.mark.parametrize('transform', ['fft', 'dft'])
@pytest.mark.parametrize('F', [4, 5, 9])
def test_istft_inverts_stft(F, transform):
    x = np.random.default_rng(F).standard_normal(256 * (F - 1))
    spec = R.stft(x, transform)
    assert spec.shape == (F, 513) and R.frames_of(x.shape[0]) == F
    err = float(np.abs(R.istft(spec, transform) - x).max())
    print(f'istft(stft(x)) - x, {F} frames, {transform}: {err:.3g}')
    assert err <= 1e-13


def test_edge_normaliser_is_what_the_kernel_documents():
    w2 = R.WINDOW ** 2
    norm = np.zeros(256 * 8 + 1024)
    for f in range(9):
        norm[256 * f:256 * f + 1024] += w2
    kept = norm[512:512 + 256 * 8]
    assert abs(kept.min() - 1.25) < 1e-15 and abs(kept[1024] - 1.5) < 1e-15 and abs(kept.max() - 1.5) < 1e-15


@pytest.mark.parametrize('transform', ['fft', 'dft'])
@pytest.mark.parametrize('u', [0, 1])
def test_stft_magnitudes_reproduce_the_feature_fixture(feats, u, transform):
    """features.npz's u*_S came from the reference's own pySTFT and dB scaling: the restatement's framing, window and transform are theirs"""
    S = R.melspec(feats[f'u{u}_wav'], feats['mel_basis'], transform).astype(np.float32)
    assert S.shape == feats[f'u{u}_S'].shape
    assert float(np.abs(S - feats[f'u{u}_S']).max()) <= 2.4e-7        # two float32 units at 1.1


@pytest.mark.parametrize('F', [4, 5, 9, 41])
def test_conditioning_fft_against_dft(feats, F):
    """The condition that lets the GPU bound be tight: two transforms that share no code stay within 1e-10 of max |x| after 32 rounds"""
    S, ph = R.parity_input(feats['u1_wav'], F)
    for p, pname in ((None, 'zero'), (ph, 'seeded')):
        for m in R.MOMENTA:
            a, b = R.griffin_lim(S, 32, m, p, 'fft'), R.griffin_lim(S, 32, m, p, 'dft')
            d = R.rel_diff(b, a)
            print(f'{F} frames, {pname} phases, momentum {m}: fft vs dft {d:.3g}, max|x| {np.abs(a).max():.3g}')
            assert a.shape == (256 * (F - 1),) and np.isfinite(a).all()
            assert d <= R.DIVERGENCE_CAP
    assert R.divergence(S, ph) <= R.DIVERGENCE_CAP


def test_zero_iterations_is_one_istft(feats):
    S, ph = R.parity_input(feats['u1_wav'], 5)
    assert np.array_equal(R.griffin_lim(S, 0, 0.99, ph), R.istft(S * np.exp(1j * ph)))
    assert np.array_equal(R.griffin_lim(S, 0, 0.0, None), R.istft(S.astype(np.complex128)))


@pytest.mark.parametrize('variant', R.WRONG)
def test_wrong_variants_are_reported_at_the_small_shapes(feats, variant):
    """every fault a vocoder kernel could plausibly have moves the 4- or the 9-frame result by far more than any bound in use"""
    worst = 0.0
    for F in (4, 9):
        S, ph = R.parity_input(feats['u1_wav'], F)
        worst = max(worst, R.rel_diff(R.griffin_lim(S, 32, 0.99, ph, variant=variant), R.griffin_lim(S, 32, 0.99, ph)))
    print(f'{variant}: {worst:.3g}')
    assert worst > 1e-6


def test_mel_to_linear_inverts_the_db_scale(feats):
    """with an exactly invertible square 'basis' the step undoes melspec's last two lines; the floor is applied"""
    rng = np.random.default_rng(3)
    amp = rng.uniform(1e-4, 1.0, (6, 513))
    mel = (20.0 * np.log10(amp) - 16.0 + 100.0) / 100.0
    got = R.mel_to_linear(mel, np.eye(513), floor=0.0)
    assert R.rel_diff(got, amp) <= 1e-13
    assert R.mel_to_linear(mel, -np.eye(513), floor=1e-3).min() == 1e-3
