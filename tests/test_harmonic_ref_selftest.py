"""harmonic_ref.py proven before test_gpu_harmonic.py relies on it (CPU only).  Inputs: harmonic_ref.parity_inputs -- features.npz's u1_wav
cut to 4 / 5 / 9 / 41 frames by griffinlim_ref.PARITY_SLICES, and u0_wav (49 frames), mels through features.npz's own basis cast to float32,
F0 from pitch_ref.track(x, 50, 250): the first two frames of both utterances are unvoiced, every later one is voiced (64 .. 175 Hz).

Measured (numpy, float64), dense against kernel order -- S relative to max |S|, share absolute, phase0 as |e^{ia} - e^{ib}|:

    input    n_iter 0: S / share / phase0     1: S / share / phase0           50: S / share / phase0
    u1_4     3.7e-16 / 0 / 0                  1.6e-16 / 2.6e-15 / 8.8e-15     3.4e-16 / 1.6e-15 / 9.5e-9
    u1_5     5.0e-16 / 0 / 0                  1.7e-16 / 5.2e-15 / 1.8e-13     4.5e-16 / 1.7e-14 / 9.3e-9
    u1_9     3.7e-16 / 0 / 0                  4.7e-16 / 6.4e-15 / 6.1e-13     4.6e-16 / 4.7e-15 / 9.3e-9
    u1_41    7.9e-16 / 0 / 0                  3.0e-16 / 6.4e-15 / 1.1e-13     4.2e-16 / 9.5e-14 / 9.3e-9
    u0       6.0e-16 / 0 / 0                  3.1e-16 / 2.6e-14 / 2.1e-13     2.7e-16 / 8.8e-14 / 6.9e-13

S and share are held under 1e-11, as the NNLS self-test holds its own.  phase0 is NOT a sum: it is computed from the share, and the
definition's sqrt(1 - w^2) turns one unit in the last place of a share next to 1 (0.9999999999999999 against 1.0 at frame 2, bin 403 of
u1) into sqrt(2^-52) = 1.5e-8 of the other component and so 9.3e-9 of phase.  That is a property of the definition -- the share reaches
the phase call rounded to a double -- and inaudible; it is recorded here and held under 4 sqrt(2^-52) = 6e-8.  It is why
test_gpu_harmonic.py compares phase0 on one and the same share (test_phase_parity there).

The wrong variants lie between 0.233 (S as a plain sum) and 2 from the definition (the larger of S's relative and the share's absolute
distance; phases as |e^{ia} - e^{ib}|), against a GPU bar that is never above 1e-9.

The claim (50 rounds, the restatement): S's error || S - |stft| || / || |stft| || over the pseudo-inverse route's on the same mel is
0.399 on u0 (0.278 against 0.698) and 0.289 on u1 (0.198 against 0.687); the bar is the midpoint between that and 1: 0.699 and 0.644.

Ground truth: for pitch_ref.tone(120) with its true F0 the fitted a_h, h <= 5, recover the partials' amplitudes 0.2 / h (a sinusoid of
amplitude c has the Hann peak 256 c, and an atom's peak is 512 W(0) = 256) -- see test_tone_amplitudes for the measured error and bound."""
import os

import numpy as np
import pytest

from tests import griffinlim_ref as R
from tests import harmonic_ref as H
from tests import pitch_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GPU_BAR = H.GPU_BOUND_CAP                                               # test_gpu_harmonic.py's bound never exceeds it
FULL = ('u0', 'u1_41')
CLAIM_RATIO = {'u0': 0.399, 'u1_41': 0.289}                             # measured on the restatement at 50 rounds
MEASURED_REL, MEASURED_REST = 3.67e-2, 7.9e-4                           # test_tone_amplitudes, measured on the restatement


@pytest.fixture(scope='module')
def S():
    feats = np.load(os.path.join(GOLD, 'features.npz'))
    B = np.asarray(feats['mel_basis'], np.float64)
    s = dict(feats=feats, B=B, P=np.linalg.pinv(B), inp=H.parity_inputs(feats))
    s['rand'] = {k: np.random.default_rng(7).uniform(-np.pi, np.pi, (v[0].shape[0], 513)) for k, v in s['inp'].items()}
    s['pinv'] = {k: R.mel_to_linear(v[0], s['P']) for k, v in s['inp'].items()}
    s['dense'] = {k: H.mel_to_linear_harmonic(v[0], v[1], B, s['pinv'][k], 50, inv_basis=s['P']) for k, v in s['inp'].items()}
    return s


def test_inputs_hold_the_conditions(S):
    for name, (mel, hz) in S['inp'].items():
        v = H.voiced(hz)
        assert v.any() and not v.all(), name                             # both kinds of frame in every input
        H.conditions(hz)
    assert [S['inp'][k][0].shape[0] for k in ('u1_4', 'u1_5', 'u1_9', 'u1_41', 'u0')] == [4, 5, 9, 41, 49]


def test_two_orders_agree(S):
    for name, (mel, hz) in S['inp'].items():
        for it in H.ITERS:
            _, (ds, dw, dp) = H.disagreement(mel, hz, S['B'], S['P'], S['rand'][name], it)
            print(f'{name}, n_iter {it}: dense vs kernel order S {ds:.3g} of max |S|, share {dw:.3g}, phase0 {dp:.3g}')
            assert ds <= H.DISAGREEMENT_CAP and dw <= H.DISAGREEMENT_CAP
            assert dp <= 4.0 * np.sqrt(H.EPS)                            # see the module docstring: one ulp of a share next to 1
    assert H.DISAGREEMENT_CAP <= 1e-11


def test_step_bound_holds_on_every_voiced_frame(S):
    worst = (np.inf, 0.0)
    for name, (mel, hz) in S['inp'].items():
        for f in hz[H.voiced(hz)]:
            A = S['B'].T @ H.dictionary(f)
            assert (A >= 0.0).all()
            lam = float(np.linalg.eigvalsh(A.T @ A)[-1])
            ratio = H.lipschitz(A) / lam
            worst = (min(worst[0], ratio), max(worst[1], ratio))
            assert ratio >= 1.0, (name, f)
    print(f'L / lambda_max over all voiced frames: {worst[0]:.4f} .. {worst[1]:.4f}')


def test_atoms_are_the_hann_lobe(S):
    """against the closed form away from its cancellation, and against the transform of a windowed cosine itself"""
    d = np.array([-1.9, -1.5, -0.5, -0.25, 0.3, 0.5, 1.5, 1.75])
    closed = np.sin(np.pi * d) / (2.0 * np.pi * d * (1.0 - d * d))
    assert np.abs(H.lobe(d) - closed).max() <= 1e-15
    assert H.lobe(0.0) == 0.5 and abs(H.lobe(1.0) - 0.25) <= 1e-16 and H.lobe(2.0) == 0.0 and H.lobe(-2.5) == 0.0
    f = 130.3
    spec = np.abs(np.fft.rfft(R.WINDOW * np.cos(2.0 * np.pi * f * (np.arange(1024) - 512) / 16000.0)))
    D = H.dictionary(f, 7600.0)[:, 0]
    near = np.flatnonzero(D)
    assert near.size == 4 and np.abs(spec[near] - D[near]).max() <= 2e-3 * 256.0   # the negative-frequency lobe's tail is all that differs


def test_unvoiced_frames_keep_the_route_and_zero_rounds_are_the_pseudo_inverse(S):
    mel, hz = S['inp']['u1_9']
    for order in ('dense', 'kernel'):
        none = np.array([np.nan, 0.0, 39.9, 1000.1, -1.0, np.inf, -np.inf, 1e300, 0.0])
        mag, share = H.mel_to_linear_harmonic(mel, none, S['B'], S['pinv']['u1_9'], 50, order=order, inv_basis=S['P'])
        assert np.array_equal(mag, S['pinv']['u1_9']) and not share.any()
        mag, share = H.mel_to_linear_harmonic(mel, hz, S['B'], np.full((9, 513), 7.0), 0, order=order, inv_basis=S['P'])
        v = H.voiced(hz)
        assert (mag[~v] == 7.0).all() and not share.any()
        assert H.rel_diff(mag[v], S['pinv']['u1_9'][v]) <= 1e-14         # a = 0: the noise part alone is the floored pseudo-inverse
    ph = H.harmonic_phase(none, np.zeros((9, 513)), S['rand']['u1_9'])
    assert np.array_equal(ph, S['rand']['u1_9'])


def test_every_wrong_variant_is_reported(S):
    smallest = np.inf
    for name in FULL:
        mel, hz = S['inp'][name]
        ref_S, ref_w = S['dense'][name]
        ref_p = H.harmonic_phase(hz, ref_w, S['rand'][name])
        for v in H.WRONG_FIT:
            got_S, got_w = H.mel_to_linear_harmonic(mel, hz, S['B'], S['pinv'][name], 50, inv_basis=S['P'], variant=v)
            d = max(H.rel_diff(got_S, ref_S), H.abs_diff(got_w, ref_w))
            print(f'{name}, {v}: {d:.3g}')
            smallest = min(smallest, d)
        for v in (p for p in H.WRONG_PHASE if p != 'no_restart'):         # that one: below
            d = H.phase_diff(H.harmonic_phase(hz, ref_w, S['rand'][name], variant=v), ref_p)
            print(f'{name}, {v}: {d:.3g}')
            smallest = min(smallest, d)
    print(f'smallest distance {smallest:.3g}')
    assert smallest >= 100.0 * GPU_BAR
    # no_restart needs a voiced frame right after an unvoiced one that follows voiced ones: the full inputs have none, so a gap is cut in
    mel, hz = S['inp']['u1_41']
    gap = hz.copy()
    gap[20] = 0.0
    w = S['dense']['u1_41'][1]
    assert np.array_equal(H.phase_u(hz, 'no_restart'), H.phase_u(hz))
    d = H.phase_diff(H.harmonic_phase(gap, w, S['rand']['u1_41'], variant='no_restart'), H.harmonic_phase(gap, w, S['rand']['u1_41']))
    print(f'u1_41 with frame 20 unvoiced, no_restart: {d:.3g}')
    assert d >= 100.0 * GPU_BAR and H.phase_u(gap)[21] == 0.0 and H.phase_u(gap)[22] > 0.0


def test_the_claim_on_the_restatement(S):
    for name, key in (('u0', 'u0_wav'), ('u1_41', 'u1_wav')):
        true = np.abs(R.stft(np.asarray(S['feats'][key], np.float64)))
        err = lambda a: float(np.linalg.norm(a - true) / np.linalg.norm(true))
        e_h, e_p = err(S['dense'][name][0]), err(S['pinv'][name])
        ratio = e_h / e_p
        bar = (CLAIM_RATIO[name] + 1.0) / 2.0
        print(f'{name}: harmonic {e_h:.4f} against the pseudo-inverse route\'s {e_p:.4f}: ratio {ratio:.4f}, bar {bar:.4f}')
        assert abs(ratio - CLAIM_RATIO[name]) <= 2e-3                    # the recorded value is the measured one
        assert ratio <= bar


def test_tone_amplitudes(S):
    """pitch_ref.tone(120): partials 0.2 / h sin(2 pi 120 h t), h <= 5.  A partial of amplitude c has the Hann peak 256 c, an atom the
    peak 512 W(0) = 256: a_h = 0.2 / h.  Interior frames, 50 rounds.  MEASURED_REL is the largest |a_h / (0.2 / h) - 1| over h <= 5 and
    all interior frames (what the mel's 80 bands, its float32 cast and 50 rounds leave), MEASURED_REST the largest harmonic above 5 over
    a_1; each is bounded with a margin of 2."""
    x = pitch_ref.tone(120.0)
    mel = R.melspec(x, S['B']).astype(np.float32)
    hz = np.full(mel.shape[0], 120.0)
    _, _, amps = H.mel_to_linear_harmonic(mel, hz, S['B'], R.mel_to_linear(mel, S['P']), 50, inv_basis=S['P'], return_a=True)
    a = np.stack(amps)[4:-4]                                             # frames clear of the reflect padding
    assert a.shape[1] == 63
    rel = np.abs(a[:, :5] / (0.2 / np.arange(1, 6)) - 1.0).max()
    rest = a[:, 5:].max() / a[:, 0].min()
    print(f'tone(120): a_h against 0.2 / h, h <= 5: worst relative error {rel:.3g}; harmonics above 5 at most {rest:.3g} of a_1')
    assert rel <= 2.0 * MEASURED_REL
    assert rest <= 2.0 * MEASURED_REST
