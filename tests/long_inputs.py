"""Utterance-length inputs for the audio kernels, shared by test_gpu_long_audio.py (GPU) and test_long_inputs_selftest.py (CPU), and numpy
emulations of the mistakes these inputs are there to catch.  Host only; every array is computed once and handed out read-only.

The per-kernel test files feed the two fixture recordings (12 345 and 10 241 samples: 49 and 41 frames) and cuts of them, so every kernel
that walks a row in fixed-size chunks runs its first chunk and nothing else.  These inputs are the shortest that make the second one run:

    long16      u0_wav, u1_wav, u1_wav reversed, u0_wav reversed: 45 172 samples at 16 kHz, 177 frames of 256.  Real speech, so the pitch
                decisions have margins to spare (asserted by the self-test); its track has a voiced run across frame 64 and one that starts
                at frame 128.
    long16_x    u0_x, u1_x and their reversals: 45 170 samples before the filter, N = 45 206 steps a pass, 177 blocks of 256.
    long10      silence_ref.speech_signal, its reversal x 0.5 and itself x 0.25 (139 755 samples at 16 kHz) brought to 10 kHz by scipy's
                resample_poly: 87 347 samples, 681 STOI frames -- three chunks of 256 with frames dropped in each.  The pairs are
                stoi_ref.make_pair of its cuts at 256, 257, 258 and 681 frames, and of two cuts of 257 and 258 frames whose last one
                and two frames are kept.
    u_tracks    crafted F0 tracks of 63 .. 1000 frames for the harmonic phase recurrence, with resets on either side of the 64-frame edge.
    FILTER_N    row lengths whose N = n + 36 ends a 256-step block after 255, 256, 1, 7, 8 and 9 steps.

The wrong variants at the end are what the self-test holds these inputs against: each must change the result on an input above and leave
every input of the per-kernel files alone."""
import functools
import os

import numpy as np
from scipy import signal

from tests import filtfilt_ref as FR
from tests import harmonic_ref as H
from tests import pitch_ref as P
from tests import silence_ref
from tests import stoi_ref as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
M_RANGE, W_RANGE = (50.0, 250.0), (100.0, 600.0)
SCALE = 32768.0


def _ro(a):
    a = np.ascontiguousarray(a, np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def feats():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------- 16 kHz: pitch, mel, vocoder, harmonic
LONG16_SAMPLES, LONG16_FRAMES = 45172, 177
LONG16_UNVOICED = (0, 1, 49, 127, 175, 176)                            # pitch_ref.track(long16, 50, 250): runs of 47, 77 and 47 between them
PITCH_RAGGED = (45172, 513, 16400, 30000)                              # the rows of the ragged pitch batch: cuts of long16


@functools.lru_cache(maxsize=None)
def long16():
    f = feats()
    u0, u1 = np.asarray(f['u0_wav'], np.float64), np.asarray(f['u1_wav'], np.float64)
    x = _ro(np.concatenate((u0, u1, u1[::-1], u0[::-1])))
    assert x.shape == (LONG16_SAMPLES,) and x.shape[0] // 256 + 1 == LONG16_FRAMES
    return x


@functools.lru_cache(maxsize=None)
def long16_track():
    """pitch_ref.track(long16, 50, 250) in Hz, 0 on unvoiced frames: the F0 the harmonic tests run on"""
    return _ro(H.to_hz(P.track(long16(), *M_RANGE)))


@functools.lru_cache(maxsize=None)
def long16_mel():
    from tests import griffinlim_ref as GL
    mel = GL.melspec(long16(), np.asarray(feats()['mel_basis'], np.float64)).astype(np.float32)
    assert mel.shape == (LONG16_FRAMES, 80)
    mel.setflags(write=False)
    return mel


def voiced_runs(v):
    """[(first frame, length)] of the runs of True in v"""
    v = np.concatenate(([False], np.asarray(v, bool), [False]))
    edges = np.flatnonzero(v[1:] != v[:-1])
    return [(int(a), int(b - a)) for a, b in zip(edges[::2], edges[1::2])]


# ---------------------------------------------------------------------------------------------- the harmonic phase recurrence
U_FRAMES = (63, 64, 65, 127, 128, 129, 200, 1000)
U_GAPS = (62, 63, 64, 65)
U_KINDS = ('glide',) + tuple(f'gap{g}' for g in U_GAPS) + ('alternating', 'unvoiced')
U_RAGGED = ((64, 'glide'), (65, 'gap64'), (128, 'alternating'), (200, 'gap63'))    # (frames, kind) of the ragged batch, max_frames = 200


def u_track(kind, F):
    """F0 in Hz, [F].  glide: voiced throughout, 110.37 Hz rising by 0.2137 Hz a frame (324 Hz at frame 1000), so u never repeats and the
    carry crosses every 64-frame edge; gapG: the glide with frame G unvoiced, which resets u at G and G + 1 (a gap at or beyond F leaves
    the glide); alternating: every other frame unvoiced, so every voiced frame restarts at 0; unvoiced: values outside the voiced range."""
    i = np.arange(F, dtype=np.float64)
    hz = 110.37 + 0.2137 * i
    if kind.startswith('gap'):
        g = int(kind[3:])
        if g < F:
            hz[g] = 0.0
    elif kind == 'alternating':
        hz[::2] = 0.0
    elif kind == 'unvoiced':
        hz = np.resize([0.0, 39.9, 1000.1, -1.0, np.nan, np.inf], F)
    else:
        assert kind == 'glide', kind
    return hz


# ---------------------------------------------------------------------------------------------- the filter
FILTER_N = (731, 732, 733, 739, 740, 741, 988)                          # N = n + 36: 767, 768, 769, 775, 776, 777, 1024
FILTER_LAST_BLOCK = (255, 256, 1, 7, 8, 9, 256)                         # steps in each one's last block of 256
LONG16_X_SAMPLES = 45170


@functools.lru_cache(maxsize=None)
def long16_x():
    f = feats()
    u0, u1 = np.asarray(f['u0_x'], np.float64), np.asarray(f['u1_x'], np.float64)
    x = _ro(np.concatenate((u0, u1, u1[::-1], u0[::-1])))
    assert x.shape == (LONG16_X_SAMPLES,) and -(-(x.shape[0] + 36) // 256) == 177
    return x


@functools.lru_cache(maxsize=None)
def filter_rows():
    """name -> samples: long16_x cut to every length of FILTER_N (from sample 12 000 on, inside u0_x's speech), and the whole of it"""
    x = long16_x()
    rows = {str(n): _ro(x[12000:12000 + n]) for n in FILTER_N}
    rows['long'] = x
    return rows


@functools.lru_cache(maxsize=None)
def filter_draws(name):
    """the dither draw of a row: numpy's legacy generator, one seed a row"""
    names = list(filter_rows())
    return _ro(np.random.RandomState(300 + names.index(name)).rand(filter_rows()[name].shape[0]))


# ---------------------------------------------------------------------------------------------- 10 kHz: STOI
LONG10_SAMPLES = 87347
# name -> (first sample, samples).  The cuts from sample 0 end in long10's noise: frames 256 and 257 of f257 / f258 are dropped, so their
# second chunk runs and writes nothing.  k257 / k258 start 6000 samples in, where those frames are speech: the second chunk keeps 1 and 2.
STOI_CUTS = {'f256': (0, 32896), 'f257': (0, 33024), 'f258': (0, 33152), 'whole': (0, LONG10_SAMPLES), 'k257': (6000, 33024),
             'k258': (6000, 33152)}
STOI_FKS = {'f256': (256, 100, 70), 'f257': (257, 101, 71), 'f258': (258, 102, 72), 'whole': (681, 236, 206), 'k257': (257, 119, 89),
            'k258': (258, 122, 92)}                                     # frames, kept, segments
STOI_KEPT = {'f256': [100], 'f257': [101, 0], 'f258': [102, 0], 'whole': None, 'k257': [118, 1], 'k258': [120, 2]}   # kept a chunk of 256
STOI_PAIR_SEED = 5
MANY_ROWS, MANY_CUT, MANY_STRIDE = 72, 4096, 256
MANY_SHORT = {5: 3968, 40: 256}                                         # row -> samples: 30 frames (no segment) and one frame


@functools.lru_cache(maxsize=None)
def long10():
    s = silence_ref.speech_signal(feats())
    x16 = np.concatenate((s, 0.5 * s[::-1], 0.25 * s))
    assert x16.shape == (139755,)
    x = _ro(signal.resample_poly(x16, 5, 8))
    assert x.shape == (LONG10_SAMPLES,)
    return x


@functools.lru_cache(maxsize=None)
def stoi_pairs():
    """name -> (x, y) at 10 kHz: stoi_ref.make_pair of the cut of long10 that STOI_CUTS[name] names"""
    out = {}
    for name, (first, cut) in STOI_CUTS.items():
        x, y = SR.make_pair(long10()[first:first + cut], STOI_PAIR_SEED)
        out[name] = (_ro(x), _ro(y))
    return out


@functools.lru_cache(maxsize=None)
def stoi_many_rows():
    """[(x, y)] x MANY_ROWS: 4096-sample cuts (31 frames) of the whole pair at the first offsets, MANY_STRIDE apart, at which the mask
    keeps all 31 frames -- one segment each -- with the two short rows of MANY_SHORT among the first 64"""
    x, y = stoi_pairs()['whole']
    rows, off = [], 0
    while len(rows) < MANY_ROWS:
        short = MANY_SHORT.get(len(rows))
        if short is not None:
            rows.append((_ro(x[:short]), _ro(y[:short])))
            continue
        assert off + MANY_CUT <= x.shape[0], 'long10 has too few stretches that keep every frame'
        cx = x[off:off + MANY_CUT]
        if SR.keep_mask(SR.energies(cx)).all() and SR.mask_margin(cx) > 1e-6:
            rows.append((_ro(cx), _ro(y[off:off + MANY_CUT])))
        off += MANY_STRIDE
    return rows


# ---------------------------------------------------------------------------------------------- the mistakes these inputs are there for
def u_carry_dropped(f0_hz, chunk=64):
    """harmonic_ref.phase_u with the carry lost at every multiple of `chunk` frames: a frame that opens a chunk chains on 0, not on u[i-1]"""
    import math
    f = [float(x) for x in np.asarray(f0_hz, np.float64)]
    v = H.voiced(f0_hz)
    u = [0.0] * len(f)
    for i in range(1, len(f)):
        if v[i] and v[i - 1]:
            t = (0.0 if i % chunk == 0 else u[i - 1]) + 0.008 * (f[i - 1] + f[i])
            u[i] = t - math.floor(t)
    return np.array(u)


def stoi_map(e, variant=None, chunk=256):
    """(inv [F] with -1 behind the kept frames, K) from the frame levels, as mask_kernel compacts them.  'base_not_carried': every chunk
    of 256 frames writes its kept frames from slot 0 on and K is the last chunk's count.  'second_block_missing': the levels from frame
    256 on are -inf, as if energy_kernel's second block had not run."""
    e = np.array(e, np.float64)
    if variant == 'second_block_missing':
        e[chunk:] = -np.inf
    keep = SR.keep_mask(e)
    inv = np.full(e.shape[0], -1, np.int64)
    base = 0
    for f0 in range(0, e.shape[0], chunk):
        kept = f0 + np.flatnonzero(keep[f0:f0 + chunk])
        if variant == 'base_not_carried':
            base = 0
        inv[base:base + kept.size] = kept
        base += kept.size
    inv[base:] = -1                                                      # the kernel's closing fill, from ITS count on
    return inv, base


def pitch_fill(F, max_frames, variant=None, lanes=64):
    """which frames of a row of max_frames dp_kernel's fill writes (True): F .. max_frames - 1; 'one_trip': the loop makes one trip of 64"""
    done = np.zeros(max_frames, bool)
    done[F:(min(F + lanes, max_frames) if variant == 'one_trip' else max_frames)] = True
    return done


FILTER_WRONG = ('single_step_lost', 'restart_at_closing_edge', 'restart_at_every_edge', 'short_tail_skipped')


def filtfilt_blocks(x, variant=None, block=256, group=8):
    """filtfilt_ref.filtfilt (gain 1, no dither) with each pass run in blocks of 256 steps as filtfilt_kernel runs it, and ONE mistake:

        single_step_lost          a last block of exactly one step is not run (N = 1 mod 256); its output stays 0
        restart_at_closing_edge   where a pass ends exactly on a block edge (N = 0 mod 256) the last block starts from zi x its first
                                  sample instead of the carried state
        restart_at_every_edge     every block starts that way: the per-kernel file's inputs (3 to 49 blocks) already tell this one
        short_tail_skipped        a last block of fewer than 8 steps (one read-ahead group) is not run; its outputs stay 0
    variant None is the restatement to the bit."""
    assert variant is None or variant in FILTER_WRONG
    b, a, zi = FR.coefficients()
    zi = [float(s) for s in zi]
    ext = FR.extend(np.asarray(x, np.float64))
    N = len(ext)

    def one_pass(u):
        z = [s * u[0] for s in zi]
        out = []
        for j0 in range(0, N, block):
            blk = u[j0:j0 + block]
            last = j0 + block >= N
            if last and ((variant == 'single_step_lost' and len(blk) == 1) or (variant == 'short_tail_skipped' and len(blk) < group)):
                out += [0.0] * len(blk)
                continue
            if j0 > 0 and (variant == 'restart_at_every_edge' or (variant == 'restart_at_closing_edge' and last and len(blk) == block)):
                z = [s * blk[0] for s in zi]
            out += FR.run(blk, b, a, z)
        return out

    v = one_pass(ext)
    w = one_pass(v[::-1])[::-1]
    return np.array(w[FR.PAD:FR.PAD + len(x)], np.float64)
