"""Recordings to (mel, normalised F0) files on the MI355X, the reference's make_spect_f0.py: see speechsplit_amd/features.py.
`python make_spect_f0.py --stationarity` tracks the pitch with RAPT's spectral-stationarity term (off by default).
`--trim-db DB`, `--trim-hang BLOCKS`, `--trim-edge BLOCKS` and `--max-pause BLOCKS` (any of them) remove silence from every recording first
(features.Silence: the threshold below the loudest 256-sample block, the hangover, the silent blocks kept at either end and the longest
pause left inside; off by default)."""
import argparse

from speechsplit_amd.features import make_spect_f0, make_spect_f0_batched, make_spect_f0_opt  # noqa: F401  (max_rows, device_draws, stationarity, silence)
from speechsplit_amd.features import Silence


def parse(argv=None):
    """the command line -> (stationarity, silence): whether --stationarity was given, and a Silence if any trim flag was (else None)"""
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--stationarity', action='store_true')
    ap.add_argument('--trim-db', type=float, default=None)
    ap.add_argument('--trim-hang', type=int, default=None)
    ap.add_argument('--trim-edge', type=int, default=None)
    ap.add_argument('--max-pause', type=int, default=None)
    a = ap.parse_args(argv)
    trim = {k: v for k, v in (('top_db', a.trim_db), ('hang', a.trim_hang), ('edge', a.trim_edge), ('pause', a.max_pause)) if v is not None}
    return a.stationarity, Silence(**trim) if trim else None


if __name__ == '__main__':
    where = ('assets/wavs', 'assets/spmel', 'assets/raptf0', 'assets/spk2gen.pkl')
    stationarity, silence = parse()
    if silence is not None:
        walk = make_spect_f0_opt(*where, stationarity=stationarity, silence=silence)
    else:
        walk = make_spect_f0_opt(*where, stationarity=True) if stationarity else make_spect_f0(*where)
    for speaker, name in walk:
        print(speaker, name)
