"""Recordings to (mel, normalised F0) files on the MI355X, the reference's make_spect_f0.py: see speechsplit_amd/features.py.
`python make_spect_f0.py --stationarity` tracks the pitch with RAPT's spectral-stationarity term (off by default)."""
import sys

from speechsplit_amd.features import make_spect_f0, make_spect_f0_batched, make_spect_f0_opt  # noqa: F401  (max_rows, device_draws, stationarity)

if __name__ == '__main__':
    where = ('assets/wavs', 'assets/spmel', 'assets/raptf0', 'assets/spk2gen.pkl')
    walk = make_spect_f0_opt(*where, stationarity=True) if sys.argv[1:] == ['--stationarity'] else make_spect_f0(*where)
    for speaker, name in walk:
        print(speaker, name)
