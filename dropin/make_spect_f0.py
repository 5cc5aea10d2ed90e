"""Recordings to (mel, normalised F0) files on the MI355X, the reference's make_spect_f0.py: see speechsplit_amd/features.py."""
from speechsplit_amd.features import make_spect_f0, make_spect_f0_batched  # noqa: F401  (the batched walk: max_rows, device_draws)

if __name__ == '__main__':
    for speaker, name in make_spect_f0('assets/wavs', 'assets/spmel', 'assets/raptf0', 'assets/spk2gen.pkl'):
        print(speaker, name)
