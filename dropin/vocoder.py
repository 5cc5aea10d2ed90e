"""Mel spectrograms to waveforms (Griffin-Lim) on the MI355X: see speechsplit_amd/vocoder.py."""
from speechsplit_amd.vocoder import *  # noqa: F401,F403
from speechsplit_amd.vocoder import griffin_lim, mel_to_linear, save_wav  # noqa: F401,E402
