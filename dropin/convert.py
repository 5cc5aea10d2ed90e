"""The conversion step of the reference's demo.ipynb (cell 0) on the MI355X engine: see speechsplit_amd/convert.py."""
from speechsplit_amd.convert import *  # noqa: F401,F403
from speechsplit_amd.convert import CONDITIONS, adapt_speaker, conversion_waveforms, convert_batch, convert_f0, convert_speakers, demo_conversion, demo_conversion_codes, plan_batches  # noqa: F401,E402
