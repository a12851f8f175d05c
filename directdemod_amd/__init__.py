"""
directdemod_amd -- MI355X-native (gfx950, HIP) implementation of DirectDemod's
per-sample hot path behind the reference's own class surface.

Drop-in modules (same names, signatures and error behaviour as the reference's
``directdemod`` package):

    comm.commSignal   filters.*   demod_fm.demod_fm   demod_am.demod_am
    chunker.chunker   constants   source (IQwav/IQdat readers + device ingest)

All arithmetic runs in hand-written HIP kernels reached through the C-ABI
library ``libdirectdemod_hip.so`` (include/directdemod_hip.h) via ctypes.  There
is no CPU fallback: without the library or without a GPU the compute calls raise.
"""
from . import constants  # noqa: F401

# `from directdemod_amd import *` brings in the drop-in modules (imported lazily: nothing here loads the HIP library)
__all__ = ["comm", "filters", "demod_fm", "demod_am", "chunker", "constants", "source", "resample", "afsk", "peakdetect", "decode_afsk1200", "noaa_sync", "decode_noaa", "qpsk", "lrpt", "decode_meteorm2", "decode_lrpt", "oqpsk", "decode_meteorm2x", "fsk", "decode_fsk9600", "sstv", "decode_sstv", "adsb", "decode_adsb", "ais", "decode_ais", "pocsag", "decode_pocsag", "acars", "decode_acars", "rs41", "decode_rs41", "rds", "decode_rds", "fmstereo", "decode_fmstereo", "shard", "stream", "decode_fm", "sink"]
__version__ = "0.1.0"
