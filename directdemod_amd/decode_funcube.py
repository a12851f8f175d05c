"""
Funcube BPSK sync detection -- the reference's decode_funcube surface (decode_funcube.py): `useful`, `getSyncs` and the module
helpers `lim` / `limBin`, plus `getSymbols`, the PLL-corrected soft symbols (gardnerA after pllObj.loop), and beyond the reference
`getFrames` / `frameInfo`: the 256-byte telemetry frames decoded from those symbols (funcube_fec.py).

One decode pass, cached, feeds every property.  Per chunk of the recording (the reference's chunker, no chunker handed to the
signal, so the mixer phase restarts at 0 in every chunk): offsetFreq in the reference's float64 arithmetic (bpsk.mix; with
corrfreq the Doppler ramp of decode_funcube.py:202-226 formed in the kernel, bpsk.mix_ramp, from frequency_shift.dopplerTrack --
computed once per recording -- and dopplerRamp) -> butter(fs, bw) low-pass in scipy.signal.lfilter's own operation order
(bpsk.Lowpass: complex64 in, complex128 out, the state carried from chunk to chunk; bit for bit lfilter's output, which the
package's block-parallel IIR is not near enough to at 7 kHz), then the symbol walk (bpsk.Walker: Gardner timing, agc, costas) and the per-sample lim values.  After the last
chunk: the MINSYNC list on the device, the MAXSYNC buffers on the host and their correlations on the device.  Only counts, the
MINSYNC list, a few sample indices and the argmaxes come down.

Deviations from the reference:
  - no progress / ETA log lines (the MINSYNC, MAXSYNC and "doppler shift is" logging.info lines are kept);
  - with exactly one MAXSYNC the reference raises ValueError (np.min of an empty np.diff); here getSyncs returns [] with useful 0.
"""
import logging
import time

import numpy as np

from . import _hip, bpsk, frequency_shift, funcube_fec, symbolsync
from .bpsk import lim, limBin  # noqa: F401  (module-level helpers, as in the reference)


class decode_funcube(symbolsync.SyncDecoder):
    """Object to decode Funcube: decode_funcube(sigsrc, offset, bw, center_frequency, signal_freq, corrfreq) as in the reference
    (bw None -> 7000).  use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it
    (source.read_device_raw).
    `useful`: 1 if two MAXSYNCs lie 4.98 s +- 0.2 s apart; `getSyncs`: np.int64 positions; `getSymbols`: at 12000 Hz.
    minsyncs: the MINSYNC ctr values; buffers: (intervals, maxBuffStart); ramps: with corrfreq, per chunk (chunk_offset,
    frequency_shift.ramp, doppCorrect_current after it).
    `getFrames`: uint8[n, 256], the telemetry frames of the AO-40 FEC blocks found in the symbols, in stream order; `frameInfo`:
    one funcube_fec.INFO record per frame.  Both are cached and come from the same cached walk as getSyncs, whether or not the
    33-bit sync fired; their stages' times are timings["fc_soft"], ["fc_sync"], ["fc_viterbi"], ["fc_rs"]."""
    WALKER = bpsk.Walker
    STAGES = ("doppler", "mix", "lowpass")
    SPACING = (4.98, 0.2)

    def __init__(self, sigsrc, offset, bw, center_frequency, signal_freq, corrfreq=False, use_device_raw=True):
        super().__init__(sigsrc, use_device_raw)
        self._bw = 7000 if bw is None else bw
        self._offset = offset
        self._center_frequency = int(center_frequency)
        self._signal_freq = int(signal_freq)
        self._corrfreq = corrfreq
        self.ramps = []
        self._frames = None

    @property
    def getFrames(self):
        """The telemetry frames, uint8[n, 256], in stream order: each codeword's bytes corrected where Reed-Solomon decoded it, as
        received where it did not (frameInfo's rs_errors, ok)"""
        return self._decode_frames()[0]

    @property
    def frameInfo(self):
        """Per frame (funcube_fec.INFO): symbol (the first symbol of the frame's first channel bit), sample (the walk's A sample of
        that symbol), inverted, sync_score (of 65), sync_corr, corrected (channel bits the Viterbi decoder changed), rs_errors (bytes
        changed in each of the two codewords, -1: not decodable), ok (both decoded), and sat_id, frame_type from byte 0
        (meaningful when ok)"""
        return self._decode_frames()[1]

    def _decode_frames(self):
        if self._frames is not None:
            return self._frames
        w = self.walker()
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            _hip.sync()
            now = time.perf_counter()
            self.timings["fc_" + name] = now - t0
            t0 = now
        D = funcube_fec.soft_bits(w.view("sym"))
        lap("soft")
        starts = funcube_fec.frame_starts(funcube_fec.sync_candidates(D))
        lap("sync")
        inv = (starts[:, 1] < 0).astype(np.int64)
        blocks, corrected = funcube_fec.viterbi(D, np.stack((starts[:, 0], inv), axis=1))
        lap("viterbi")
        frames, errors = funcube_fec.reed_solomon(blocks)
        lap("rs")
        info = np.zeros(len(starts), dtype=funcube_fec.INFO)
        info["symbol"] = starts[:, 0] + funcube_fec.SYMBOLS_PER_BIT
        info["sample"] = [int(w.aidx.view(int(k), 1).to_host()[0]) for k in info["symbol"]]
        info["inverted"], info["sync_corr"], info["sync_score"] = inv, starts[:, 1], starts[:, 2]
        info["corrected"], info["rs_errors"] = corrected, errors
        info["ok"] = np.all(errors >= 0, axis=1)
        info["sat_id"], info["frame_type"] = frames[:, 0] >> 6, frames[:, 0] & 0x3F
        self._frames = (frames, info)
        return self._frames

    def _front_end(self, src, ck, lap):
        bf = bpsk.Lowpass(src.sampFreq, self._bw)
        track = ramp = None
        self.ramps = ramps = []
        if self._corrfreq and src.length > 0:
            track = frequency_shift.dopplerTrack(src, self._center_frequency, self._signal_freq, 20000)
            ramp = frequency_shift.dopplerRamp(self._offset, src.sampFreq)
            track.shift(0, len(ck.getChunks))             # the one device pass over the recording, timed on its own
            lap("doppler")

        def front(number, a, b, d):
            if track is None:
                mixed = bpsk.mix(d, src.sampFreq, self._offset)
            else:
                chunk_offset = track.shift(number, len(ck.getChunks))
                logging.info("doppler shift is %f Hz", chunk_offset)
                r = ramp.next(chunk_offset, b - a)
                ramps.append((float(chunk_offset), r, float(ramp.current)))
                mixed = bpsk.mix_ramp(d, src.sampFreq, r)
            lap("mix")
            x = bf.apply(mixed)
            lap("lowpass")
            return x
        return front

    def _sync_search(self, w, total, a_at, lap):
        mins = bpsk.minsync_list(w)
        lap("minsync")
        for k, m in mins:
            logging.info("MINSYNC: %d %f", k + 1, abs(m - bpsk.WIN / 2))
        bufs = bpsk.maxsync_buffers(mins[:, 0], total, a_at, w.nsym)
        am = bpsk.maxsync_argmax(w.lim_values, bufs)
        lap("maxsync")
        return [int(k) + 1 for k in mins[:, 0]], bufs, am

    def _position(self, start, arg):
        return start + np.int64(arg)
