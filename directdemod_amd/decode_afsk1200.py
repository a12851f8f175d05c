"""
AFSK1200 (APRS) decoding -- the reference's decode_afsk1200 surface (decode_afsk1200.py): `useful`, `getMsg` and the static
helpers, plus `getFrames`, which returns the accepted frames' fields instead of printing them.

Every stage runs on the device and hands device arrays to the next: the fused offsetFreq -> blackmanHarris(151) -> bwLim chain per
chunk, demod_fm over the whole signal, the Butterworth band-pass, the correlators (afsk.binary_filter, afsk.bit_edges), |changes|,
the lookahead peak pick (dd_peakdetect_f64), the bit slicer (dd_afsk_bits_f64) and the frame check (dd_afsk_frames_check / _pack).
Only counts, flag positions and the accepted frames' bytes come down.

Deviations from the reference:
  - nothing is printed; getFrames holds the fields, and a logging.info line is written per frame;
  - a CRC-valid frame with fewer than two bytes after its address field gets control = pid = None and info = "" (the reference
    raises IndexError);
  - the result is cached even when it is None (the reference decodes again on every getMsg that found nothing).
"""
import logging
import time

import numpy as np

from . import _hip, afsk, chunker, comm, constants, demod_fm, filters

MSG = "template: space rocks!"          # what the reference's getMsg returns when a frame passed (:262)
FLAG = (0, 1, 1, 1, 1, 1, 1, 0)


def fcs_crc16(data_stream):
    """framechecksequence.fcs_crc16: CRC-16 (reflected 0x8408, init and xorout 0xFFFF) of a '0'/'1' string, as 16 characters LSB first"""
    fcs = 0xFFFF
    for bit in data_stream:
        shift = fcs & 1
        fcs >>= 1
        if str(shift) != bit:
            fcs ^= 0x8408
    fcs ^= 0xFFFF
    return bin(fcs)[2:].zfill(16)[::-1]


def _fields(raw):
    """bits_to_msg's split of the message bytes: (destination, source, path, control, pid, info); address characters are byte >> 1
    up to and including the first byte with its low bit set"""
    header, rest = [], b""
    for k, byte in enumerate(raw):
        header.append(chr(byte >> 1))
        if byte & 1:
            rest = raw[k + 1:]
            break
    h = "".join(header)
    control = hex(rest[0]) if len(rest) >= 2 else None
    pid = hex(rest[1]) if len(rest) >= 2 else None
    info = rest[2:].decode("latin-1") if len(rest) >= 2 else ""
    return h[:7], h[7:14], h[14:], control, pid, info


class decode_afsk1200:
    """Object to decode AFSK1200: decode_afsk1200(sigsrc, offset, bw) as in the reference (bw None -> 22050).
    use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it (source.read_device_raw)."""

    BAUDRATE = 1200
    MARK_FREQUENCY = 1200
    SPACE_FREQUENCY = 2200

    def __init__(self, sigsrc, offset, bw=None, use_device_raw=True):
        self.__bw = 22050 if bw is None else bw
        self.__sigsrc = sigsrc
        self.__offset = offset
        self.__use_raw = use_device_raw
        self.__done = False
        self.__msg = None
        self.__useful = 0
        self.__frames = []
        self.timings = {}                  # seconds per stage of the last decode (front end, band-pass, correlators, peaks, bits, frames)

    @property
    def useful(self):
        """1 if at least one frame with a correct CRC was found, else 0"""
        return self.__useful

    @property
    def getMsg(self):
        """"template: space rocks!" when a frame passed its CRC, else None (the reference's return value)"""
        self._decode()
        return self.__msg

    @property
    def getFrames(self):
        """The accepted frames in stream order, one dict each: flag (index of its start flag), start (bit of that flag), nbytes
        (the frame's length in bytes with its FCS, as the reference prints it), destination, source, path, control, pid
        (hex strings or None), info (str, one character per byte) and raw (the message bytes without FCS)"""
        self._decode()
        return list(self.__frames)

    # ------------------------------------------------------------------ the device pipeline
    def _baseband(self, taps=151):
        """decode_afsk1200.py:67-90: chunk loop offsetFreq -> blackmanHarris(151) -> bwLim(bw) -> extend (decode_ais asks for a
        shorter window at low sample rates)"""
        src = self.__sigsrc
        sig = comm.commSignal(src.sampFreq)
        ck = chunker.chunker(src)
        bh = filters.blackmanHarris(taps)
        read = src.read
        if self.__use_raw and hasattr(src, "read_device_raw") and src.read_device_raw(0, 1) is not None:
            read = src.read_device_raw
        for a, b in ck.getChunks:
            c = comm.commSignal(src.sampFreq, read(a, b), ck)
            c.offsetFreq(self.__offset)
            c.filter(bh)
            c.bwLim(self.__bw)
            sig.extend(c)
        return sig

    def _audio(self):
        """decode_afsk1200.py:67-94: the chunk loop, then demod_fm over the whole"""
        sig = self._baseband()
        sig.funcApply(demod_fm.demod_fm().demod)
        return sig

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        t = {}
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            _hip.sync()
            now = time.perf_counter()
            t[name] = now - t0
            t0 = now
        sig = self._audio()
        sig.device_signal
        lap("front_end")
        sig.filter(filters.butter(sig.sampRate, 1200 - 500, 2200 + 500, typeFlt=constants.FLT_BP))
        audio = comm._convert(sig.device_signal, np.float64)
        lap("bandpass")
        bw = self.__bw
        spb = bw // self.BAUDRATE
        bf = afsk.binary_filter(audio, bw)
        changes = afsk.bit_edges(bf, spb)
        mag = _hip.DevArray(changes.n, np.float64)
        _hip.check(_hip.lib().dd_abs_f64(changes.ptr, 0, mag.ptr, changes.n, None), "dd_abs_f64")
        lap("correlators")
        (px, _), _ = afsk.peak_lists(mag, int(spb * 0.65))
        lap("peaks")
        bs = afsk.bit_stream(bf, px, bw)
        lap("bits")
        info, raws = afsk.frames(bs)
        flags = bs.flags.to_host() if len(raws) else None
        lap("frames")
        self.timings = t
        frames = []
        acc = np.nonzero(info[:, 1] == 1)[0] if len(info) else []
        for f, raw in zip(acc, raws):
            dst, src, path, control, pid, text = _fields(raw)
            rec = {"flag": int(f), "start": int(flags[f]), "nbytes": int(info[f, 0]) // 8, "destination": dst, "source": src,
                   "path": path, "control": control, "pid": pid, "info": text, "raw": raw}
            logging.info("AFSK1200 frame #%d at bit %d, %d bytes: %s > %s %s: %s", rec["flag"], rec["start"], rec["nbytes"],
                         src, dst, path, text)
            frames.append(rec)
        self.__frames = frames
        if frames:
            self.__msg = MSG
            self.__useful = 1
        self.__done = True

    # ------------------------------------------------------------------ the reference's static helpers (host NumPy)
    @staticmethod
    def decode_nrzi(nrzi):
        """:279-301: element 0 is 1; element k is 1 where nrzi[k-1] == nrzi[k], else 0 (also [1] for an empty input)"""
        nrzi = np.asarray(nrzi)
        out = [1]
        if nrzi.size > 1:
            out += (nrzi[:-1] == nrzi[1:]).astype(int).tolist()
        return out

    @staticmethod
    def find_bit_stuffing(code_bit):
        """:303-333: bit k is marked 1 (bit is 0) or 2 (bit is 1) when the run of ones just before it is exactly 5 long"""
        b = np.asarray(code_bit, dtype=np.int64)
        out = np.zeros(len(b), dtype=np.int64)
        counter = 0
        for k in range(len(b)):
            if counter == 5:
                out[k] = 2 if b[k] == 1 else (1 if b[k] == 0 else 0)
            counter = counter + 1 if b[k] == 1 else (0 if b[k] == 0 else counter)
        return out

    @staticmethod
    def reduce_stuffed_bit(code_bit, stuffed_bit):
        """:335-353: the bits whose mark is 0"""
        return [c for c, s in zip(code_bit, stuffed_bit) if s == 0]

    @staticmethod
    def bits_to_msg(bits):
        """:272-277's field split over message bits (LSB first per byte) -> the information field (nothing is printed)"""
        raw = bytes(int(sum(int(bits[k + j]) << j for j in range(len(bits[k:k + 8])))) for k in range(0, len(bits), 8))
        return _fields(raw)[5]
