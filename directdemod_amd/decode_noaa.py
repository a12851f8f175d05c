"""
NOAA APT decoding -- the reference's decode_noaa surface (decode_noaa.py): sync detection from noaa_sync, image extraction
(getImage :255-465) and false colour (getColor :537-598) on the device.

Device work of getImage, after the crude sync: the zero-phase Butterworth band-pass and the block envelope of the crude-rate
audio (existing kernels), then the segmented median (dd_median_segments_f64: the 2 080 global segments, the calibration strips
and the sync FIFO windows), the batched line extraction (dd_apt_lines_f64: every half-line resampled and reduced to 1 040 pixel
medians in one call) and the pixel mapping (dd_apt_map_u8).  The O(lines) control logic stays on the host: the sync filling, the
A/B pairing, the line table and the telemetry state machine; their inputs come down from the device once, and the per-line
mapping parameters go up once.
"""
import numpy as np

from . import _ops, constants, demod_am, filters
from .noaa_sync import noaa_sync

NUM_PIXELS = int(0.5 / constants.NOAA_T)         # 2080 words per line (:296)
HALF_PIXELS = NUM_PIXELS // 2
WIGGLE = 200                                     # __fillSync's tolerance in samples (:480)
NCORR = 3                                        # depth of the calibration median FIFOs (:324)


def _most_common(values):
    """the value that occurs most often; of several such, the one a set of them yields first (the reference's max(set(.), key=count))"""
    vals = list(values)
    return max(set(vals), key=vals.count)


def fill_sync(csync, max_len):
    """decode_noaa.__fillSync (:467-509): keep the syncs spaced by the most common spacing (within WIGGLE samples), then fill
    the gaps before the first and between / after the kept ones at that spacing, up to max_len.  Returns a sorted list."""
    csync = np.asarray(csync, dtype=np.float64)
    step = _most_common(np.diff(csync))
    valid = []
    for a, b in zip(csync[:-1], csync[1:]):
        if abs(b - a - step) < WIGGLE:
            if a not in valid:
                valid.append(a)
            if b not in valid:
                valid.append(b)
    out = valid[:]
    c = valid[0] - step
    while c > WIGGLE:                            # before the first kept sync
        out.append(c)
        c -= step
    at, c = 0, step
    while valid[at] + c < max_len:               # walk from each kept sync to the next one (or to the end)
        nxt = at + 1 < len(valid)
        if nxt and (abs(valid[at + 1] - c - valid[at]) < WIGGLE or c + valid[at] > valid[at + 1]):
            at, c = at + 1, step
        else:
            out.append(valid[at] + c)
            c += step
    return list(np.sort(out))


def to_rate(sync, crude_rate, rate):
    """:287-293: crude sync indices -> sample positions at `rate` (float64, the reference's operation order)"""
    c = np.asarray(sync) / crude_rate
    c *= rate
    return c


def pair_syncs(a, b, rate):
    """:301-310: the filled sync lists of A and B, channel A first and as many B as A"""
    a, b = list(a), list(b)
    if b[0] < a[0]:
        b.pop(0)
    if b[-1] < a[-1]:
        a.pop(-1)
    if len(a) != len(b):
        b = np.array(a) + int(0.25 * rate)
    return a, b


def line_table(a, b, unc, rate, n):
    """:330-344 and :348: per decoded line (startA, endA, startB, endB, sync A found uncorrected); lines out of bounds are skipped"""
    rows = []
    for i in range(len(a)):
        sa, sb = int(a[i]), int(b[i])
        ea, eb = sb, sb + int(0.25 * rate)
        if i + 1 < len(a):
            eb = int(a[i + 1])
        if eb > n or ea > n or sa < 0 or sb < 0:
            continue
        rows.append((sa, ea, sb, eb, bool(np.any(unc == a[i]))))
    return rows


def slice_bounds(a, b, n):
    """Python's slice semantics of x[a:b] on a length-n array: (start, length)"""
    s, e, _ = slice(a, b).indices(n)
    return s, max(0, e - s)


def calibrate(low, high, strip_a, strip_b, sync_low, sync_high, in_unc):
    """The telemetry state machine of :348-425 over per-line scalars.

    low, high: the initial mapping bounds (percentiles of the global medians); per line i: strip_a[i] / strip_b[i] the medians of
    the strips before sync A / B, sync_low[i] / sync_high[i] the medians of the sync FIFOs (used where in_unc[i]).
    Returns (params, low, high, slope, intercept, [chIDA, chIDB]), low / high as the last line left them: params[i] = (0, low, high) while no calibration has been found, else
    (1, slope, intercept) -- the lines before the first calibration take its slope, as the reference's imageBuffer does."""
    from scipy import stats
    fifo, fifo_a, fifo_b, ch_b, ch_a = [], [], [], [], []
    last, last_sig = None, None
    state, pix_pts, sig_pts = 0, [], []
    slope = intercept = None
    ch = [None, None]
    params, first_cal = [], None
    for i in range(len(strip_a)):
        if in_unc[i]:
            v11, v244 = sync_low[i], sync_high[i]
            low = v11 - (v244 - v11) * (11 - 0) / (244 - 11)
            high = v11 - (v244 - v11) * (11 - 255) / (244 - 11)
        sv, sv2 = strip_a[i], strip_b[i]
        fifo = (fifo + [255 * (sv - low) / (high - low)])[-NCORR:]
        cur = np.median(fifo)
        fifo_a = (fifo_a + [sv])[-NCORR:]
        cur_sig = np.median(fifo_a)
        fifo_b = (fifo_b + [sv2])[-NCORR:]
        cur_sig2 = np.median(fifo_b)
        ch_b = (ch_b + [cur_sig2])[-100:]
        ch_a = (ch_a + [cur_sig])[-100:]
        if last is None or abs(cur - last) > 255.0 / 16:
            if state == 0 and last_sig is not None:          # a step: the first two wedges
                pix_pts, sig_pts, state = [last, cur], [last_sig, cur_sig], 1
            elif 1 <= state <= 6:                             # wedges rising by more than 2/24 of full scale
                if cur - pix_pts[-1] > 2 * 255.0 / (8 * 3):
                    pix_pts.append(cur)
                    sig_pts.append(cur_sig)
                    state += 1
                else:
                    state = 0
            elif state == 7:                                  # the drop after wedge 8: fit the nine points
                if pix_pts[-1] - cur > 2 * 255.0 / 3:
                    pix_pts = [cur] + pix_pts
                    sig_pts = [cur_sig] + sig_pts
                    fit = stats.linregress(sig_pts, np.arange(9) * 255.0 / 8)
                    slope, intercept = fit[0], fit[1]
                    if first_cal is None:
                        first_cal = i
                    if len(ch_b) > 1 + 64 + 8:
                        ch = [int(np.round((slope * np.median(ch_b[-1 - 64 - 8:-1 - 64]) + intercept) / (255.0 / 8))),
                              int(np.round((slope * np.median(ch_a[-1 - 64 - 8:-1 - 64]) + intercept) / (255.0 / 8)))]
                    ch_a, ch_b = [], []
                    state = 0
                else:
                    state = 0
        last, last_sig = cur, cur_sig
        params.append((0.0, low, high) if slope is None else (1.0, slope, intercept))
    if first_cal is not None:
        for i in range(first_cal):
            params[i] = params[first_cal]
    return params, low, high, slope, intercept, ch


class decode_noaa(noaa_sync):
    '''Object to decode NOAA APT: sync (noaa_sync), image, channel IDs and false colour on the device'''

    def __init__(self, sigsrc, offset, bw=None):
        super().__init__(sigsrc, offset, bw)
        self.__crude_audio = None
        self.__extracted_audio = None
        self.__image = None
        self.__image_dev = None
        self.__color = None
        self.__chid = [None, None]
        self.__low = self.__high = None
        self.__slope = self.__intercept = None
        self.__fill = None

    def audio(self, audioFreq=constants.NOAA_CRUDESYNCSAMPRATE, strictness=False, chunkSize=constants.PROC_CHUNKSIZE):
        out = super().audio(audioFreq, strictness, chunkSize)
        if audioFreq == constants.NOAA_CRUDESYNCSAMPRATE and not strictness:
            self.__crude_audio = out             # getImage's input (the reference's __audOut of getCrudeSync)
        return out

    @property
    def getAudio(self):
        '''the audio at NOAA_AUDSAMPRATE, strictly resampled (:85-96)'''
        if self.__extracted_audio is None:
            self.__extracted_audio = self.audio(constants.NOAA_AUDSAMPRATE, True)
        return self.__extracted_audio

    def getAccurateSync(self, batched=True, resident=True):
        '''[A, diff(A), peak heights A, times A, B, diff(B), peak heights B, times B] (:880)'''
        (ia, pa, ta), (ib, pb, tb) = super().getAccurateSync(batched=batched, resident=resident)
        ia = [int(v) for v in ia]
        ib = [int(v) for v in ib]
        return [ia, np.diff(ia), list(pa), list(ta), ib, np.diff(ib), list(pb), list(tb)]

    @property
    def channelID(self):
        if self.__image is None:
            self.getImage
        return list(self.__chid)

    @property
    def getImage(self):
        '''the image, uint8 [lines x 2080] (:255-465)'''
        if self.__image is None:
            self.__extract()
        return self.__image

    @property
    def getImageA(self):
        return self.getImage[:, :HALF_PIXELS]

    @property
    def getImageB(self):
        return self.getImage[:, HALF_PIXELS:]

    @property
    def getColor(self):
        '''false colour image, uint8 [lines x 1040 x 3] (:537-598)'''
        if self.__color is None:
            img = self.getImage
            rows, width = img.shape
            if width < NUM_PIXELS:
                raise IndexError("image rows hold %d pixels, the false colour needs %d" % (width, NUM_PIXELS))
            self.__color = _ops.apt_color(self.__image_dev, rows, width).to_host()[:rows * HALF_PIXELS * 3].reshape(rows, HALF_PIXELS, 3)
        return self.__color

    def getMapImage(self, cTime, destFileRot, destFileNoRot, satellite, tleFile=None):
        '''Map overlay of the image: not provided by this package (it needs TLE files, pyorbital and a map library's data);
        raises NotImplementedError.'''
        raise NotImplementedError("getMapImage is not provided by directdemod_amd")

    # ---- the decoder's calibration results (for tests and tools)
    @property
    def calibration(self):
        '''(low, high, slope, intercept) of the last getImage'''
        return self.__low, self.__high, self.__slope, self.__intercept

    @property
    def filledSync(self):
        '''the filled sync positions (A, B) of the last getImage, before the A/B pairing'''
        return self.__fill

    def __extract(self):
        sa, sb = self.getCrudeSync()
        if self.__crude_audio is None:
            self.audio(constants.NOAA_CRUDESYNCSAMPRATE, False)
        aud = self.__crude_audio
        rate = aud.sampRate
        x = aud.device_signal
        if x.dtype != np.dtype(np.float64):
            from .comm import _convert
            x = _convert(x, np.float64)
        bp = filters.butter(rate, 400, 4400, typeFlt=constants.FLT_BP, zeroPhase=True).applyOn(x)      # :278
        env = demod_am.demod_am().demod_blocks(bp, 60000 * 4)                                           # :281
        n = env.n

        unc = to_rate(sa, self.crudeRate, rate)                                                         # :284-296
        self.__fill = (fill_sync(unc, n), fill_sync(to_rate(sb, self.crudeRate, rate), n))
        a, b = pair_syncs(self.__fill[0], self.__fill[1], rate)
        rows = line_table(a, b, unc, rate, n)

        # the half-line table (A0, B0, A1, B1, ...) and where the sync pixels of the A halves go: the low stream first, then the high
        bits = np.asarray(constants.NOAA_SYNCA, dtype=np.int64)
        nlow, nhigh = int(np.sum(bits == 0)), int(np.sum(bits == 1))
        nl = len(rows)
        tab = np.array([(r[0], max(0, r[1] - r[0]), r[2], max(0, r[3] - r[2])) for r in rows], dtype=np.int64).reshape(nl, 4)
        starts, lens = tab[:, 0::2].reshape(-1), tab[:, 1::2].reshape(-1)
        use = np.array([r[4] for r in rows], dtype=bool)
        k_a = tab[:, 1] // HALF_PIXELS
        low_end = np.cumsum(np.where(use, k_a * nlow, 0))           # the streams' lengths after each line
        high_end = np.cumsum(np.where(use, k_a * nhigh, 0))
        total_low = int(low_end[-1]) if nl else 0
        half_off = np.full((nl, 2, 2), -1, dtype=np.int64)           # [line][half][low, high]
        half_off[use, 0, 0] = (low_end - k_a * nlow)[use]
        half_off[use, 0, 1] = (total_low + high_end - k_a * nhigh)[use]
        stream_len = total_low + (int(high_end[-1]) if nl else 0)
        mask = sum(1 << j for j in range(len(bits)) if bits[j])
        pix, stream = _ops.apt_lines(env, starts, lens, half_off.reshape(-1), mask, len(bits), stream_len)

        # every median in two device calls, one download
        m = n // NUM_PIXELS
        L1 = int((len(constants.NOAA_SYNCA) * constants.NOAA_T) * rate)
        L2 = int((len(constants.NOAA_SYNCB) * constants.NOAA_T) * rate)
        seg = [(np.arange(NUM_PIXELS, dtype=np.int64) * m, np.full(NUM_PIXELS, m, dtype=np.int64))]
        s1 = np.array([slice_bounds(r[0] - L1, r[0], n) for r in rows], dtype=np.int64).reshape(-1, 2)
        s2 = np.array([slice_bounds(r[2] - L2, r[2], n) for r in rows], dtype=np.int64).reshape(-1, 2)
        seg.append((s1[:, 0], s1[:, 1]))
        seg.append((s2[:, 0], s2[:, 1]))
        fl = NUM_PIXELS + 2 * nl
        lo_len = np.minimum(low_end, constants.NOAA_COLORCORRECT_FIFOLEN)
        hi_len = np.minimum(high_end, constants.NOAA_COLORCORRECT_FIFOLEN)
        fo = np.concatenate([low_end - lo_len, total_low + high_end - hi_len]).astype(np.int64)
        fn = np.concatenate([lo_len, hi_len]).astype(np.int64)
        from ._hip import DevArray
        meds = DevArray(fl + 2 * nl, np.float64)
        _ops.median_segments(env, np.concatenate([s[0] for s in seg]), np.concatenate([s[1] for s in seg]), out=meds.view(0, fl))
        if nl:
            _ops.median_segments(stream, fo, fn, out=meds.view(fl, 2 * nl))
        mh = meds.to_host()
        g = mh[:NUM_PIXELS]
        strip_a, strip_b = mh[NUM_PIXELS:NUM_PIXELS + nl], mh[NUM_PIXELS + nl:fl]
        sync_low, sync_high = mh[fl:fl + nl], mh[fl + nl:]

        low, high = np.percentile(g, (0.5, 99.5))                                                       # :312-315
        params, low, high, slope, intercept, ch = calibrate(low, high, strip_a, strip_b, sync_low, sync_high, use)
        self.__low, self.__high, self.__slope, self.__intercept, self.__chid = low, high, slope, intercept, ch
        if nl == 0:
            raise ValueError("max() arg is an empty sequence")            # no line to decode (:458-462)
        img = _ops.apt_map(pix, nl, NUM_PIXELS, params)
        self.__image_dev = img
        self.__image = img.to_host()[:nl * NUM_PIXELS].reshape(nl, NUM_PIXELS)
