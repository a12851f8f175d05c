"""
Wide or narrow FM to audio -- the reference's decode_fm surface (decode_fm.py:15-72): ``decode_fm(sigsrc, offset, bw, audioFreq)``
and the ``getAudio`` property.

The chunk loop of decode_fm.py:61-70 -- offsetFreq -> blackmanHarris(151) -> bwLim(bw) -> demod_fm -> strict bwLim(audioFreq), the
results extended chunk after chunk -- is the loop decode_noaa runs with other constants, so both decoders call ``fm_audio_chunks``
below.  Over a device-resident recording the recorded chunks execute as one chunk list (comm.flush_all: dd_fused_process_chunks, then
dd_resample_fft_chunks for the strict resample of every chunk).  The strict resample works on one chunk at a time, as in the
reference: the audio depends on the chunk size.

Deviation from the reference: decode_fm.py:57 builds its chunker on a module global ``sigsrc``, which
exists only under the reference's own ``__main__``; here the chunker is built on the source the object was given.
"""
from . import chunker, comm, constants, demod_fm, filters


def fm_audio_chunks(src, offset, bw, audioFreq, strictness, chunkSize=None, use_device_raw=True, bhFilter=None):
    """The FM audio chunk loop of decode_noaa.py:600-629 and decode_fm.py:54-72 over `src`: a commSignal at `audioFreq`.
    Filter state, NCO index, decimation phase and the discriminator's last sample move on from chunk to chunk (the filter and the
    demodulator are made here, once per call, as the reference makes them).  use_device_raw: read through the source's device
    routes (raw u8 pairs resident on the device where it offers them, else read_device); False: its plain ``read``.
    bhFilter: the blackmanHarris(151) to use, for callers that look at its launch counters afterwards."""
    audioOut = comm.commSignal(audioFreq)
    if bhFilter is None:
        bhFilter = filters.blackmanHarris(151)
    fmDemodulator = demod_fm.demod_fm()
    chunkerObj = chunker.chunker(src, constants.PROC_CHUNKSIZE if chunkSize is None else chunkSize)
    read = src.read
    if use_device_raw:
        if hasattr(src, "read_device"):
            read = src.read_device
        if hasattr(src, "read_device_raw") and src.read_device_raw(0, 1) is not None:
            read = src.read_device_raw          # the recording stays in HBM as raw pairs; the fused kernel widens them
    for a, b in chunkerObj.getChunks:
        sig = comm.commSignal(src.sampFreq, read(a, b), chunkerObj).offsetFreq(offset) \
            .filter(bhFilter).bwLim(bw, uniq="First").funcApply(fmDemodulator.demod) \
            .bwLim(audioFreq, strictness)
        audioOut.extend(sig)
    return audioOut


class decode_fm:
    '''
    Object to decode wide or narrow FM: decode_fm(sigsrc, offset, bw, audioFreq) as in the reference (bw None -> 30000,
    audioFreq None -> 15000).  chunkSize (None -> constants.PROC_CHUNKSIZE) and use_device_raw are this package's extensions.
    '''

    def __init__(self, sigsrc, offset, bw=None, audioFreq=None, chunkSize=None, use_device_raw=True):
        '''Args:
            sigsrc: IQ data source
            offset (:obj:`float`): Frequency offset of source in Hz
            bw (:obj:`int`, optional): Bandwidth
            audioFreq (:obj:`int`, optional): sampling rate of the audio
        '''
        self.__bw = 30000 if bw is None else bw
        self.__sigsrc = sigsrc
        self.__offset = offset
        self.__audioFreq = 15000 if audioFreq is None else audioFreq
        self.__strictness = True
        self.__chunkSize = chunkSize
        self.__use_raw = use_device_raw
        self.__audio = None
        self.__filter = None

    @property
    def getAudio(self):
        '''Get the audio from data

        Returns:
            :obj:`commSignal`: An audio signal (computed once per object)
        '''
        if self.__audio is None:
            self.__filter = filters.blackmanHarris(151)
            self.__audio = fm_audio_chunks(self.__sigsrc, self.__offset, self.__bw, self.__audioFreq, self.__strictness,
                                           self.__chunkSize, self.__use_raw, self.__filter)
        return self.__audio

    def _decode_filter(self):
        """the blackmanHarris(151) getAudio ran through, its recorded chunks executed (tests read its launch counters)"""
        self.getAudio.device_signal
        return self.__filter

    def _launch_count(self):
        """fused kernel launches of getAudio (a chunk list in one launch counts once)"""
        return self._decode_filter()._launch_count()
