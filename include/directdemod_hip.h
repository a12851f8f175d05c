/*
 * directdemod_hip.h -- C-ABI of the MI355X (gfx950) IQ-sample DSP hot path that
 * replaces DirectDemod's NumPy/SciPy per-sample path.
 *
 * The reference is pure Python (no FFI of its own); every entry point below
 * replaces one SciPy/NumPy call site of the reference, cited as file:line
 * relative to the reference tree.  The Python classes in directdemod_amd/
 * (commSignal, filters.*, demod_fm, demod_am, chunker -- same names/signatures
 * as the reference's) bind these symbols with ctypes; INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; all buffers are DEVICE pointers unless the parameter
 *     name ends in _host;  complex64 = interleaved float {re,im}.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     compute entry points are asynchronous on that stream; carried state
 *     lives in device memory inside the handles, so chunk loops need no
 *     host<->device synchronisation.
 *   - return value: 0 = DD_OK, <0 = error (never throws); dd_last_error()
 *     returns a thread-local message.
 *   - one caller thread per handle (the reference is single-threaded and its
 *     state carry makes chunk order significant).
 */
#ifndef DIRECTDEMOD_HIP_H
#define DIRECTDEMOD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_OK               0
#define DD_ERR_INVALID     -1   /* bad argument (maps to ValueError/TypeError) */
#define DD_ERR_HIP         -2   /* HIP runtime error */
#define DD_ERR_NOMEM       -3
#define DD_ERR_UNSUPPORTED -4
#define DD_ERR_NODEVICE    -5   /* no MI355X visible: the product path fails loudly */
#define DD_ERR_TIMEOUT     -6   /* a chunk-list launch (dd_*_process_chunks) gave up waiting for the carried state of the previous
                                 * chunk inside the launch: the outputs of THAT call are invalid.  Reported by the next chunk-list
                                 * call on the same filter or by dd_stream_sync, whichever comes first */

/* FIR history initialisation (filters.py:44-48, 64-70) */
#define DD_HIST_ZEROS 0     /* plain lfilter / lfiltic with no past inputs */
#define DD_HIST_ONES  1     /* lfilter_zi(b,[1]) unscaled == delay line of 1.0+0j (quirk Q1) */
#define DD_HIST_GIVEN 2     /* explicit past inputs, oldest first */

/* dd_chain_create flags */
#define DD_CHAIN_NCO        1   /* apply commSignal.offsetFreq        (comm.py:63-78)   */
#define DD_CHAIN_FM         2   /* apply demod_fm.demod on the output (demod_fm.py:29-51) */
#define DD_CHAIN_U8_INPUT   4   /* input is interleaved u8 I,Q; source.read fused (source.py:117-118) */
#define DD_CHAIN_FORCE_DIRECT 8 /* disable the MFMA fast path (f32 direct form only) */
#define DD_CHAIN_TIGHT       16 /* M = 1 chains: keep the running-sum kernel (k_chain_cos1k, filters.hamming(255)) off -- its FIR output is
                                 * a0 R + a1 C with R, C the rectangular-window sums, which cancel to the window's -50 dB in the stop band: FM
                                 * angles of a signal the filter rejects are good to 1e-3 rad there, against 3e-4 for the transform kernel
                                 * this flag selects instead (1.4 x the time).  Also a flag of dd_fused_process(_chunks);
                                 * Python: filters.filter.tight = True.  No reference counterpart (float64 there, filters.py:64-70) */

/* ---- runtime ---------------------------------------------------------------- */
const char* dd_last_error(void);
const char* dd_version(void);
int  dd_device_count(int* count);
int  dd_set_device(int device);
/* the calling thread's current device (HIP keeps one per host thread, default 0): a helper thread started on behalf of a caller
 * takes the caller's device with dd_set_device(dd_get_device()) before it touches the GPU */
int  dd_get_device(int* device);
int  dd_device_name(char* buf, int buflen);
int  dd_malloc(void** dptr, size_t bytes);
int  dd_free(void* dptr);
int  dd_memset(void* dptr, int value, size_t bytes, void* stream);
int  dd_host_alloc_pinned(void** hptr, size_t bytes);
int  dd_host_free_pinned(void* hptr);
/* pin / unpin a range of caller-owned host memory in place (hipHostRegister): lets source.IQwav's memmap or an
 * in-memory recording feed hipMemcpyAsync directly (BASELINE north_star: "pinned-host ring buffers with
 * hipMemcpyAsync overlapped on a side stream").  DD_ERR_UNSUPPORTED when the range cannot be pinned. */
int  dd_host_register(void* hptr, size_t bytes);
int  dd_host_unregister(void* hptr);
/* (diagnostic entry points -- dd_debug_*: kernel selection for A/B runs, LDS fills, launch-plan arithmetic for the CPU test suite -- are
 * declared in directdemod_hip_debug.h; none of them has a reference counterpart, none is needed to use the library) */
int  dd_memcpy_h2d(void* dst, const void* src_host, size_t bytes, void* stream);
int  dd_memcpy_d2h(void* dst_host, const void* src, size_t bytes, void* stream);
int  dd_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
/* a 4 KB and a 1 MB synchronous host-to-device copy on the calling thread's device (the process's first copy pays ~90 ms of runtime set-up
 * whatever its size, its first large one another ~7 ms): _hip.py makes them on a helper thread when the GPU is first touched.  No reference counterpart. */
int  dd_copy_warmup(void);
/* names one kernel of every translation unit of the library, so that the runtime loads the code objects now (1-4 ms each) and not inside the
 * caller's first launches: _hip.py calls it on the same helper thread, after dd_copy_warmup.  No reference counterpart. */
int  dd_code_warmup(void);
int  dd_stream_create(void** stream);
int  dd_stream_destroy(void* stream);
int  dd_stream_sync(void* stream);
int  dd_event_create(void** ev);
int  dd_event_destroy(void* ev);
int  dd_event_record(void* ev, void* stream);
int  dd_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* syncs on ev_stop */
int  dd_event_sync(void* ev);
int  dd_stream_wait_event(void* stream, void* ev);   /* later work on `stream` waits for `ev` (no host sync) */

/* ---- S1: source.IQwav/IQdat/IQwavAlt.read (source.py:117-118,209-210,303-304) -- */
/* interleaved uint8 I,Q  ->  complex64 minus (127.5+127.5j) */
int dd_u8iq_to_c64(const uint8_t* in_iq, float* out_c64, int64_t n, void* stream);

/* ---- N1: commSignal.offsetFreq (comm.py:63-78) ------------------------------ */
/* out[i] = in[i] * exp(-j 2 pi f (start_index+i)/fs).  `cycles_q64` is
 * frac(f/fs) * 2^64 (two's complement wrap), computed exactly on the host; the
 * phase is exact modular integer arithmetic for any start_index.
 * In place allowed (in == out). */
int dd_nco_c64(const float* in_c64, float* out_c64, int64_t n, uint64_t cycles_q64,
               int64_t start_index, void* stream);
/* the same with a per-sample frequency array (device, float64 Hz): comm.py:77 with an array
 * freqOffset (Doppler correction, decode_funcube.py:228); phase formed and reduced in float64 */
int dd_nco_c64_freqs(const float* in_c64, float* out_c64, int64_t n, const double* freqs_hz, double samp_rate,
                     int64_t start_index, void* stream);
/* the same with the frequency formed in the kernel: f[i] = start_hz + i * delta_hz (one multiplication, one addition, each
 * rounded to float64), clipped to target_hz from above when target_hz > start_hz and from below otherwise -- the ramp of
 * decode_funcube.py:215-226 (np.arange(cur, cur + n d + 10 d, d)[:n], then the clip).  `delta_hz` is NumPy's fill step
 * (start + d) - start, formed on the host; phase arithmetic exactly dd_nco_c64_freqs'.  In place allowed. */
int dd_nco_c64_ramp(const float* in_c64, float* out_c64, int64_t n, double start_hz, double delta_hz, double target_hz,
                    double samp_rate, int64_t start_index, void* stream);

/* ---- D1: sandbox/frequency_shift.py (the --freqshift part of decode_funcube.py:202-228) ---- */
/* make_fft (frequency_shift.py:5-44) over raw interleaved uint8 I,Q on the device.  Slices of `window` samples (a power of
 * two, 16..8192) start at raw offsets 0, 2 window, ... including a final partial one; every slice counts towards `every`, only
 * full ones add |FFT((I-127) + j(Q-127))| (magnitudes, not powers) to the row's sum; a row closes at the first count >= every
 * (ceil(every) slices), slices after the last closed row are dropped.  out_rows[r * window + c] =
 * log(fftshift(sum)[c] / window / every), float32, `max_rows` rows of room; *n_rows is the row count (out_rows may be null to
 * ask for it alone).  A row's windows are summed in a fixed order (a fixed split into segments, then the segments in order):
 * no atomics, equal runs give equal bits.  raw_bytes even, at least one full window; every <= 1 with a partial tail is
 * DD_ERR_INVALID (the reference dies in fftshift of a scalar). */
int dd_waterfall_u8(const uint8_t* raw_iq, int64_t raw_bytes, int window, double every, float* out_rows, int64_t max_rows,
                    int64_t* n_rows, void* stream);
/* per row of a [rows x width] float32 array the index, relative to band_start, of the first maximum over columns
 * [band_start, band_stop): np.argmax of frequency_shift.py:95 (the row minimum subtracted at :94 does not move it).
 * Like np.argmax, the first NaN of the band wins; the result always lies in [0, band_stop - band_start). */
int dd_band_argmax_f32(const float* rows_f32, int64_t rows, int width, int band_start, int band_stop, int32_t* out_idx,
                       void* stream);

/* ---- F1/F3: filters.filter.applyOn, FIR (a=[1]) (filters.py:21-75) ------------ */
typedef struct dd_fir dd_fir;
int dd_fir_create(dd_fir** h, const double* taps, int ntaps);
int dd_fir_destroy(dd_fir* h);
/* (re)initialise the carried history: DD_HIST_ZEROS / DD_HIST_ONES / DD_HIST_GIVEN
 * (hist_host: ntaps-1 complex64 (or float for the real path), oldest first). */
int dd_fir_reset(dd_fir* h, int mode, const float* hist_host, void* stream);
/* history of the float64 real path (dd_fir_f64) given as ntaps-1 doubles, oldest first: lfiltic(b,[1],x,initOut)
 * (filters.py:47-48,66-67) with initOut values that are not float32 numbers.  Call after dd_fir_reset. */
int dd_fir_reset_hist_f64(dd_fir* h, const double* hist_host, void* stream);
/* causal FIR, complex64 in -> complex64 out, same length, history carried
 * (storeState) or not (carry=0: history read but left untouched). */
int dd_fir_c64(dd_fir* h, const float* in_c64, float* out_c64, int64_t n, int carry, void* stream);
/* real float64 path used at audio rate (NOAA tail keeps float64) */
int dd_fir_f64(dd_fir* h, const double* in, double* out, int64_t n, int carry, void* stream);

/* ---- F2: filters.filter zeroPhase -> scipy.signal.filtfilt (filters.py:72-73) -- */
/* odd extension 3*ntaps, forward/backward with zi*x0; stateless.
 * is_complex: 0 = float64 real, 1 = complex128 interleaved doubles.  n > 3*ntaps. */
int dd_filtfilt_f64(const double* taps_host, int ntaps, const double* in, double* out,
                    int64_t n, int is_complex, void* stream);
/* complex64 in/out, float32 arithmetic (full-rate IQ windows, decode_noaa.py:852) */
int dd_filtfilt_c64(const double* taps_host, int ntaps, const float* in_c64, float* out_c64,
                    int64_t n, void* stream);

/* ---- F4: filters.butter -> scipy.signal.lfilter with a != [1] (filters.py:232-273) ---
 * Transposed direct form II recurrence, float64, state carried on the device.
 * Short inputs: one lane per real component.  From 4096 samples up: block-parallel
 * (block end states from zero, two- or three-level scan of the block start states with
 * the block map A^256 held in double-double, blocks re-run from their true start states;
 * asynchronous on `stream`, intermediates in a scratch buffer owned by the handle), which
 * is what full-rate IQ through a butter takes (decode_funcube.py:160,230; SURVEY.md
 * 8f-3).  b, a: `n` coefficients each
 * (pad the shorter with zeros), a[0] != 0.  zi_host: n-1 initial state values
 * (scipy.signal.lfilter_zi(b, a), unscaled like filters.py:45) or NULL for zeros. */
typedef struct dd_iir dd_iir;
int dd_iir_create(dd_iir** h, const double* b, const double* a, int n, const double* zi_host);
int dd_iir_destroy(dd_iir* h);
/* is_complex: 0 = float64, 1 = complex128 (interleaved); carry: keep the final state */
int dd_iir_f64(dd_iir* h, const double* in, double* out, int64_t n, int is_complex, int carry, void* stream);
/* the same on complex64 input, complex128 output (what scipy.signal.lfilter returns for a complex64 signal and float64 coefficients): the IQ
 * stream as source.py hands it over, low-passed before any decimation (decode_funcube.py:160, decode_meteorm2.py:157 -> filters.py:75).  From 4096
 * samples up the block-parallel passes read the complex64 samples as they are (8 + 8 + 16 bytes per sample move instead of 72 through a widened
 * copy); shorter or unaligned inputs are widened into `out` and filtered there.  in_c64 != out_c128. */
int dd_iir_c64(dd_iir* h, const void* in_c64, double* out_c128, int64_t n, int carry, void* stream);
/* scipy.signal.filtfilt(b, a, x): odd extension 3*n, zi scaled by the first sample of each pass */
int dd_iir_filtfilt_f64(dd_iir* h, const double* in, double* out, int64_t n, int is_complex, void* stream);

/* ---- R1: commSignal.bwLim non-strict (comm.py:118-130) ---------------------- */
/* out[i] = in[offset + i*m]; elem_bytes in {4,8,16}; n_out = ceil((n-offset)/m) */
int dd_decimate(const void* in, void* out, int64_t n, int m, int offset, int elem_bytes,
                int64_t* n_out, void* stream);

/* ---- D1: demod_fm.demod (demod_fm.py:29-51) --------------------------------- */
typedef struct dd_fm dd_fm;
int dd_fm_create(dd_fm** h);
int dd_fm_destroy(dd_fm* h);
int dd_fm_reset(dd_fm* h);
/* angle(x[i]*conj(x[i-1])); first call with carry writes n-1 outputs, later calls n
 * (quirk Q3); carry=0 always n-1.  *n_out receives the count written. */
int dd_fm_discrim_c64(dd_fm* h, const float* in_c64, float* out, int64_t n, int carry,
                      int64_t* n_out, void* stream);

/* ---- D2: demod_fmAD.demod (demod_fm.py:57-96) -------------------------------- */
/* np.diff(np.unwrap(np.angle(x))): per-sample angles (angle(0) = 0), each difference moved by 2 pi when its magnitude is
 * beyond pi.  The carried quantity is the last ANGLE (demod_fm.py:89,93), kept on the device inside the handle: first call
 * with carry writes n-1 outputs, later calls n; carry=0 always n-1.  *n_out receives the count written.  A sample of exactly
 * zero gives angle(next) - 0 and 0 - angle(previous) here, where dd_fm_discrim_c64 gives 0 twice. */
typedef struct dd_fmad dd_fmad;
int dd_fmad_create(dd_fmad** h);
int dd_fmad_destroy(dd_fmad* h);
int dd_fmad_reset(dd_fmad* h);
int dd_fm_angle_diff_c64(dd_fmad* h, const float* in_c64, float* out, int64_t n, int carry,
                         int64_t* n_out, void* stream);

/* ---- F5: filters.medianFilter.applyOn -> scipy.signal.medfilt (filters.py:322-326) --- */
/* sliding median of odd width ksize over a 1-D real signal, zeros beyond both ends; out[i] is one of the inputs (or the
 * padding zero), bit for bit.  ksize even: DD_ERR_INVALID; ksize > DD_MEDFILT_MAX: DD_ERR_UNSUPPORTED.  n < ksize is valid.
 * in != out.  A workgroup writes DD_MEDFILT_TILE outputs. */
#define DD_MEDFILT_MAX  255
#define DD_MEDFILT_TILE 1024
int dd_medfilt_f32(const float* in, float* out, int64_t n, int ksize, void* stream);
int dd_medfilt_f64(const double* in, double* out, int64_t n, int ksize, void* stream);

/* ---- F6: filters.blackmanHarrisConv.applyOn -> scipy.signal.convolve(x, w, mode='same') (filters.py:145-174) --- */
/* out[i] = sum_k taps[k] in[i + (ntaps-1)/2 - k], in taken as zero outside [0, n) (np.convolve(in, taps)[s : s + n], odd
 * and even ntaps, n < ntaps included).  taps: ntaps float64 on the DEVICE.  Sums in float64; the complex64 form rounds once
 * at the store.  Stateless; in != out. */
int dd_conv_same_f64(const double* in, double* out, int64_t n, const double* taps, int ntaps, void* stream);
int dd_conv_same_c64(const float* in_c64, float* out_c64, int64_t n, const double* taps, int ntaps, void* stream);

/* ---- fused hot path: offsetFreq -> filter(FIR) -> bwLim(M) -> demod_fm -------
 * (decode_noaa.py:623, decode_fm.py:64-68, decode_afsk1200.py:79-94,
 *  tutorial/3_chunking.py:24-38).  One kernel per chunk; all carried state (NCO
 *  sample index, FIR history, decimation phase, last FM sample) is derived from
 *  the absolute sample index or kept on the device. */
/* Object-model form: state lives where the reference keeps it -- FIR history in the
 * filter object (dd_fir), last FM sample in the demodulator (dd_fm, NULL = no FM,
 * output is complex64), NCO sample index and decimation phase are the chunker
 * variables "freqoffset"/"bwlim" passed by value (chunker.py:54-84, comm.py:73-76,
 * 121-125).  nco: 0/1.  offset: chunk-relative index of the first kept sample.
 * flags: DD_CHAIN_U8_INPUT | DD_CHAIN_FORCE_DIRECT.  carry: storeState of the filter. */
int dd_fused_process(dd_fir* fir, dd_fm* fm, const void* in, void* out, int64_t n,
                     int nco, uint64_t cycles_q64, int64_t start_index, int decim, int offset,
                     int flags, int carry, int64_t* n_out, void* stream);

/* A chunk LIST through the object-model form: `in` points at the first chunk's first sample, chunk i is
 * bounds_host[i+1] - bounds_host[i] samples long (nchunks + 1 ascending offsets), start_index / offset are the chunker
 * variables of the FIRST chunk (the later chunks' follow by the reference's carry rules, comm.py:75-76, 123-125), the
 * filter and the demodulator carry their state (storeState) exactly as over nchunks dd_fused_process calls: outputs
 * concatenated at `out`, bit-identical to that loop, counts in n_out_host; ONE launch for a decimating chain.  The drop-in
 * classes use it when a chunk loop's chunks are consecutive views of one device-resident recording (comm.py). */
int dd_fused_process_chunks(dd_fir* fir, dd_fm* fm, const void* in, void* out, const int64_t* bounds_host, int nchunks,
                            int nco, uint64_t cycles_q64, int64_t start_index, int decim, int offset, int flags,
                            int64_t* n_out_host, void* stream);

/* Convenience handle bundling one filter, one FM demodulator and the chunker
 * variables of one stream (used by bench.py and the sharded multi-GPU driver). */
typedef struct dd_chain dd_chain;
int dd_chain_create(dd_chain** h, const double* taps, int ntaps, uint64_t cycles_q64,
                    int decim, int flags);
int dd_chain_destroy(dd_chain* h);
/* start a new stream (new chunker object): abs index 0, history ones, no FM state */
int dd_chain_reset(dd_chain* h, void* stream);
/* Start a stream position without touching the device: the next chunk is taken to begin at
 * absolute sample `abs_index` with an all-zero FIR history and no previous FM sample (index 0:
 * the stream start, history of ones like dd_chain_reset).  A shard can then be run in ONE call
 * over [start - lead, stop) with lead >= ntaps-1+decim and the lead-in's outputs discarded --
 * the same outputs as dd_chain_prime + dd_chain_process (the halo is re-filtered
 * locally, no exchange), one launch instead of two. */
int dd_chain_seek(dd_chain* h, int64_t abs_index, void* stream);

/* multi-GPU / shard start: establish state as if samples [0, abs_index) had been
 * processed, from the `n_halo` raw input samples that precede abs_index
 * (n_halo >= ntaps-1+decim; fewer only if abs_index == n_halo i.e. stream start). */
int dd_chain_prime(dd_chain* h, const void* halo_in, int64_t n_halo, int64_t abs_index, void* stream);
/* number of outputs the next dd_chain_process(n) will write (pure host arithmetic) */
int64_t dd_chain_out_count(const dd_chain* h, int64_t n);
/* process one chunk of n input samples (complex64, or u8 pairs with DD_CHAIN_U8_INPUT).
 * out: float32 radians when DD_CHAIN_FM, else complex64. */
int dd_chain_process(dd_chain* h, const void* in, void* out, int64_t n, int64_t* n_out, void* stream);
/* Several chunks in one call: chunk i is the samples [bounds_host[i], bounds_host[i+1]) of `in` (nchunks + 1 ascending
 * offsets).  Same outputs, bit for bit, as nchunks dd_chain_process calls in that order -- concatenated at `out`, counts
 * per chunk in n_out_host (may be NULL) -- and the same carried state afterwards; for a decimating chain (the reference's
 * chunk loops: decode_fm.py:54-70 with 2^22-sample chunks, decode_noaa.py:614-624) ONE kernel launch instead of one per
 * chunk (persistent workgroups walk every chunk's tiles, the state a chunk hands to the next travels through device
 * memory inside the launch).  bench.py: C3's sixteen chunks 0.23 ms as a loop, 0.12 ms here. */
int dd_chain_process_chunks(dd_chain* h, const void* in, void* out, const int64_t* bounds_host, int nchunks,
                            int64_t* n_out_host, void* stream);
/* which kernel the chain dispatches to: 0 = f32 direct form, 1 = f16-split MFMA Toeplitz */
int dd_chain_path(const dd_chain* h);
/* the kernel the last dd_chain_process call launched (one launch per call): lets tests and benchmarks assert
 * that the intended kernel -- not a slower sibling with the same results -- produced the output */
#define DD_KERNEL_NONE 0             /* nothing launched yet (or a chunk without a kept sample) */
#define DD_KERNEL_DENSE_F32 1        /* k_chain_dense: M = 1, f32 direct form */
#define DD_KERNEL_DECIM_TILES 2      /* k_chain_decim: M > 1, one workgroup per tile (short or unaligned chunks) */
#define DD_KERNEL_DECIM_PERSISTENT 3 /* k_chain_decim_p: M > 1, persistent interior run + edge tiles in the same launch */
#define DD_KERNEL_MFMA_WS 4          /* retired (k_chain_mfma_ws, round 1's wave-specialised MFMA kernel, since removed): never reported; the number is not reused */
#define DD_KERNEL_MFMA_TILES 5       /* k_chain_mfma_edge: M = 1, MFMA, one workgroup per tile */
#define DD_KERNEL_MFMA_AB 6          /* k_chain_mfma_ab: M = 1, FM or complex64 output, two alternating matrix-wave sets + edge tiles in the same launch */
#define DD_KERNEL_FFT_OS 7           /* k_chain_fft1k: M = 1, FM output, 162..256 taps: f32 overlap-save FFT convolution, one wave per 1024-point block, NCO commuted into the tap spectrum, whole chunk in one launch */
#define DD_KERNEL_DECIM_MULTI 8      /* k_chain_decim_multi: M > 1, every chunk of a dd_chain_process_chunks call in one launch */
#define DD_KERNEL_COS_RS 9           /* k_chain_cos1k: M = 1, FM or complex64 output, 255 taps a0 + a1 cos(2 pi k / 254) (filters.hamming): the FIR as three running sums, one wave per run of 1024-sample rows, whole chunk in one launch */
#define DD_KERNEL_DECIM_WAVE 10      /* k_chain_decim_w: M > 1 (even, 8..64), up to 256 taps, FM or complex64 output, complex64 or raw u8 input: one wave per row of 64 kept outputs on the absolute decimation grid, no barrier; a chunk list is ONE launch of it.  Since round 6 only where K > 8 M */
#define DD_KERNEL_DECIM_BLOCKS 11    /* k_chain_decim_b (round 6): the same rows and grids for K <= 8 M (every K for M >= 32: the reference's /34 and /50) -- every staged sample is read once: a lane forms the ceil(K / M) block sums of the M samples that end at its kept sample on the matrix pipe (v_mfma_f32_4x4x1, exact f32), the sums travel up the lanes */
int dd_chain_last_kernel(const dd_chain* h);
int dd_fir_last_kernel(const dd_fir* h);       /* the same for a filter object driven through dd_fused_process (the drop-in classes) */
long long dd_fir_launch_count(const dd_fir* h); /* fused kernel launches through this filter since it was created or last reset (a chunk list in one launch counts once): tests tell "one launch" from "a launch per chunk" by it */
/* HIP-event timing of the last dd_chain_process main kernel is up to the caller. */

/* ---- R2: commSignal.bwLim strict -> scipy.signal.resample (comm.py:110-116) --- */
/* Fourier-domain resample of one chunk, float64 real: n -> num samples.  Asynchronous on `stream`; the intermediates
 * live in a grow-only buffer kept by the library (no allocation, no synchronisation in the steady state). */
int dd_resample_fft_f64(const double* in, double* out, int64_t n, int64_t num, void* stream);
/* The same per-chunk resample for a whole chunk list in one call (a chunk loop ends every chunk in bwLim(strict):
 * decode_fm.py:54-70): chunk i is the n_host[i] samples at in + in_off_host[i] (float32 when in_is_f32 -- the FM output of
 * dd_chain_process_chunks -- else float64) and becomes num_host[i] float64 samples at out + out_off_host[i]; offsets in
 * elements.  Chunks of equal (n, num) share batched hipFFT plans: two transforms per group instead of two per chunk. */
int dd_resample_fft_chunks(const void* in, int in_is_f32, const int64_t* in_off_host, const int64_t* n_host, double* out,
                           const int64_t* out_off_host, const int64_t* num_host, int count, void* stream);

/* ---- polyphase rational resampler (BASELINE north_star, config 3 "polyphase resample to 11.025 kS/s").
 * The reference has NO counterpart (its only resampler is the FFT one above, comm.py:110-116): a build-defined
 * stage following SciPy's published scipy.signal.resample_poly (upfirdn of the front-padded, up-scaled low-pass
 * `taps`; n_pre_remove outputs dropped), float64 real, in STREAM form: state (the last ceil(ntaps/up) inputs, the
 * input and output positions) is carried from call to call, a call emits the outputs whose inputs have all
 * arrived, flush = 1 emits the tail (inputs past the end are zeros) -- concatenated, the outputs equal
 * resample_poly of the concatenated input.  One caller thread per handle. */
typedef struct dd_rpoly dd_rpoly;
int dd_rpoly_create(dd_rpoly** h, const double* taps, int ntaps, int up, int down, int64_t n_pre_remove);
int dd_rpoly_destroy(dd_rpoly* h);
int dd_rpoly_reset(dd_rpoly* h);
int64_t dd_rpoly_out_count(const dd_rpoly* h, int64_t n, int flush);
int dd_rpoly_process(dd_rpoly* h, const double* in, int64_t n, int flush, double* out, int64_t* n_out, void* stream);

/* ---- A1: demod_am.demod = abs(hilbert(x)) (demod_am.py:18-29) in fixed blocks
 *      (decode_noaa.py:647-653: 240 000-sample blocks, chunker rule).  Asynchronous on `stream` like
 *      dd_resample_fft_f64: intermediates come from a grow-only buffer the library keeps per (device, stream) -- no
 *      allocation and no synchronisation in the steady state; callers on different streams never share a buffer,
 *      two host threads on one stream take turns enqueuing ----------- */
int dd_am_envelope_f64(const double* in, double* out, int64_t n, int64_t block, void* stream);

/* ---- X1: decode_noaa.__correlate (decode_noaa.py:659-675) --------------------- */
/* out[i] = corr_same(h,needle)[i] / sqrt(winenergy_same(h,m)[i] * sum(needle^2)) */
int dd_xcorr_norm_f64(const double* h, int64_t n, const double* needle_host, int m,
                      double* out, void* stream);

/* ---- X2: peak pick of decode_noaa.__correlateAndFindPeaks (decode_noaa.py:713-751) */
/* cor: n float64 on device, n < 2^31 (the selection and candidate kernels count in 32 bits; DD_ERR_INVALID beyond).  Writes up to
 * max_peaks int64 indices (already shifted by -needle_len/2, sorted) to peaks_host and their count to n_peaks.  The kernels are
 * those of dd_noaa_crude_tail, run for one needle with the threshold computed on the host: no limit on the expected peak count
 * or on the number of candidates.  Synchronous. */
int dd_find_peaks_f64(const double* cor, int64_t n, double samp_rate, int needle_len,
                      int64_t* peaks_host, int max_peaks, int* n_peaks, void* stream);

/* ---- accurate-sync windows, batched (decode_noaa.getAccurateSync, decode_noaa.py:808-880;
 *      SURVEY.md 8f-2).  For each of n_windows windows of win_len IQ samples starting at
 *      iq[starts_host[w]] (iq on the device; iq_kind 0 = complex64, 1 = interleaved uint8 pairs
 *      minus 127.5, source.py:117-118) runs the per-window chain of :852-853 --
 *      offsetFreq (sample index restarting at 0, cycles_q64 as in dd_nco_c64) -> zero-phase FIR
 *      fir_taps (blackmanHarris(151)) -> demod_fm (stateless) -> demod_am -> zero-phase FIR
 *      pre_taps on the envelope (hamming(492), the default argument of :677; pre_ntaps 0 = none)
 *      -> normalised correlation with the needle (:659-675) -> peak pick (:713-751) -- and
 *      returns per window: peak_host = picked index in the window, already minus needle_len/2
 *      (INT64_MIN if no sample exceeds the threshold); height_host = correlation at the peak
 *      (:762); tsync_host = mean of the envelope over the needle length following the sync
 *      (:755-757), NaN where the reference appends None.  Windows must be shorter than the
 *      0.45 s peak-group distance (true for getAccurateSync's windows at any sample rate);
 *      longer ones are DD_ERR_INVALID -- run them through the per-stage entry points.
 *      All taps / needle pointers are host float64.  Synchronous. */
int dd_noaa_sync_windows(const void* iq, int iq_kind, const int64_t* starts_host, int n_windows,
                         int64_t win_len, uint64_t cycles_q64,
                         const double* fir_taps_host, int fir_ntaps,
                         const double* pre_taps_host, int pre_ntaps,
                         const double* needle_host, int needle_len, double samp_rate,
                         int64_t* peak_host, double* height_host, double* tsync_host, void* stream);
/* ... the window lists of several sync words in one call (getAccurateSync, decode_noaa.py:828-835, searches sync A around the
 *      crude A positions and sync B around the crude B positions: two lists, one chain, two needles of one length).
 *      needle_host holds n_needles (1 or 2) needles of needle_len values back to back; needle_of_window_host[w] names the
 *      needle window w is correlated with (NULL: needle 0).  Results in window order.  One upload, one copy back. */
int dd_noaa_sync_windows_multi(const void* iq, int iq_kind, const int64_t* starts_host, const int* needle_of_window_host,
                               int n_windows, int64_t win_len, uint64_t cycles_q64,
                               const double* fir_taps_host, int fir_ntaps,
                               const double* pre_taps_host, int pre_ntaps,
                               const double* needle_host, int needle_len, int n_needles, double samp_rate,
                               int64_t* peak_host, double* height_host, double* tsync_host, void* stream);

/* dd_noaa_prepare -- builds ahead of time, ON THE HOST, what dd_noaa_crude_tail needs for `n` audio samples in blocks of `block` (0: nothing;
 * decode_noaa.py:647-653) and what dd_noaa_sync_windows needs for windows of `window` IQ samples (0: nothing; decode_noaa.py:823-825): the
 * Hilbert-kernel spectra of the block, of the ragged last block and of the window (closed forms and host transforms, ~12 ms each; no device call --
 * the call that needs a spectrum uploads it, 0.3 ms).  Optional: noaa_sync calls it from threads of their own when the decoder object is created,
 * beside the runtime's first copy, the upload and the audio chain.  `stream` is unused.  No reference counterpart (scipy.signal.hilbert plans
 * nothing ahead). */
int  dd_noaa_prepare(int64_t n, int64_t block, int64_t window, void* stream);
/* P -- getCrudeSync's audio-rate tail (decode_noaa.py:781-790) in one host call: the envelope of `audio` (device float32 or
 *      float64, n samples at samp_rate) in `block`-sample blocks by the chunker rule (__getAM :631-657 -> demod_am.py:29),
 *      then for each of n_needles (1 or 2: sync A and sync B, :786 and :790) piecewise-constant needles of m samples
 *      (needles_host[needle][m], host float64) the normalised correlation (:659-675) and the peak pick (:713-751).  Per
 *      needle d the picked indices -- ascending, already minus m / 2 -- land in peaks_host[d * max_peaks ...] and their
 *      number in n_peaks[d]; env_out (device float64[n], may be NULL) receives the envelope.  The index lists are those of
 *      dd_am_envelope_f64 + dd_xcorr_norm_f64 + dd_find_peaks_f64 called stage by stage.  DD_ERR_UNSUPPORTED (nothing done)
 *      for needles with more than 64 runs, more than 2048 expected peaks (~17 min of audio) or more than 65 536 samples
 *      above the threshold: take the staged route.  Synchronous. */
int dd_noaa_crude_tail(const void* audio, int audio_is_f32, int64_t n, double samp_rate, int64_t block,
                       const double* needles_host, int m, int n_needles, double* env_out,
                       int64_t* peaks_host, int max_peaks, int* n_peaks, void* stream);

/* ---- AFSK1200 correlators (decode_afsk1200.py:99-158) ------------ */
/* binary_filter[s] = mi^2 + mq^2 - si^2 - sq^2, the four sums over buffer_size samples
 * from s against tables_host[4][bs] = mark cos/sin, space cos/sin (:110-123); entries
 * s >= n - bs are 0 (:126).  Same operation order as the reference: float64 bit-exact. */
int dd_afsk_binary_filter_f64(const double* sig, int64_t n, const double* tables_host, int bs,
                              double* out, void* stream);
/* out = np.correlate(np.sign(binary_filter), [-1]*(spb/2) + [1]*(spb - spb/2), 'same') / spb (:147-156) */
int dd_afsk_edges_f64(const double* binary_filter, int64_t n, int spb, double* out, void* stream);

/* AFSK1200 frame logic behind the correlators (decode_afsk1200.py:160-269).
 * dd_peakdetect_f64 -- peakdetect.peakdetect(y, lookahead=L, delta) (decode_afsk1200.py:160): the lookahead state machine over
 *      y[0 .. n-L), exact for finite y (non-finite input: DD_ERR_INVALID).  Maxima (position, value) into max_pos / max_val, minima
 *      into min_pos / min_val (device, capacities cap_*; n/2 + 2 is always enough), the first hit popped as the reference does;
 *      counts_host[2] = how many of each.
 * dd_afsk_bits_f64 -- from the maxima positions peaks[m] (device) and binary_filter bf[n]: bit_repeated = rint(diff(peaks) / (bw/1200))
 *      (:189), per bit the mean of bf[x_i + r spb : x_i + (r+1) spb] in NumPy's summation order (:199-203; NaN for an empty slice),
 *      sgn = np.sign of it (NaN as 2), bits = decode_nrzi (:208), marks = find_bit_stuffing (:229), flags = the start-flag positions
 *      (:217-224).  Device outputs of capacity cap_bits / cap_flags; counts_host[2] = (bits, flags).
 * dd_afsk_frames_check -- per consecutive flag pair i (:236-251): info_host[2i] = the count of unstuffed bits between them,
 *      info_host[2i + 1] = 1 when the reference accepts it (count % 8 == 0, message > 128 bits, fcs_crc16 matches).
 * dd_afsk_frames_pack -- the message bytes (the unstuffed bits but the last 16, LSB first, bits_to_msg's order) of every pair with
 *      off_host[i] >= 0 to out + off_host[i] (device, out_bytes a multiple of 4, zeroed first). */
int dd_peakdetect_f64(const double* y, int64_t n, int64_t lookahead, double delta, int64_t* max_pos, double* max_val,
                      int64_t cap_max, int64_t* min_pos, double* min_val, int64_t cap_min, int64_t* counts_host, void* stream);
int dd_afsk_bits_f64(const double* bf, int64_t n, const int64_t* peaks, int64_t m, double bw, int spb, int64_t cap_bits,
                     double* mean, int8_t* sgn, int8_t* bits, int8_t* marks, int64_t* flags, int64_t cap_flags,
                     int64_t* counts_host, void* stream);
int dd_afsk_frames_check(const int8_t* bits, const int8_t* marks, int64_t nbits, const int64_t* flags, int64_t nflags,
                         int64_t* info_host, void* stream);
int dd_afsk_frames_pack(const int8_t* bits, const int8_t* marks, int64_t nbits, const int64_t* flags, int64_t nflags,
                        const int64_t* info_host, const int64_t* off_host, uint8_t* out, int64_t out_bytes, void* stream);

/* ---- Meteor-M2 QPSK sync detection (decode_meteorm2.py:229-324) ----------------------------------------------------
 * dd_meteor_mix -- out[k] = complex64(x[k] * (cos th, sin th)), th = (w * k) * inv_fs, w = -2 pi f: the reference's offsetFreq
 *     arithmetic in float64; x = raw u8 pairs - 127.5 (raw_u8) or complex64 (c64), exactly one of them given.
 * dd_meteor_walk -- the Gardner / agc / costas walk over x[n] (complex128, absolute sample index base + j), state in *state
 *     (DDMeteorState, carried from chunk to chunk), params_host = DDMeteorParams (7 doubles, then the 256-entry tanh table); both
 *     structs and the walk's body, which dd_funcube_walk shares, are in csrc/dd_symbol_walk.h.
 *     Symbol k (the walk's k-th A sample) writes bidx[k], aidx[k] (sample indices), agc[k] (agc output of A), ph[k] (the costas
 *     phasor active after the step), sym[k] (corrected symbol), pf[k] = (phase, freq) after the step; k >= cap sets the
 *     state's overflow flag instead.
 * dd_meteor_lim -- out[base + j] = (lim(real(x[j] * o) / 2), lim(imag(x[j] * o) / 2)) as int8 pairs, o the phasor of the last
 *     symbol with aidx < base + j (1 before the first).
 * dd_meteor_minsync -- bits[k] = limBin(re) | limBin(im) << 1 of sym[k]; for every k >= 59 whose 60-symbol window scores
 *     |mismatches - 60| > 30 against sync72khz (re, im order) or sync72khz1 (im, re order; sync_bits_host[120 ..]):
 *     cand[3c .. 3c+2] = (k, mismatches1, mismatches2), *count = the number of such k (entries past cap are dropped).
 * dd_meteor_maxcorr -- per buffer i (bufs_host[5i ..] = lo0, n0, lo1, n1, template: samples [lo0, lo0+n0) then [lo1, lo1+n1)
 *     of lim[lim_len], two entries each): out[2i] = argmax |np.correlate(buffer, np.repeat(templates[template], 28), 'same')|
 *     (first maximum), out[2i+1] = that maximum.  templates_host = int8[2][120]. */
int dd_meteor_mix(const void* raw_u8, const void* c64, int64_t n, double w, double inv_fs, void* out, void* stream);
int dd_meteor_walk(const void* x, int64_t n, int64_t base, void* state, const double* params_host, int64_t cap,
                   int64_t* bidx, int64_t* aidx, void* agc, void* ph, void* sym, void* pf, void* stream);
int dd_meteor_lim(const void* x, int64_t n, int64_t base, const int64_t* aidx, int64_t nsym, const void* ph, void* out,
                  int64_t out_len, void* stream);
int dd_meteor_minsync(const void* sym, int64_t nsym, const uint8_t* sync_bits_host, uint8_t* bits, int64_t cap,
                      int64_t* cand, unsigned long long* count, void* stream);
int dd_meteor_maxcorr(const void* lim, int64_t lim_len, const int64_t* bufs_host, int64_t nbuf, const int8_t* templates_host,
                      int64_t* out, void* stream);

/* ---- Meteor-M2 LRPT channel decoding (beyond the reference; DESIGN.md section 4.14 defines every stage) ---------------------
 * dd_lrpt_soft -- soft[2k], soft[2k+1] = lim(re(sym[k]) / 2), lim(im(sym[k]) / 2) as int8 (sym complex128, the walk's sym[]).
 * dd_lrpt_asm_search -- for every symbol p <= nsym - 32 and hypothesis h in 0..7: score = how many of the encoded sync marker's
 *     code bits 12..63 equal the hard bit 2p + j under h; every score >= min_score appends cand[3c .. 3c+2] = (p, h, score),
 *     *count = the number of such (p, h) (entries past cap are dropped).  The order of the entries is not defined.
 * dd_lrpt_viterbi -- per span i (spans_host[2i], [2i+1] = first symbol p, hypothesis h): the nbits input bits of the rate-1/2,
 *     K = 7 code's most likely path over the steps p .. p + nbits - 1, decoded in blocks of 512 steps with 128 steps of warm-up
 *     and tail, packed MSB first into bits_packed[i * nbits / 8 ..].  nbits a multiple of 512, h in 0..7, p + nbits <= nsym,
 *     at most 65535 spans per call.
 * dd_lrpt_finish -- per frame i (8192 bits of dd_lrpt_viterbi's output, the same spans): bodies[1020 i ..] = bytes 4..1023 XOR
 *     the CCSDS pseudo-noise sequence; info[3i .. 3i+2] = (marker bits in error, hard input bits of steps 6..8191 that differ
 *     from the re-encoded decoded bits, the virtual channel id = body[1] & 0x3F).
 * dd_lrpt_rs -- Reed-Solomon (255,223) correction (GF(256) modulo 0x187, roots (alpha^11)^j for
 *     j = 112..143, conventional basis, interleave depth 4) of the four codewords of each of nframes 1020-byte bodies:
 *     fixed[1020 i ..] = the body with every codeword that lies within 16 byte errors of a codeword replaced by it (parity
 *     included), the others as received; errors[4 i + w] = the bytes changed in codeword w (0..16), or -1 where it was left.
 * dd_lrpt_jpeg -- the image packets' payload (the two luminance Huffman tables of T.81 Annex K, no byte
 *     stuffing, 14 blocks per packet, the DC predictor 0 at the packet's start, the luminance quantiser scaled by q, an integer
 *     8x8 inverse transform).  Packet i's entropy-coded bytes are data[offsets_host[i] .. offsets_host[i+1]) (an empty range is
 *     allowed), q_host[i] its quality factor.  mcus[i] = the blocks decoded before the first failure (0..14, always written);
 *     block m < mcus[i] goes to the 8x8 bytes at out[dst_host[i] + 8 m + y * pitch + x]; dst_host[i] = -1 decodes without
 *     writing pixels.  pitch >= 112, offsets not decreasing, a packet below 2^27 bytes.  No byte past offsets_host[i+1] is read for packet i. */
int dd_lrpt_soft(const void* sym, int64_t nsym, int8_t* soft, void* stream);
int dd_lrpt_asm_search(const int8_t* soft, int64_t nsym, int min_score, int64_t cap, int64_t* cand, unsigned long long* count,
                       void* stream);
int dd_lrpt_viterbi(const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans, int64_t nbits,
                    uint8_t* bits_packed, void* stream);
int dd_lrpt_finish(const uint8_t* bits_packed, const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans,
                   uint8_t* bodies, int32_t* info, void* stream);
int dd_lrpt_rs(const uint8_t* bodies, int64_t nframes, uint8_t* fixed, int32_t* errors, void* stream);

/* ---- The LRPT modes of the Meteor-M N2-x satellites, from soft symbols (DESIGN.md section 4.18 defines every stage) ----------
 * dd_lrpt_asm_search_t -- dd_lrpt_asm_search against the 64-bit code word `encoded` (first code bit in bit 63) instead of the
 *     encoded sync marker; with encoded = 0x035D49C24FF2686B it finds what dd_lrpt_asm_search finds.
 * dd_lrpt_finish_nrzm -- dd_lrpt_finish for a differential (NRZ-M) stream: with v the frame's 8192 decoded bits, d[0] = 0 and
 *     d[i] = v[i] ^ v[i-1]; bodies = bytes 4..1023 of d XOR the pseudo-noise sequence; info = (bits 1..31 of d that differ from
 *     the marker, the re-encode count of v as dd_lrpt_finish gives it, the virtual channel id from d).
 * dd_lrpt_deint_scores -- the marker of the 80 ksym/s interleaver: for every symbol q <= nsym - 4 and hypothesis h, how many of
 *     the 8 hard bits from bit 2q under h equal those of 0x27 (MSB first), added into scores[((q / (40 seg)) * 40 + q % 40) * 8 + h].
 *     scores holds ceil(nsym / (40 seg)) * 320 values and is zeroed by the call; 1 <= seg <= 2^24.
 * dd_lrpt_deinterleave -- for the stream locked at symbol offset o (0..39) under hypothesis h: y[72 t + i] = rail i % 2 of symbol
 *     o + 40 t + 4 + i / 2 under h (128 stored as 127), t < (nsym - o) / 40; out pair k = (x[2k], x[2k+1]) with
 *     x[n] = y[n + branches * delay * (n % branches)], for n < N = 72 groups - branches * delay * (branches - 1) rounded down to even.
 *     *nsym_out (host) = N / 2, 0 when the stream does not fill the branches.  out has room for 36 * (nsym / 40) pairs.
 *     branches must divide 72, delay >= 0. */
int dd_lrpt_asm_search_t(const int8_t* soft, int64_t nsym, unsigned long long encoded, int min_score, int64_t cap, int64_t* cand,
                         unsigned long long* count, void* stream);
int dd_lrpt_finish_nrzm(const uint8_t* bits_packed, const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans,
                        uint8_t* bodies, int32_t* info, void* stream);
int dd_lrpt_deint_scores(const int8_t* soft, int64_t nsym, int64_t seg, int32_t* scores, void* stream);
int dd_lrpt_deinterleave(const int8_t* soft, int64_t nsym, int o, int h, int branches, int delay, int8_t* out, int64_t* nsym_out,
                         void* stream);
int dd_lrpt_jpeg(const uint8_t* data, const int64_t* offsets_host, const uint8_t* q_host, const int64_t* dst_host, int64_t npackets,
                 int64_t pitch, uint8_t* out, int32_t* mcus, void* stream);

/* ---- OQPSK demodulation for the Meteor-M N2-x satellites (beyond the reference; DESIGN.md section 4.19 defines every operation) ----
 * dd_oqpsk_walk -- the OQPSK symbol walk over x[n] (complex128, absolute sample index base + j): Gardner timing on both staggered
 *     rails of the derotated samples, agc (gain cap 200) and a Costas loop whose phase is kept in turns, in one serial chain with no
 *     libm call.  state = DDOqpskState (csrc/dd_oqpsk.h; 15 doubles, 5 int64), carried from chunk to chunk; params_host =
 *     DDMeteorParams with the loop gains in turns; table = device double[1024][2] = (cos, sin)(2 pi i / 1024).  Symbol k (the k-th B
 *     event after an A) writes bidx[k], aidx[k] (the samples its Q and its I were read at), sym[k] = (I, Q) and uf[k] = (phase in
 *     turns, frequency in turns per symbol) after its step; k >= cap sets the state's overflow flag instead.
 * dd_lrpt_restagger -- out pair j = (I[j + lead], Q[j + lead + s]) of the nsym soft pairs, lead = 1 for s = -1, else 0:
 *     nsym - |s| pairs (none for nsym <= |s|); s in -1, 0, 1. */
int dd_oqpsk_walk(const void* x, int64_t n, int64_t base, void* state, const double* params_host, const void* table, int64_t cap,
                  int64_t* bidx, int64_t* aidx, void* sym, void* uf, void* stream);
int dd_lrpt_restagger(const int8_t* soft, int64_t nsym, int s, int8_t* out, void* stream);

/* ---- G3RUH 9600 baud FSK (beyond the reference; DESIGN.md section 4.20 defines every operation) --------------------------------
 * dd_fsk_walk -- bit-timing recovery over FM-demodulated audio x[n] (float64, absolute sample index base + j): a dc tracker and a
 *     mean-|y| normaliser on every sample, linearly interpolated transition and eye samples, a clamped Gardner error; one serial
 *     chain of + - * / comparisons and fabs.  state = DDFskState (csrc/dd_fsk.h; 6 doubles t, dc, am, prev, mid, last and 2 int64
 *     ctr, overflow), carried from call to call; params_host = 4 doubles P, P / 2, P / 2 + 1, g with 2 <= P <= 64.  Symbol k writes
 *     sym[k] (the eye), sidx[k] (its sample) and tmu[k] (the timing after its update); k >= cap sets the state's overflow flag
 *     instead and ctr counts on.
 * dd_fsk_bits -- r[k] = sym[k] > 0, d[k] = r[k] ^ r[k-12] ^ r[k-17] (0 before the start), bits[0] = 1, bits[k] = (d[k] == d[k-1]);
 *     marks and flags as dd_afsk_bits_f64 gives them.  Device outputs int8[nsym] and flags[cap_flags]; counts_host[2] = (nsym, flags). */
int dd_fsk_walk(const double* x, int64_t n, int64_t base, void* state, const double* params_host, int64_t cap, double* sym,
                int64_t* sidx, double* tmu, void* stream);
int dd_fsk_bits(const double* sym, int64_t nsym, int8_t* r, int8_t* bits, int8_t* marks, int64_t* flags, int64_t cap_flags,
                int64_t* counts_host, void* stream);

/* ---- Slow-scan television, PD modes (beyond the reference; DESIGN.md section 4.21 defines every stage) ----------------------------
 * All float64, + - * / comparisons, ceil and rint, each rounded on its own; sstv.py restates every entry in NumPy.
 * dd_sstv_lag -- z[i] = sum over k < K of h[k] x[i - k] (x = 0 before the start; real and imaginary sums apart, k ascending),
 *     d[i] = z[i] conj(z[i - 1]) with z[-1] = 0, as n (re, im) pairs.  taps_host = K real parts, then K imaginary parts; K odd, <= 511.
 * dd_sstv_classes -- cls[i] in 0..4 (none, 1100, 1200, 1300 Hz, leader) from the angle of d[i] against six band edges,
 *     edges_host = six cosines then six sines, ascending angles in (0, pi): class j + 1 for [edge j, edge j + 1), j < 3, and 4 for
 *     [edge 4, edge 5); an imaginary part <= 0 and a NaN give 0.
 * dd_sstv_runs -- count(i) = how many of cls[i .. i + window) equal target, i <= n - window; every maximal run of count >= thresh
 *     gives one position, the first index of its largest count, in ascending order: pos[min(*count_host, cap)], *count_host = the
 *     number of runs.  More runs than cap: DD_ERR_INVALID with the count filled and nothing written past cap.  n < window: no runs.
 * dd_sstv_pixels -- per segment g < nseg and pixel p < W: a = ceil(t0[g] + p step), b = ceil(t0[g] + (p + 1) step), clipped to
 *     [0, n], D = d[a] + .. + d[b - 1] ascending, levels[g W + p] = clip(rint((angle(D) c1 - 1500) 255 / 800), 0, 255) with
 *     sstv.atan_host's polynomial angle (0 for a negative imaginary part), c1 = rate / 2 pi; an empty interval or D = 0 gives level 0
 *     and counts in *empty_host.  t0 is a device array.
 * dd_sstv_color -- levels[pair][4][W] = Y0, Cr, Cb, Y1 -> rgb[2 pair + row][W][3]: R = (100 Y + 140 Cr - 17850) / 100,
 *     G = (100 Y - 71 Cr - 33 Cb + 13260) / 100, B = (100 Y + 178 Cb - 22695) / 100, floor division, clipped to 0..255. */
int dd_sstv_lag(const double* x, int64_t n, const double* taps_host, int K, void* d, void* stream);
int dd_sstv_classes(const void* d, int64_t n, const double* edges_host, int8_t* cls, void* stream);
int dd_sstv_runs(const int8_t* cls, int64_t n, int target, int64_t window, int64_t thresh, int64_t* pos, int64_t cap,
                 int64_t* count_host, void* stream);
int dd_sstv_pixels(const void* d, int64_t n, const double* t0, int64_t nseg, int W, double step, double c1, uint8_t* levels,
                   int64_t* empty_host, void* stream);
int dd_sstv_color(const uint8_t* levels, int64_t npairs, int W, uint8_t* rgb, void* stream);

/* ---- 1090 MHz Mode S / ADS-B squitters (beyond the reference; DESIGN.md section 4.22 defines every stage) -------------------------
 * All integer; adsb.py restates every entry in NumPy.  iq = n raw uint8 (I, Q) pairs on the device, n < 2^28; rate = samples per
 * second, 2 000 000 .. 20 000 000; phases = candidates per sample, 1, 2, 4 or 8.  Candidate k starts k / phases samples into the
 * recording; its chip c covers rate / 2 000 000 samples from k / phases + c rate / 2 000 000 on; a chip's energy is the sum of
 * overlap * ((2 I - 255)^2 + (2 Q - 255)^2) with the overlaps in units of gcd(2 000 000 / phases, rate) / 2 000 000 sample.  The
 * candidates are the k >= 0 whose 240 chips end inside the recording.
 * dd_adsb_candidates -- the candidates that pass the preamble test (E0 > E1 < E2 > E3, E6 < E7 > E8 < E9 > E10, and 6 E[q] <
 *     E0 + E2 + E7 + E9 for q = 4, 5, 11, 12, 13, 14; all strict) in ascending order: list[min(*count_host, cap)], *count_host =
 *     how many passed.  More than cap: DD_ERR_INVALID with the count filled and nothing written past cap.
 * dd_adsb_demod -- per listed candidate c < m: bit b = E[16 + 2 b] > E[17 + 2 b], DF = bits 0..4, L = 112 for DF >= 16 else 56,
 *     rem = the remainder of the L-bit word by 0x1FFF409, score = the sum over b < L of |E[16 + 2 b] - E[17 + 2 b]|; for L = 112
 *     and DF 17 or 18, a rem equal to the remainder of one lone bit at a position >= 5 gives fixed = that position and flips the
 *     bit, else fixed = -1.  frames[14 c ..] = the word, zero beyond L; meta[4 c ..] = L, DF, rem, fixed; score[c].  list, frames,
 *     meta and score are device arrays.  A k that is no candidate of the recording gives zeros and fixed = -1. */
int dd_adsb_candidates(const void* iq, int64_t n, int64_t rate, int phases, int64_t* list, int64_t cap, int64_t* count_host,
                       void* stream);
int dd_adsb_demod(const void* iq, int64_t n, int64_t rate, int phases, const int64_t* list, int64_t m, uint8_t* frames,
                  int32_t* meta, int64_t* score, void* stream);

/* ---- AIS, 9600 baud GMSK bursts carrying HDLC frames (beyond the reference; DESIGN.md section 4.23 defines every stage) -----------
 * ais.py restates every entry in NumPy.  audio = n float64 discriminator outputs (radians per sample) on the device, n < 2^31;
 * sps = samples per bit, 4 .. 16; w = samples summed per bit value, odd, 1 .. 15.  q[i] = rint(audio[i] * (2^20 / pi)) as an integer
 * (0 for a NaN and beyond +-2^21), 0 outside the audio; everything behind it is integer.  v(t, k) = the sum of the w samples q
 * around sample floor(t + (k + 0.5) sps), the product and the sum rounded one by one in float64.  S(t) = v(t, 0) + .. + v(t, 15);
 * the level of bit k is + when 16 v(t, k) > S(t), strictly.  The template is (- - + +) x 4, seven -, one +: the last 16 training bits
 * and the start flag after NRZI.  The starts are the t >= 0 with floor(23.5 sps) + w / 2 < n - t.
 * dd_ais_candidates -- the starts whose 24 levels equal the template, or its negation, in all but at most `slack` places (0 .. 11),
 *     in ascending order: list[min(*count_host, cap)], *count_host = how many passed.  More than cap: DD_ERR_INVALID with the count
 *     filled and nothing written past cap.
 * dd_ais_demod -- per listed start c < m: 1280 levels at k = 24 .., bit i = 1 where level i repeats level i - 1 (NRZI; level -1 is
 *     template bit 23); e = the start of the first run of six 1s; status 1 (no end flag) without one or when bit e + 6 lies past the
 *     1280, 2 (abort) when bit e + 6 is 1; the data are the bits before e - 1 less every 0 that follows five 1s; status 3 (stuffing
 *     violation) when five 1s end at e - 2, 4 (bad length) unless the count is a multiple of 8 and at least 40, 5 (bad CRC) unless
 *     the CRC-16 register (reflected 0x8408, preset 0xFFFF) over all of them ends at 0xF0B8, else 0 (accepted).
 *     frames[160 c ..] = the data bits, the first in bit 0 of byte 0 (AIS sends a byte's lowest bit first: these are the message's
 *     bytes and its FCS), zero beyond the count and for status 1 and 2; meta[4 c ..] = status, bit count, CRC register (status 0 and
 *     5, else 0), polarity (1 when the levels are nearer the negated template); score[c] = the sum over the template of
 *     |16 v - S|.  list, frames, meta and score are device arrays.  A start outside [0, n) gives status 1 and zeros. */
int dd_ais_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap, int64_t* count_host,
                      void* stream);
int dd_ais_demod(const double* audio, int64_t n, double sps, int w, const int64_t* list, int64_t m, uint8_t* frames, int32_t* meta,
                 int64_t* score, void* stream);

/* ---- POCSAG paging, 2-FSK at 512 / 1200 / 2400 baud (beyond the reference; DESIGN.md section 4.24 defines every stage) ------------
 * pocsag.py restates every entry in NumPy.  audio, n, q and v(t, k) as for AIS above, with sps = samples per bit, 4 .. 128, and w
 * odd, 1 .. 77.  S(t) = v(t, 0) + .. + v(t, 31); bit k of the start t is 0 when 32 v(t, k) > S(t), strictly (the higher frequency
 * is a 0), else 1.  A codeword holds its first-sent bit in bit 31.  The starts are the t >= 0 with floor(31.5 sps) + w / 2 < n - t.
 * dd_pocsag_candidates -- the starts whose 32 bits equal the frame sync codeword 0x7CD215D8, or its inverse, in all but at most
 *     `slack` places (0 .. 8), in ascending order: list[min(*count_host, cap)], *count_host = how many passed.  More than cap:
 *     DD_ERR_INVALID with the count filled and nothing written past cap.
 * dd_pocsag_batches -- per listed start c < m: the 544 bits k = 0 .. 543 against S(t) of the first 32, inverted when more than 16
 *     of those differ from the sync codeword (polarity 1).  Codewords 1 .. 16: the syndrome of bits 31 .. 1 modulo x^10 + x^9 + x^8 +
 *     x^6 + x^5 + x^3 + 1 (0x769); 0: no error there; that of one bit: the bit is flipped; that of two bits: both are flipped; else
 *     uncorrectable.  Odd parity over the 32 bits after that flips bit 0 and counts as one more error.  A codeword with more than
 *     `fix` (0 .. 2) errors is uncorrectable.  words[17 c ..] = codeword 0 as received and the others corrected, or as received where
 *     uncorrectable; errs[17 c ..] = the sync codeword's wrong places, then the errors repaired per codeword, 255 = uncorrectable;
 *     meta[4 c ..] = status, polarity, how many of the 16 were accepted, errs[17 c]; score[c] = the sum over the sync codeword of
 *     |32 v - S|.  list, words, errs, meta and score are device arrays.  A start outside [0, n) gives status 1 and zeros. */
int dd_pocsag_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap,
                         int64_t* count_host, void* stream);
int dd_pocsag_batches(const double* audio, int64_t n, double sps, int w, int fix, const int64_t* list, int64_t m, uint32_t* words,
                      uint8_t* errs, int32_t* meta, int64_t* score, void* stream);

/* ---- ACARS on VHF, 2400 baud MSK on 1200 / 2400 Hz over AM (beyond the reference; DESIGN.md section 4.25 defines every stage) -----
 * acars.py restates every entry in NumPy.  audio = n float64 samples of the AM envelope on the device, n < 2^31; sps = samples per
 * bit, 8 .. 64; w = samples summed on either side of a bit's end, 1 .. 32.  q[i] = rint(audio[i] * 2^12) as an integer (0 for a NaN
 * and beyond +-2^21), 0 outside the audio; everything behind it is integer.  B(t, k) = floor(t + (k + 1) sps), the product and the
 * sum rounded one by one in float64; v(t, k) = (q[B] + .. + q[B + w - 1]) - (q[B - w] + .. + q[B - 1]); bit k of the start t is 1
 * when v(t, k) > 0, strictly.  The template is 0x54686880, * SYN SYN SOH with each character's lowest bit first and the first-sent
 * bit in bit 31.  The starts are the t >= 0 with t + floor(32 sps) + w <= n.
 * dd_acars_candidates -- the starts whose 32 bits equal the template, or its inverse, in all but at most `slack` places (0 .. 5), in
 *     ascending order: list[min(*count_host, cap)], *count_host = how many passed.  More than cap: DD_ERR_INVALID with the count
 *     filled and nothing written past cap.
 * dd_acars_blocks -- per listed start c < m: the 1920 bits k = 32 .. 1951, all inverted when more than 16 of the first 32 differ from
 *     the template (polarity 1); bit p = k - 32 is bit p mod 8 of character p / 8.  e = the least character index from 12 on that holds
 *     0x83 or 0x97 with e + 2 <= 239; without one status 2 (no end).  s = the CRC-16 register (reflected 0x8408, preset 0) over
 *     characters 0 .. e + 2; c = the characters among 0 .. e with an even number of ones.  s = 0: accepted.  Else, with fix >= 1 and
 *     c = 1, the one bit of that character whose flip clears s is flipped; with fix >= 1 and c = 0 the one such bit of characters
 *     e + 1 and e + 2; with fix >= 2 and c = 2 the one pair of a bit of the first such character and a bit of the second, when exactly
 *     one pair clears s; anything else is status 3 (bad block check).  bytes[240 c ..] = the characters, repaired where accepted;
 *     meta[8 c ..] = status (0 accepted), polarity, the template's wrong places, e (-1 without), c, bits repaired, whether character
 *     e + 3 is 0x7F, s as received; score[c] = the sum over the template of |v|.  list, bytes, meta and score are device arrays.
 *     A start outside [0, n) gives status 1, e = -1 and zeros. */
int dd_acars_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap, int64_t* count_host,
                        void* stream);
int dd_acars_blocks(const double* audio, int64_t n, double sps, int w, int fix, const int64_t* list, int64_t m, uint8_t* bytes,
                    int32_t* meta, int64_t* score, void* stream);

/* ---- Vaisala RS41 radiosonde telemetry, 2-GFSK at 4800 baud (beyond the reference; DESIGN.md section 4.26 defines every stage) ------
 * rs41.py restates every entry in NumPy.  audio, n, q and v(t, k) as for AIS above, with sps = samples per bit, 4 .. 64, and w odd,
 * 1 .. 39.  The header on the air is 10 B6 CA 11 22 96 12 F8, each byte's lowest bit first: 25 ones and 39 zeros among the places
 * k = 0 .. 63.  S1(t) = the sum of v(t, k) over the one-places, S0(t) over the zero-places; a bit k of the start t is high when
 * 1950 v(t, k) > 39 S1(t) + 25 S0(t) and low when 1950 v(t, k) < 39 S1(t) + 25 S0(t), both strictly.  Polarity 0 reads high as 1 and
 * anything else as 0; polarity 1 reads low as 1 and anything else as 0.  The starts are the t >= 0 with floor(63.5 sps) + w / 2 < n - t.
 * dd_rs41_candidates -- the starts whose 64 bits equal the header in all but at most `slack` places (0 .. 11) in polarity 0 or, failing
 *     that, in polarity 1, in ascending order: list[min(*count_host, cap)], *count_host = how many passed.  More than cap:
 *     DD_ERR_INVALID with the count filled and nothing written past cap.
 * dd_rs41_frames -- per listed start c < m: the polarity is 1 when the header has fewer wrong places in polarity 1 than in polarity 0;
 *     byte i of the frame is bits 8 i .. 8 i + 7, the first-sent in bit 0, XOR MASK[i mod 64] (section 4.26).  The frame is 518 bytes
 *     long when byte 56 as received is nearer in Hamming distance to F0 than to 0F and floor(t + 4143.5 sps) + w / 2 < n, else 320.
 *     Codeword j (0, 1): c_p = frame[8 + 24 j + p] for p < 24 and frame[56 + 2 (p - 24) + j] from there on while the frame lasts, 0
 *     behind it; RS(255,231) over GF(2)[x]/0x11D, alpha = 2, roots alpha^0 .. alpha^23: the codeword within 12 bytes that changes no
 *     byte behind the frame's end, or none.  fixed[518 c ..] = the frame with the decodable codewords corrected, recv[518 c ..] = the
 *     frame as received, both zero past the length; meta[6 c ..] = status, polarity, length, the header's wrong places, the bytes
 *     changed in codeword 0 and in codeword 1 (-1: none within reach).  list, fixed, recv and meta are device arrays.  A start outside
 *     [0, n), or with floor(t + 2559.5 sps) + w / 2 >= n, gives status 1 and zeros. */
int dd_rs41_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap, int64_t* count_host,
                       void* stream);
int dd_rs41_frames(const double* audio, int64_t n, double sps, int w, const int64_t* list, int64_t m, uint8_t* fixed, uint8_t* recv,
                   int32_t* meta, void* stream);

/* ---- RDS on broadcast FM, 1187.5 bit/s differential biphase on 57 kHz (beyond the reference) ---------------
 * rds.py restates every entry in NumPy.  mpx is the FM discriminator's float64 output in radians per sample at R S/s;
 * q = rint(mpx * 2^15 / pi), 0 for a NaN and beyond +-2^15.
 * dd_rds_baseband -- b[2 o], b[2 o + 1] = (the sum over i < D of q[o D + i] * table[phase(n0 + o D + i)]) >> 10 (arithmetic, of the
 *     int64 sum) for o < n / D; a tail shorter than D is dropped.  phase(j) = bits 31 .. 22 of (j * step) mod 2^32, step =
 *     rint(57000 * 2^32 / R); table = 1024 int32 pairs rint(2^14 exp(-2 pi i (j + 1/2) / 1024)), 1 <= D <= 32.  |b| <= 2^24.
 * With sps = baseband samples per bit, 12 .. 32, h = floor(sps / 2) and m pairs of b: z[p] = the sum of b[p .. p + h - 1] less the sum
 * of b[p - h .. p - 1] for h <= p <= m - h, else 0; p_k(t) = floor((t + k sps) + 0.5), each operation rounded to float64; bit k of the
 * start t is 1 iff Re(z[p_k] conj(z[p_(k-1)])) < 0 (int64), k = 0 .. 103, first-sent first into four blocks of 26 bits.  A block is
 * clean for an offset word iff block mod 0x5B9 equals it: A 0FC, B 198, C 168, C' 350, D 1B4.  A start fits when 0 <= t < m,
 * p_-1 >= 0 and p_103 <= m - h.
 * dd_rds_candidates -- the starts that fit with at least `clean` (2 .. 4) clean blocks, the four tested against A, B, C or C', D, in
 *     ascending order: list[min(*count_host, cap)], *count_host = how many passed.  More than cap: DD_ERR_INVALID with the count
 *     filled and nothing written past cap.
 * dd_rds_groups -- per listed start c < count: a block that is not clean is repaired when exactly one burst of at most `fix` bits
 *     (0 .. 5, a burst begins and ends in a wrong bit) makes it clean.  The third block is held against C' when the second, after
 *     its repair, has bit 11 of its information word set, against C when not; if the second is not decodable, against whichever of
 *     the two it is clean for, and C if neither.  words[4 c ..] = the four 16-bit information words (as received where not
 *     decodable); meta[8 c ..] = four statuses (0 clean, n bits repaired, -1 not decodable), the third offset word (0 C, 1 C'), the
 *     metric = the sum over the bits of min(|Re| >> 20, 2^24) <= 104 * 2^24, 0, the blocks decoded.  A start that does not fit gives
 *     zeros, statuses of -1 and meta[8 c + 6] = 1.  b, list, words and meta are device arrays. */
int dd_rds_baseband(const double* mpx, int64_t n, int D, uint64_t n0, uint64_t step, const int32_t* table, int32_t* b, void* stream);
int dd_rds_candidates(const int32_t* b, int64_t m, double sps, int clean, int64_t* list, int64_t cap, int64_t* count_host, void* stream);
int dd_rds_groups(const int32_t* b, int64_t m, double sps, int fix, const int64_t* list, int64_t count, uint16_t* words, int32_t* meta,
                  void* stream);

/* ---- FM stereo audio from the multiplex: pilot, 38 kHz subcarrier, de-emphasis (beyond the reference) -------
 * fmstereo.py restates every entry in NumPy.  mpx, q and table as for RDS above; phase19(j) = bits 31 .. 22 of (j * step19) mod 2^32
 * with step19 = rint(19000 * 2^32 / R), phase38 the same of step38 = 2 step19 mod 2^32.  All shifts are arithmetic, all divisions floor.
 * dd_fms_pilot -- P[2 k], P[2 k + 1] = (the sum over i < 256 of q[256 k + i] * table[phase19(256 k + i)]) >> 10 for k < n / 256 (a tail
 *     shorter than a block is dropped).  |P| <= 2^27.
 * dd_fms_carrier -- per block k < nb: S[k] = (the sum of P[j] over |j - k| <= 8, 0 <= j < nb) >> 8 (int64 sums, stored as int32 pairs),
 *     cnt = the blocks summed; lock[k] = 1 iff |S|^2 > 0 and |S|^2 >= thr * cnt^2 (0 <= thr <= 2^48), else 0; u[2 k], u[2 k + 1] =
 *     -((Sr^2 - Si^2) << 14) / |S|^2 and -((2 Sr Si) << 14) / |S|^2 when locked, (0, 0) when not: exp(2 i delta) in Q14, delta the
 *     pilot's phase against the table's.  P must be as dd_fms_pilot gives it (|P| <= 2^27) for the sums to fit.
 * dd_fms_audio -- with u of nb blocks and the block of sample j = min(j / 256, nb - 1) (nb = 0: u = 0 everywhere), (tr, ti) =
 *     conj(table[phase38(j)]): c = (tr ui + ti ur) >> 14, c2 = (c G) >> 12 (0 <= G <= 12288), a[j] = (q[j] (2^14 + c2)) >> 8,
 *     b[j] = (q[j] (2^14 - c2)) >> 8; out[2 o] = (the sum over i < ntaps of taps[i] a[o D + d0 - i]) >> 15, out[2 o + 1] the same of b,
 *     for o < ceil(n / D); samples outside [0, n) count as 0.  1 <= ntaps <= 1024, 1 <= D <= 12, 0 <= d0 < ntaps; the sum of |taps|
 *     must not exceed 2^17 (sums below 2^41, outputs below 2^26).  mpx, table, u, taps (int32) and out are device arrays. */
int dd_fms_pilot(const double* mpx, int64_t n, uint64_t step19, const int32_t* table, int32_t* P, void* stream);
int dd_fms_carrier(const int32_t* P, int64_t nb, int64_t thr, int32_t* S, int32_t* u, uint8_t* lock, void* stream);
int dd_fms_audio(const double* mpx, int64_t n, uint64_t step38, const int32_t* table, const int32_t* u, int64_t nb, int G,
                 const int32_t* taps, int ntaps, int D, int d0, int32_t* out, void* stream);

/* ---- Funcube BPSK sync detection (decode_funcube.py:148-306) ------------------------------------------------------------
 * dd_funcube_mix_ramp -- dd_meteor_mix with the frequency formed per sample: th = ((w * f[k]) * k) * inv_fs, w = -2 pi,
 *     f[k] = f0 + k * delta (np.arange's fill) clipped to target from above when target > f0, from below otherwise.
 * dd_funcube_lowpass -- scipy.signal.lfilter(b, a, x, zi) of complex64 x into complex128 out, sample by sample in lfilter's own
 *     operation order (bit for bit its output); ncoef = 7 with a[0] = 1 (butter's sixth order); state = device double[2][6],
 *     the real and the imaginary parts' delays, read on entry and left for the next chunk.
 * dd_funcube_walk -- dd_meteor_walk with decode_funcube's agc (gain cap 20) and costas (error imag * hyp(real) / 255); the same
 *     state, parameters and per-symbol outputs.  ph[k] is the phasor symbol k was corrected with, which is pllObj.output after it.
 * dd_funcube_lim -- out[base + j] = lim(real(x[j] * o) / 2) as int8, o the phasor of the last symbol with aidx < base + j
 *     (1 before the first).
 * dd_funcube_minsync -- bits[k] = limBin(real(sym[k])); for every k >= 329 whose 330-symbol window has |mismatches - 165| > 120
 *     against the 33 sync bits (sync_bits_host), each ten symbols long: cand[2c], cand[2c+1] = (k, mismatches), *count = the
 *     number of such k (entries past cap are dropped).
 * dd_funcube_maxcorr -- per buffer i (bufs_host[5i ..] = lo0, n0, lo1, n1, scratch offset: samples [lo0, lo0+n0) then
 *     [lo1, lo1+n1) of lim[lim_len]): out[2i] = argmax |np.correlate(buffer, np.repeat(t, rep), 'same')| (first maximum),
 *     out[2i+1] = that maximum, t = 127 / -128 per sync bit.  Each buffer's n0 + n1 + 1 int32 prefix sums go to
 *     scratch[offset ..]; the ranges must not overlap. */
int dd_funcube_mix_ramp(const void* raw_u8, const void* c64, int64_t n, double w, double f0, double delta, double target,
                        double inv_fs, void* out, void* stream);
int dd_funcube_lowpass(const void* in_c64, void* out_c128, int64_t n, const double* b_host, const double* a_host, int ncoef,
                       double* state, void* stream);
int dd_funcube_walk(const void* x, int64_t n, int64_t base, void* state, const double* params_host, int64_t cap,
                    int64_t* bidx, int64_t* aidx, void* agc, void* ph, void* sym, void* pf, void* stream);
int dd_funcube_lim(const void* x, int64_t n, int64_t base, const int64_t* aidx, int64_t nsym, const void* ph, int8_t* out,
                   int64_t out_len, void* stream);
int dd_funcube_minsync(const void* sym, int64_t nsym, const uint8_t* sync_bits_host, uint8_t* bits, int64_t cap,
                       int64_t* cand, unsigned long long* count, void* stream);
int dd_funcube_maxcorr(const int8_t* lim, int64_t lim_len, const int64_t* bufs_host, int64_t nbuf, const uint8_t* sync_bits_host,
                       int rep, int32_t* scratch, int64_t scratch_len, int64_t* out, void* stream);

/* ---- Funcube telemetry frames (beyond the reference; DESIGN.md section 4.17 defines every stage) ----------------------------
 * dd_fc_diff -- r[k] = soft[2k] (dd_lrpt_soft's pairs of the walk's nsym symbols), S[i] = r[i] + .. + r[i+9]; for i < nsym - 19,
 *     with a = S[i+10], b = S[i]: D[i] = 0 when a or b is 0, else +-min(min(|a|, |b|) / 10, 127), + where the signs differ.
 *     nsym < 20 writes nothing.
 * dd_fc_sync_search -- for every position p <= m - 51991 of D[m]: C = sum over k < 65 of (2 V[k] - 1) D[p + 800 k], V the sync
 *     vector; score = how many k have (D > 0), or (D < 0) when C < 0, equal to V[k]; every score >= min_score appends
 *     cand[3c .. 3c+2] = (p, C, score), *count = the number of such p (entries past cap are dropped).  The order is not defined.
 * dd_fc_viterbi -- per frame i (frames_host[2i], [2i+1] = position p, polarity inv in 0..1; 0 <= p <= m - 51991): the 5132 soft
 *     code values +-D[p + 10 pos(j)] through the 80 x 65 interleaver, the terminated rate-1/2, K = 7 trellis of 2566 steps from
 *     state 0 to state 0, blocks[320 i ..] = the first 2560 decoded bits packed MSB first XOR the CCSDS pseudo-noise sequence,
 *     corrected[i] = how many of the 5132 hard bits differ from the re-encoded decoded bits.
 * dd_fc_rs -- per block i: codeword c in 0..1 is blocks[320 i + c + 2 k], k < 160, decoded as dd_lrpt_rs's (255,223) code behind
 *     95 zero bytes; frames[256 i + c + 2 k], k < 128, = its data bytes, corrected where it decoded and as received where not;
 *     errors[2 i + c] = the bytes changed (0..16), or -1 (no codeword within 16 errors, or one with a non-zero byte among the 95). */
int dd_fc_diff(const int8_t* soft, int64_t nsym, int8_t* D, void* stream);
int dd_fc_sync_search(const int8_t* D, int64_t m, int min_score, int64_t cap, int64_t* cand, unsigned long long* count, void* stream);
int dd_fc_viterbi(const int8_t* D, int64_t m, const int64_t* frames_host, int64_t nframes, uint8_t* blocks, int32_t* corrected,
                  void* stream);
int dd_fc_rs(const uint8_t* blocks, int64_t nframes, uint8_t* frames, int32_t* errors, void* stream);

/* APT image extraction (decode_noaa.getImage / getColor).
 * dd_median_segments_f64 -- out[i] = np.median(src[off_host[i] : off_host[i] + len_host[i]]) for `count` segments (device out):
 *      numpy's semantics (odd: middle element, even: (a + b) / 2, empty or holding a NaN: NaN); segments of any length.
 * dd_apt_lines_f64 -- half-line h is the len_host[h] envelope samples at env + start_host[h]: scipy.signal.resample to
 *      num = (len / 1040) * 1040 into work (sum of num doubles, half after half), then pix[h][p] = median of the k = num / 1040
 *      values of pixel p (pix: nhalf x 1040; NaN when k = 0).  sync_off_host[2h], [2h + 1]: element offsets into sync_stream where
 *      the k values of each of pixels 0 .. sync_bits-1 go, pixel after pixel, to the low (bit of sync_mask clear) or the high part
 *      (bit set); -1 = none.
 * dd_apt_map_u8 -- out = clip(rint(v), 0, 255) as uint8 per row r of pix (nrows x row_len), with par_host[r] = (mode, a, b):
 *      mode 0: v = 255 * (x - a) / (b - a); mode 1: v = x * a + b (numpy's operation order, no fused multiply-adds).
 * dd_apt_color_u8 -- the false colour of getColor: v = img[r][c], t = img[r][1040 + c] (c < 1040) -> out[r][c][3] (RGB),
 *      colorsys.hsv_to_rgb and int(k * 255.0) in the reference's operation order. */
int dd_median_segments_f64(const double* src, const int64_t* off_host, const int64_t* len_host, int count, double* out, void* stream);
int dd_apt_lines_f64(const double* env, int64_t n_env, const int64_t* start_host, const int64_t* len_host, int nhalf,
                     const int64_t* sync_off_host, uint64_t sync_mask, int sync_bits, double* work, double* pix,
                     double* sync_stream, void* stream);
int dd_apt_map_u8(const double* pix, int64_t nrows, int row_len, const double* par_host, uint8_t* out, void* stream);
int dd_apt_color_u8(const uint8_t* img, int64_t nrows, int row_len, uint8_t* out, void* stream);

/* np.abs for demod_am.demod_amFLT (demod_am.py:35-62: butter low-pass of |sig|).
 * kind 0: float64, 1: complex128, 2: complex64 input; float64 output (hypot). */
int dd_abs_f64(const void* in, int kind, double* out, int64_t n, void* stream);

/* float32 -> float64 / complex64 -> complex128 widening (audio-rate hand-over) */
int dd_f32_to_f64(const float* in, double* out, int64_t n, void* stream);
int dd_f64_to_f32(const double* in, float* out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIRECTDEMOD_HIP_H */
