/*
 * directdemod_hip_debug.h -- diagnostic entry points of libdirectdemod_hip.so (round 6: moved out of the public header
 * directdemod_hip.h).  Used by the test suite and the tools under tools/ only: forcing one of several kernels
 * that compute the same thing (A/B runs, parity of every kernel against the oracle), filling LDS with a pattern, withholding an
 * in-launch hand-over, and the host arithmetic of launch plans (checked without a GPU).  No reference counterpart; not part of
 * the drop-in boundary.
 */
#ifndef DIRECTDEMOD_HIP_DEBUG_H
#define DIRECTDEMOD_HIP_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* diagnostic: fill the LDS of every compute unit with `pattern` (LDS is not cleared between workgroups).  The parity
 * suite runs the chain kernels after a NaN fill and after a zero fill and requires bit-identical outputs. */
int  dd_debug_fill_lds(uint32_t pattern, void* stream);
/* diagnostic: force one of the M = 1 chain kernels for every later launch of this process -- "ab" (k_chain_mfma_ab), "fft1k" (k_chain_fft1k, wherever it applies), "cos1k" (k_chain_cos1k where it applies -- 255 taps of a
 * two-term cosine series -- and the choice by tap class elsewhere), "decimp" (M > 1: the tile kernels of rounds 1-4 instead of
 * k_chain_decim_b / k_chain_decim_w; M = 1: by tap class but without k_chain_cos1k), "auto" / NULL (by tap class, the default).  The parity,
 * full-size and determinism suites run both FM kernels this way; the environment variable DD_MFMA_KERNEL seeds the choice
 * once per process.  No reference counterpart. */
int  dd_debug_select_kernel(const char* name);
/* diagnostic: the NEXT chunk-list launch withholds the hand-over flag of chunk `withhold_chunk` (>= 0; -1: none) and every
 * later one bounds its in-launch waits by 2^spin_log2 polls (0: the default, 2^19 = about a tenth of a second per wait).  Lets a test see DD_ERR_TIMEOUT
 * instead of silently wrong samples.  No reference counterpart (the reference's chunk loop is sequential, decode_noaa.py:619-624). */
int  dd_debug_seam(int withhold_chunk, int spin_log2);
/* diagnostics that need no GPU (host arithmetic of two launch paths, checked by the CPU test suite):
 * dd_debug_fft1k_plan -- the block grid and the block -> wave map of a k_chain_fft1k launch over a chunk of L samples (s = 1: a
 *   stream start, no angle for the first output; out_align_elems: how many elements `out` sits behind a 64-byte line; ncu compute
 *   units; rounds: 0 = default).  out[0..6] = base, nblk, grid, nwaves, K, b, 32, then r0[32], r1[32], wstart[32].
 * dd_debug_cos_fit -- 1 when the taps are a cosine series of at most four terms for which the zero-phase filter of the
 *   accurate-sync windows takes its prefix-sum form (a[0..3], *Q filled), else 0.
 * dd_debug_sync_envelope -- the envelope stage of dd_noaa_sync_windows alone: X_dev c64 [nwin][L] (device) -> env_dev f64
 *   [nwin][L - 1] = abs(hilbert(angle(X[n+1] conj X[n]))) (decode_noaa.py:852 -> demod_am.py:29).  route 0: the three-launch
 *   float64 transform of csrc/dd_hconv_kernels.h (512 x 512 for 65 536 < L <= 131 072, 512 x 256 for 32 768 < L <= 65 536), route 1: the FFT
 *   library's padded real transforms. */
int  dd_debug_fft1k_plan(int64_t L, int s, int out_align_elems, int ncu, int rounds, int* out);
/* dd_debug_cos1k_plan -- the row grid of a k_chain_cos1k launch (same arguments): out[0..3] = base (first sample of row 0; row q covers
 *   samples [base + 1024 q, +1024)), rows, workgroups, waves (wave w takes rows [rows w / waves, rows (w + 1) / waves)). */
int  dd_debug_cos1k_plan(int64_t L, int s, int out_align_elems, int ncu, int* out);
/* dd_debug_cos1k_shape -- a test door, not a tuning knob: every later k_chain_cos1k launch of this process runs on `nwaves` waves (a
 *   multiple of 4: nwaves / 4 workgroups; 0: the plan's own) with runs of `run_rows` rows dealt to the waves in turn (0: the launch
 *   path's own rule), so that a chunk of a few dozen rows walks the run map that otherwise needs 2^25 samples.  0, 0 restores the default.
 * dd_debug_cos1k_runs -- what a launch over `nrows` rows takes, given the plan's `nwaves`: out[0..2] = workgroups, waves, run length
 *   (0: one run per wave, rows [rows w / waves, rows (w + 1) / waves)), the override included where one is set.  Host arithmetic. */
int  dd_debug_cos1k_shape(int nwaves, int run_rows);
int  dd_debug_cos1k_runs(int nrows, int nwaves, int* out);
/* dd_debug_decimw_plan -- the row grid of a k_chain_decim_w / k_chain_decim_b launch over a chunk that starts at absolute sample abs0 with
 *   decimation phase off and keeps Ld samples: out[0..11] = R0 (absolute index of the first row: row R is the block of 2048 samples
 *   [2048 R, 2048 (R + 1))), rows, phi = (abs0 + off) mod M, samples kept in LDS in front of a block, start shift (0 / 1), taps per lane
 *   rounded up to 16 (window form), waves per CU, rows per run, form (1: block sums, k_chain_decim_b, K <= 8 M; 0: one window per lane,
 *   k_chain_decim_w), partial sums per output ceil(K / M), first block sample of the second accumulator set, samples of the LDS image.
 *   DD_ERR_UNSUPPORTED when the kernels do not take (K, M). */
int  dd_debug_decimw_plan(int64_t abs0, int64_t Ld, int K, int M, int off, int ncu, int64_t* out);
/* dd_debug_decim_tile_plan -- the tile grid of a k_chain_decim / k_chain_decim_p / k_chain_decim_multi launch over a chunk of L samples
 *   through K taps and decimation M >= 2 with decimation phase off (fm: FM output, has_last: an FM sample precedes the chunk; u8: raw u8
 *   input; in_align_bytes: the input pointer's address modulo 16): out[0..8] = T (FIR outputs per tile), tiles, S (samples a tile stages),
 *   S2 (S rounded up to whole 16-byte loads), persistent (1: the interior run goes to persistent workgroups, DD_KERNEL_DECIM_PERSISTENT;
 *   0: every tile through k_chain_decim, DD_KERNEL_DECIM_TILES), lo, hi (the interior run [lo, hi): the tiles staged with unconditional
 *   16-byte loads over the whole of S2; lo = hi = tiles when there is none), dynamic LDS bytes of k_chain_decim, and of the persistent
 *   launch.  DD_ERR_INVALID where the launch refuses (a tile beyond 160 KB of LDS) and for arguments no launch takes. */
int  dd_debug_decim_tile_plan(int64_t L, int K, int M, int off, int fm, int has_last, int u8, int in_align_bytes, int64_t* out);
/* dd_debug_decimb_lds_check --k_chain_decim_b's LDS image for K taps, decimation M and stream phase phi (absolute index of the first kept
 *   sample mod M), evaluated on the host with the kernel's own address functions: a run starts from a row before it whose first kept
 *   sample sits at offset phi (staged in part, no halo; both ways of staging it) over a fresh image, and goes on row by row (halo of the
 *   row before, whole row, tail zeros) until every row phase of the stream has come.  The cells that the matrix steps of the blocks that
 *   reach an output read, zero taps included, and the halo: out[0] = reads of cells nothing wrote, out[1] = reads of cells that hold a
 *   sample an EARLIER row wrote (the current one did not), out[2..3] = smallest and largest cell read, out[4] = cells of the image,
 *   out[5] = largest cell written, out[6] = largest cell of any read requested (the steps read ahead included), out[7] = rows checked,
 *   out[8] = accumulator sets (1 / 2), out[9..10] = smallest and largest cell counted in out[0] (-1: none), out[11] = 1 for the padded
 *   image (M = 0 mod 4).  DD_ERR_UNSUPPORTED unless k_chain_decim_b takes (K, M). */
int  dd_debug_decimb_lds_check(int K, int M, int phi, int64_t* out);
/* dd_debug_chain_select -- which kernel family a fused launch through a filter of these taps takes: the dispatcher of dd_chain.hip, asked
 *   with the selector as an argument (a dd_debug_select_kernel name; the process-wide choice is neither read nor changed).  flags: DD_CHAIN_*;
 *   in_align_bytes: the input pointer's address modulo 16.  *family = DD_FAMILY_*: the family tried FIRST -- a family whose state cannot be
 *   created on the device falls through to the next one (cos1k -> fft1k -> MFMA -> dense). */
#define DD_FAMILY_DENSE 0    /* k_chain_dense (DD_KERNEL_DENSE_F32) */
#define DD_FAMILY_TILES 1    /* k_chain_decim / _p / _multi (DD_KERNEL_DECIM_TILES / _PERSISTENT / _MULTI) */
#define DD_FAMILY_ROWS 2     /* k_chain_decim_w / _b (DD_KERNEL_DECIM_WAVE / _BLOCKS) */
#define DD_FAMILY_COS1K 3    /* k_chain_cos1k (DD_KERNEL_COS_RS) */
#define DD_FAMILY_FFT1K 4    /* k_chain_fft1k (DD_KERNEL_FFT_OS) */
#define DD_FAMILY_MFMA 5     /* k_chain_mfma_ab / _edge (DD_KERNEL_MFMA_AB / _TILES) */
int  dd_debug_chain_select(const double* taps_host, int ntaps, int decim, int flags, int in_align_bytes, const char* selector_name, int* family);
int  dd_debug_cos_fit(const double* taps_host, int K, double* a_out, int* Q_out);
int  dd_debug_sync_envelope(const void* X_dev, int64_t L, int nwin, int route, double* env_dev, void* stream);
/* dd_debug_sync_prefilter -- the envelope pre-filter stage of dd_noaa_sync_windows alone: x_dev f64 [nwin][n] (device) -> out_dev f64
 *   [nwin][n] = filtfilt(taps, [1], x) per window (decode_noaa.py:677 -> filters.py:72-73).  route 0: the prefix-sum form for taps that are
 *   a cosine series (DD_ERR_UNSUPPORTED when dd_debug_cos_fit refuses them), route 1: the tiled direct form on the same taps.
 *   n <= 3 K: DD_ERR_INVALID with SciPy's padlen message, as the batch reports it.
 * dd_debug_sync_tail -- the correlation / peak stage alone: hay_dev f64 [nwin][n] (device) is searched for needle
 *   needle_of_window_host[w] (NULL: needle 0) of needle_host [n_needles][needle_len] (piecewise constant, at most 64 runs), env_dev
 *   f64 [nwin][n] gives the post-sync mean (decode_noaa.py:671-673, :713-762 with two expected peaks).  peak = first index of the
 *   largest correlation - needle_len / 2, height = that correlation, tsync = mean(env[peak + m .. peak + 2 m)) when peak + 2 m < n, else NaN.
 *   A window whose maximum does not exceed the threshold, or whose correlation holds a NaN (a NaN sample; a silent stretch as long as
 *   the needle, 0 / 0), is (INT64_MIN, NaN, NaN). */
int  dd_debug_sync_prefilter(const double* x_dev, int64_t n, int nwin, const double* taps_host, int K, int route, double* out_dev, void* stream);
int  dd_debug_sync_tail(const double* hay_dev, const double* env_dev, int64_t n, int nwin, const double* needle_host, int needle_len,
                        int n_needles, const int* needle_of_window_host, int64_t* peak_host, double* height_host, double* tsync_host,
                        void* stream);
/* dd_debug_adsb_chips -- the 240 chip energies E_k[0 .. 240) of every listed candidate (the arguments of dd_adsb_demod in
 *   directdemod_hip.h): energies[240 c ..] for c < m, a device array; a k that is no candidate of the recording gives zeros.  Lets a
 *   test place a disagreement of dd_adsb_candidates or dd_adsb_demod at one chip. */
int  dd_debug_adsb_chips(const void* iq, int64_t n, int64_t rate, int phases, const int64_t* list, int64_t m, int64_t* energies,
                         void* stream);
/* dd_debug_pocsag_masks -- the mask byte of every sample that dd_pocsag_candidates lists from (its arguments): mask[n] on the device,
 *   1 = the sync codeword within `slack` places, 3 = its inverse, 0 otherwise and past the last start. */
int  dd_debug_pocsag_masks(const double* audio, int64_t n, double sps, int w, int slack, uint8_t* mask, void* stream);
/* dd_debug_acars_masks -- the mask byte of every sample that dd_acars_candidates lists from (its arguments): mask[n] on the device,
 *   1 = the template * SYN SYN SOH within `slack` places, 3 = its inverse, 0 otherwise and past the last start. */
int  dd_debug_acars_masks(const double* audio, int64_t n, double sps, int w, int slack, uint8_t* mask, void* stream);
/* dd_debug_rs41_masks -- the mask byte of every sample that dd_rs41_candidates lists from (its arguments): mask[n] on the device,
 *   1 = the RS41 header within `slack` places, 3 = the header of the negated audio, 0 otherwise and past the last start. */
int  dd_debug_rs41_masks(const double* audio, int64_t n, double sps, int w, int slack, uint8_t* mask, void* stream);
/* dd_debug_rs41_rs -- the Reed-Solomon wave as dd_rs41_frames instantiates it, RS(255,231) over GF(2)[x]/0x11D with roots alpha^0 ..
 *   alpha^23, over m words of 255 bytes (byte i the coefficient of x^(254 - i)): fixed[255 c ..] = the word within 12 bytes of word c
 *   with errors[c] = the bytes changed, or the word itself with -1 where there is none or where it would change a byte below
 *   first_valid (0 .. 255).  words, fixed and errors are device arrays.  Lets the decoder be tested without audio. */
int  dd_debug_rs41_rs(const uint8_t* words, int64_t m, int first_valid, uint8_t* fixed, int32_t* errors, void* stream);
/* dd_debug_rds_masks -- the mask byte of every start that dd_rds_candidates lists from (its arguments): mask[m] on the device,
 *   score << 1 | (score >= clean) with score = the blocks whose remainder is their offset word's, 0 where the group does not fit. */
int  dd_debug_rds_masks(const int32_t* b, int64_t m, double sps, int clean, uint8_t* mask, void* stream);
/* dd_debug_rds_halfbit -- the half-bit differences the RDS kernels decide bits from: z[2 p], z[2 p + 1] = the sum of b[p .. p + h - 1]
 *   less the sum of b[p - h .. p - 1], h = floor(sps / 2), for h <= p <= m - h and 0 elsewhere; b and z are device arrays of m pairs. */
int  dd_debug_rds_halfbit(const int32_t* b, int64_t m, double sps, int32_t* z, void* stream);
/* dd_debug_rds_repair -- the block repair of dd_rds_groups over loose words: word c of 26 bits against offset word offs[c] (0 A, 1 B,
 *   2 C, 3 C', 4 D) gives status[c] = 0 when it is clean, n when the one burst of at most `fix` bits (0 .. 5) that makes it clean has
 *   n ones, with fixed[c] the block without that burst, and -1 with fixed[c] = the word where there is none.  Device arrays. */
int  dd_debug_rds_repair(const uint32_t* words, const int32_t* offs, int64_t count, int fix, uint32_t* fixed, int32_t* status,
                         void* stream);
/* dd_debug_fms_mix -- the two mixed signals dd_fms_audio filters (its arguments): ab[2 j] = a[j], ab[2 j + 1] = b[j] for j < n, so the
 *   mixer and the filter can be tested apart. */
int  dd_debug_fms_mix(const double* mpx, int64_t n, uint64_t step38, const int32_t* table, const int32_t* u, int64_t nb, int G,
                      int32_t* ab, void* stream);
/* dd_debug_fms_audio_route -- dd_fms_audio with the filter's arithmetic chosen: route 0 sums in int64, route 1 in float64 fused
 *   multiply-adds; both are exact below 2^53 and give the same bits (profiles/fmstereo.txt compares their speed). */
int  dd_debug_fms_audio_route(const double* mpx, int64_t n, uint64_t step38, const int32_t* table, const int32_t* u, int64_t nb, int G,
                              const int32_t* taps, int ntaps, int D, int d0, int route, int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIRECTDEMOD_HIP_DEBUG_H */
