/* baz_music_hip.h -- C-ABI of the MI355X (gfx950) MUSIC direction-of-arrival engine.
 *
 * This is the drop-in boundary for ONE path of balint256/gr-baz: the body of
 *     baz_music_doa::work()            /root/reference/lib/baz_music_doa.cc:72-161
 * plus the state that work() reads:
 *     baz_music_doa::baz_music_doa()   /root/reference/lib/baz_music_doa.cc:35-53   (m, n, nsamples, resolution, table)
 *     set_array_response()             /root/reference/lib/baz_music_doa.cc:60-70   (table replacement)
 * The GNU Radio host block (gr_baz_amd/host/baz_music_doa.{h,cc}) keeps the reference's
 * make()/work()/set_array_response() signatures (lib/baz_music_doa.h:36,48,59) and does
 * nothing but marshal gr_complex / float buffers across this ABI.
 *
 * Conventions: plain C types, no exceptions, no torch/GNU Radio types.  The caller owns
 * every host buffer; the library owns all device memory it allocates.  0 == success,
 * negative == error (baz_music_strerror).  A context is single-producer: one thread calls
 * process*(); baz_music_set_table() may be called from any other thread (it is serialised
 * against process*() like the reference's d_mutex, lib/baz_music_doa.cc:67,101).
 *
 * Data layouts (identical to what the reference block sees on its ports):
 *   in        : batch items, each nsamples gr_complex (float re, float im), antenna-
 *               interleaved  x(r,c) = in[c*m + r]              (lib/baz_music_doa.cc:82-84)
 *   table     : resolution x m gr_complex, row-major [bin][antenna]  (array_response_t,
 *               lib/baz_music_doa.h:32-33, as delivered by swig/baz_swig.i:564)
 *   ang, lvl  : batch x n float   (output ports 0 and 1, lib/baz_music_doa.cc:146-155)
 *   spectrum  : batch x resolution float (optional port 2, lib/baz_music_doa.cc:120-121)
 */
#ifndef INCLUDED_BAZ_MUSIC_HIP_H
#define INCLUDED_BAZ_MUSIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define BAZ_MUSIC_API __attribute__((visibility("default")))
#else
#define BAZ_MUSIC_API
#endif

typedef struct baz_music_ctx baz_music_ctx;

enum {
    BAZ_MUSIC_OK = 0,
    BAZ_MUSIC_E_INVALID = -1,     /* bad argument (the reference only assert()s, .cc:45-50,62-63) */
    BAZ_MUSIC_E_NOMEM = -2,       /* host or device allocation failed */
    BAZ_MUSIC_E_HIP = -3,         /* HIP runtime error (baz_music_last_hip_error) */
    BAZ_MUSIC_E_UNSUPPORTED = -4, /* valid for the reference but not built here (m > BAZ_MUSIC_MAX_M ...) */
    BAZ_MUSIC_E_NODEVICE = -5     /* no gfx950 device / device_id out of range */
};

#define BAZ_MUSIC_MAX_M 64u       /* antennas handled by the gfx950 kernels */
#define BAZ_MUSIC_FAST_M 16u      /* ... by the kernels specialised per m (config 5 uses 16); 17..64 run the run-time-m path */
#define BAZ_MUSIC_MAX_N 63u       /* expected emitters (n < m) */

/* Stage indices for baz_music_stage_ms / baz_music_stage_name. */
enum { BAZ_MUSIC_STAGE_COV = 0, BAZ_MUSIC_STAGE_EVD = 1, BAZ_MUSIC_STAGE_SCAN = 2, BAZ_MUSIC_STAGE_MERGE = 3,
       BAZ_MUSIC_NUM_STAGES = 4 };

/* Replaces baz_music_doa::baz_music_doa (lib/baz_music_doa.cc:35-53).  Validates what the
 * reference only assert()s: m>0, 0<n<m (n==m underflows .cc:93), nsamples>0, nsamples%m==0,
 * resolution>0.  table_ri = resolution*m complex64 as interleaved floats.  device_id < 0
 * selects the current HIP device. */
BAZ_MUSIC_API int baz_music_create(baz_music_ctx** out, uint32_t m, uint32_t n, uint32_t nsamples,
                                   uint32_t resolution, const float* table_ri, int device_id);

/* Replaces baz_music_doa::~baz_music_doa (lib/baz_music_doa.cc:55-58). */
BAZ_MUSIC_API void baz_music_destroy(baz_music_ctx* ctx);

/* Replaces baz_music_doa::set_array_response (lib/baz_music_doa.cc:60-70): takes effect for
 * every item submitted after it returns. Thread-safe against process*().
 * The reference holds d_mutex (.cc:67) for one vector copy (.cc:69).  Here every device image of the new table (bilinear-form
 * table, raw-table operand, f16 pieces of the gated scan, int8 digit planes, ||a||^2) is built BY THE DEVICE on a side stream
 * into a second set of buffers while process*() keeps running on the old one; the lock that serialises against process*() is
 * taken only to exchange the two sets (gr_baz_amd/csrc/table_kernels.hip.h).  A batch sees the old table or the new one, never a
 * mixture.  Concurrent callers of set_table are serialised among themselves. */
BAZ_MUSIC_API int baz_music_set_table(baz_music_ctx* ctx, const float* table_ri);
/* Wall time of the last baz_music_set_table() of this context in milliseconds, and the part of it spent waiting for and
 * holding the lock shared with process*() (what a running work() can be held up by). */
BAZ_MUSIC_API int baz_music_last_retune_ms(baz_music_ctx* ctx, double* total_ms, double* swap_ms);

/* NUMERIC CONTRACT of the float outputs.  The reference stores (float)(1.0 / d), d = ||G^H a||^2 in fp64
 * (lib/baz_music_doa.cc:114-121,153).  Here d is evaluated in fp64 (projector form, literal form near nulls) and the
 * stored value is v_rcp_f32((float)d): within ~2 ulp_f32 (2.4e-7 relative) of the reference's correctly rounded value,
 * against north_star's 1e-5 -- so spectrum / lvl floats are close to, not bit-equal with, a CPU run of the reference.
 * Where the two differ in KIND: for 0 < d < FLT_MIN (1.2e-38) the reference stores a finite 1e38+ value while (float)d
 * is subnormal or 0 and v_rcp_f32 returns +inf; d == 0 gives +inf in both.  lvl[i] == spectrum[bin_i] holds bit for bit,
 * as in the reference.  ang is (float)(bin * 360.0 / resolution), exact.
 * ACROSS WIRINGS: with 6 to 8 antennas lvl is produced by different arithmetic with and without the spectrum port (the int8
 * scan, good to 7.5e-7, against exact fp64 values of the gated scan): lvl of one block agrees between its two wirings to
 * 2 ulp_f32 (tests/test_i8_scan.py pins 1.5e-6), the DoA bins except between bins whose strengths tie that closely.  Up
 * to 5 and from 9 antennas on both wirings give the same bits.
 *
 * Replaces the body of baz_music_doa::work (lib/baz_music_doa.cc:72-161) for `batch`
 * consecutive items held in HOST memory; blocks until ang/lvl/spectrum are filled.
 * lvl and spectrum may be NULL (ports 1 / 2 not wired; guards the reference's NULL-lvl
 * dereference, .cc:147-154). Returns the number of items processed (== batch) or <0. */
BAZ_MUSIC_API int baz_music_process(baz_music_ctx* ctx, const float* in_ri, uint32_t batch,
                                    float* ang, float* lvl, float* spectrum);

/* Same arithmetic on DEVICE-resident buffers (HBM), asynchronous on the context's stream:
 * d_in batch*nsamples complex64; d_ang, d_lvl batch*n float; d_spectrum batch*resolution
 * float or NULL. d_lvl may be NULL. Returns 0 or <0.
 * ORDERING: the launches go to the context's stream -- its own non-blocking stream unless baz_music_set_stream()
 * installed the caller's -- and nothing orders that stream against whatever produced d_in or pre-filled / will read
 * the outputs.  Either make it the producer's stream (set_stream), or call the _on form below, or synchronise. */
BAZ_MUSIC_API int baz_music_process_device(baz_music_ctx* ctx, const void* d_in, uint32_t batch,
                                           void* d_ang, void* d_lvl, void* d_spectrum);

/* The same call with stream semantics relative to `caller_stream` (a hipStream_t; NULL = the legacy default
 * stream): the batch starts after everything enqueued on caller_stream so far, and work enqueued on caller_stream
 * afterwards sees the outputs (two event record / wait pairs; none when caller_stream IS the context's stream). */
BAZ_MUSIC_API int baz_music_process_device_on(baz_music_ctx* ctx, void* caller_stream, const void* d_in,
                                              uint32_t batch, void* d_ang, void* d_lvl, void* d_spectrum);

/* Use an externally owned hipStream_t (e.g. the host framework's current stream) for all
 * subsequent launches; NULL restores the context's own stream (so the legacy default stream, whose
 * handle is NULL, cannot be selected: pass a created stream). */
BAZ_MUSIC_API int baz_music_set_stream(baz_music_ctx* ctx, void* hip_stream);

/* Blocks until everything submitted on the context's stream has finished. */
BAZ_MUSIC_API int baz_music_sync(baz_music_ctx* ctx);

/* Pre-allocates device workspace (covariances, projector coefficients) for `max_batch`
 * items so that process_device() never allocates inside a timed / captured region. */
BAZ_MUSIC_API int baz_music_reserve(baz_music_ctx* ctx, uint32_t max_batch);

/* Per-stage device timing with hipEvents recorded on the launch stream around each
 * kernel of process_device().  enable: 1 = start recording every stage (and reset), 2 = only the dominant
 * (scan) stage -- each recorded event pair costs ~10 us of launch gap --, 0 = stop. */
BAZ_MUSIC_API int baz_music_profile(baz_music_ctx* ctx, int enable);
/* Synchronises, then returns total milliseconds and number of launches recorded for `stage`. */
BAZ_MUSIC_API int baz_music_stage_ms(baz_music_ctx* ctx, int stage, double* total_ms, uint64_t* launches);
/* Kernel (symbol) name launched for `stage` with the context's configuration. */
BAZ_MUSIC_API const char* baz_music_stage_name(baz_music_ctx* ctx, int stage);

/* Test / diagnostic taps (device pointers): run a single stage.
 *   cov : d_in -> d_R      batch * m*m complex128 (row-major R[i][j], (re,im) doubles)   .cc:82-85
 *   evd : d_R  -> d_Q      m*m doubles per item, item-minor: d_Q[e*q_stride + item]; the
 *                          real coefficients of the noise-subspace projector G G^H         .cc:88-93
 * q_stride is returned by baz_music_q_stride() for the given batch.  Past BAZ_MUSIC_FAST_M antennas no projector is
 * formed (the literal form runs straight from the noise eigenvectors): `evd` and `q` return BAZ_MUSIC_E_UNSUPPORTED. */
BAZ_MUSIC_API int baz_music_debug_cov(baz_music_ctx* ctx, const void* d_in, uint32_t batch, void* d_R);
BAZ_MUSIC_API int baz_music_debug_evd(baz_music_ctx* ctx, const void* d_R, uint32_t batch, void* d_Q);
/*   q   : d_in -> d_Q      the two stages back to back, exactly as process_device() runs them for this
 *                          configuration; projector coefficients as for `evd` */
BAZ_MUSIC_API int baz_music_debug_q(baz_music_ctx* ctx, const void* d_in, uint32_t batch, void* d_Q);
/*   coarse margin : the scan that runs when port 2 is NOT wired and m <= 8 (lib/baz_music_doa.cc:97-99: only the top-n list
 *                          is observable then) evaluates every 16-item x 16-bin tile in a coarse f16-matrix-core form first and
 *                          the exact fp64 form only where a tile can still hold a top-n member; ang / lvl are bit-identical to
 *                          the full scan as long as |coarse - exact| <= NG 2^-16 (S + |exact|), NG = 1 (m <= 4) or ceil(m^2 / 32) (gr_baz_amd/csrc/
 *                          scan_coarse_kernels.hip.h).  This tap runs covariance + EVD of the batch and then BOTH forms on every
 *                          (item, bin); *worst = the largest observed error / allowance (sound below 1; derived with a factor
 *                          > 2 to spare).  BAZ_MUSIC_E_UNSUPPORTED for m > 8 or a table whose scale does not fit. */
BAZ_MUSIC_API int baz_music_debug_coarse_margin(baz_music_ctx* ctx, const void* d_in, uint32_t batch, float* worst);
/*   lab statistic: exact (16-item row group x 16-bin tile) evaluations of the coarse-gated scan's launches since the last
 *                          read (the counter resets); -1 unless the context was created under BAZ_MUSIC_COARSE_STATS=1. */
BAZ_MUSIC_API int64_t baz_music_debug_coarse_fired(baz_music_ctx* ctx);
/*   int8 scan   : from 6 to BAZ_MUSIC_FAST_M antennas (n <= 4) the scan evaluates d = a^H Q a on the int8 matrix core with both
 *                          operands cut into balanced base-256 digits -- integer accumulation, no rounding.  Every value is
 *                          first evaluated with four digits (error <= E4 = m^2 Fscale 4.04 2^-30) and keeps that form where it is
 *                          accurate to 7.5e-7; the others take five digits (E5 = m^2 Fscale 5.05 2^-38 + Fscale 2^-36), and where
 *                          even that is not accurate to 7.5e-7, seven (error <= m^2 Fscale 7.07 2^-54 + 2^-53 d: the accuracy class
 *                          of the fp64 form) -- decided per value by that value alone; near-null values take the reference's
 *                          literal form as in the fp64 scan (gr_baz_amd/csrc/scan_i8_kernels.hip.h; BAZ_MUSIC_EXACT=1 at create
 *                          keeps the fp64 scan).  `margin` runs covariance + EVD of the batch and then every form on every
 *                          (item, bin): worst[0] = the largest observed |d5 - d| / E5 (the bound holds while it stays below 1),
 *                          worst[1] = the largest |d7 - d| / (its bound + the fp64 form's own worst-case error), worst[2] = the
 *                          largest |d4 - d| / E4.  `stats` returns and resets the wave tiles that ran the seven-digit form /
 *                          walked since the last read.  `uses_i8_scan`: 1 when that scan is the one this context runs.
 *                          `i8_image` needs no device: the digit images of a table (size returned; written when out_bytes
 *                          suffices: five leading digits, then digits 5 and 6) and params[16] = {7 level weights, 2^54, T, E5,
 *                          refined allowance, 5, 7, E4, T4}. */
BAZ_MUSIC_API int baz_music_debug_i8_margin(baz_music_ctx* ctx, const void* d_in, uint32_t batch, float worst[3]);
BAZ_MUSIC_API int baz_music_debug_i8_stats(baz_music_ctx* ctx, uint64_t* refined_tiles, uint64_t* tiles);
BAZ_MUSIC_API int baz_music_uses_i8_scan(const baz_music_ctx* ctx);
BAZ_MUSIC_API size_t baz_music_debug_i8_image(uint32_t m, uint32_t resolution, const float* table_ri, uint8_t* out,
                                              size_t out_bytes, double* params);
/*   table images : `table_image` copies image `which` of the table IN FORCE back from the device -- 0 the bilinear-form table in
 *                          MFMA B-operand order, 1 the raw table in that order, 2 the gated scan's f16 pieces + fp64 operand, 3 the
 *                          int8 digit planes, 4 ||a||^2 per bin (padded), 5 / 6 the run-time-m path's transposed table and
 *                          ||a||^2, 7 the scalar parameters (BAZ_MUSIC_TABLE_NPARAMS doubles) -- and returns its size in bytes
 *                          (0: no such image for this configuration / table; nothing is written when out_bytes is too small).
 *                          `host_table_image` (needs no device) builds the same image with the round-4 host routines: the
 *                          checker the device builders must agree with byte for byte (tests/test_retune.py). */
#define BAZ_MUSIC_TABLE_NPARAMS 22
/* which + BAZ_MUSIC_TABLE_IMAGE_INNER: while baz_music_set_beamspace is on, image `which` of the projected table T^H a that the inner
 * context holds (0 while the mode is off). */
#define BAZ_MUSIC_TABLE_IMAGE_INNER 256
BAZ_MUSIC_API size_t baz_music_debug_table_image(baz_music_ctx* ctx, int which, void* out, size_t out_bytes);
BAZ_MUSIC_API size_t baz_music_debug_host_table_image(uint32_t m, uint32_t n, uint32_t resolution, const float* table_ri,
                                                      int which, void* out, size_t out_bytes);
/*   sorting     : LAB BUILD ONLY (libbaz_music_hip_lab.so, BAZ_MUSIC_SORT): measured and NOT shipped (profiles/r05_sort_negative.txt) -- the
 *                          release library has none of its kernels, never orders a batch and keeps no fire statistic; there `sort_state`
 *                          returns five zeros.  In the lab build, without port 2 (m <= 4) the context can order the items of a batch by the
 *                          position of their two deepest nulls (a counting sort on a 16-bit key from a float32 sample of the spectrum;
 *                          gr_baz_amd/csrc/sort_kernels.hip.h) and hand the gated scan the order as an index list; ang / lvl are bit-identical
 *                          either way.  `sort_state`: launches of the gated scan with / without the sort, and the exact evaluations / tile
 *                          pairs walked / sorted flag of the last finished one. */
BAZ_MUSIC_API int baz_music_debug_sort_state(baz_music_ctx* ctx, uint64_t out[5]);
/*   guard zones : LAB BUILD ONLY, process environment BAZ_MUSIC_GUARD=1: every device buffer of the library lies between two 64-KiB zones
 *                          filled with a pattern (and is itself pre-filled with it).  `guard_check` synchronises the device, compares the
 *                          zones of every live buffer and returns the number of zones found overwritten since the process started (a free
 *                          checks its buffer too) -- 0 means no kernel wrote outside a buffer of this library; details go to stderr.
 *                          `guard_active`: 1 when the guard is on.  Both return 0 in the release library. */
BAZ_MUSIC_API int baz_music_debug_guard_check(void);
BAZ_MUSIC_API int baz_music_debug_guard_active(void);
/*   live buffers : the library's live allocations in this process, out[0] device buffers, out[1] page-locked host buffers (release and lab
 *                          build alike; no lock).  Every one has an owner (gr_baz_amd/csrc/device_buffer.hip.h): after the last context
 *                          is destroyed both counts are what they were before the first was created. */
BAZ_MUSIC_API void baz_music_debug_live_buffers(uint64_t out[2]);
/*   (host only) the bin ranges per item the int8 scan launches with: whole rounds of the `slots` resident workgroups. */
BAZ_MUSIC_API uint32_t baz_music_debug_i8_nsplit(uint32_t batch, uint32_t nsteps, uint32_t slots);
BAZ_MUSIC_API uint32_t baz_music_q_stride(uint32_t batch);

/* Algorithmic HBM bytes per item: 8*nsamples + 8*n + 4*resolution (the last
 * term only when the spectrum port is wired). */
BAZ_MUSIC_API uint64_t baz_music_bytes_per_item(const baz_music_ctx* ctx, int with_spectrum);

BAZ_MUSIC_API const char* baz_music_strerror(int code);
/* hipGetErrorString of the last failing HIP call in this context ("" if none). */
BAZ_MUSIC_API const char* baz_music_last_hip_error(const baz_music_ctx* ctx);
BAZ_MUSIC_API const char* baz_music_version(void);
/* Number of usable gfx950 devices (0 when none) and the device a context lives on.  The host block deals its
 * instances over the devices round-robin (instance i -> device i mod count, SURVEY.md 8e: stream s -> GPU s mod G)
 * unless BAZ_MUSIC_DEVICE pins one. */
/* OPT-IN extension, not reference behaviour: mode 1 makes ang/lvl the n strongest LOCAL MAXIMA
 * of the pseudo-spectrum (bin b with s[b] > s[b-1] and s[b] >= s[b+1] on the circle) instead of the reference's n
 * strongest bins (lib/baz_music_doa.cc:129-141, which usually are neighbours on one lobe).  Same output format,
 * descending strength, (0, 0) for missing peaks.  Mode 0 (default) is the reference.  Mode 1 is offered up to
 * BAZ_MUSIC_FAST_M antennas (BAZ_MUSIC_E_UNSUPPORTED beyond). */
BAZ_MUSIC_API int baz_music_set_peak_mode(baz_music_ctx* ctx, int mode);
/* OPT-IN extension, NOT reference behaviour: forward-backward averaging (FB) and/or spatial smoothing (SS) of the
 * covariance, the standard fixes for coherent emitters (multipath, repeaters), whose rank-1 signal covariance leaves a signal
 * direction in the reference's noise subspace.  subarray = m_s with n < m_s <= m and m_s >= 2, L = m - m_s + 1 subarrays;
 * (subarray == m, forward_backward == 0) switches the mode off.
 *   DEFINITION  with X one item (m x K, x(r,c) = in[c*m + r]) and X_l = rows l .. l+m_s-1 of X:
 *                 R_ss = (1/L) sum_l X_l X_l^H / K;   FB: R = (R_ss + P conj(R_ss) P^T) / 2
 *               with P the centro-symmetry involution of the m_s subarray elements.  R is exactly the plain covariance of the
 *               re-stacked item Y = [X_0 .. X_{L-1} (, P conj(X_0) .. P conj(X_{L-1}))], m_s x K', K' = L K (FB ? 2 : 1), so
 *               the context runs an inner context of shape (m_s, n, m_s K', resolution) on the FIRST m_s COLUMNS of the table
 *               (gr_baz_amd/csrc/smoothing_kernels.hip.h re-stacks).  Every numeric statement above holds for that inner
 *               problem; the angle grid and the output ports do not change.
 *   CHECKS      on the fp32 table, each relation to a relative tolerance of 1e-5 of the bin's max_k |a_k(theta)|^2 (products
 *               in fp64; steering tables of the helper satisfy them to ~1e-7):
 *                 SS (m_s < m): shift invariance a_{i+l}(theta) a_0(theta) = a_i(theta) a_l(theta), i < m_s, l < L, every bin;
 *                 FB: an involution P of the m_s elements and a per-bin scalar c(theta) with conj(a_i) = c a_P(i), every bin.
 *               P is derived from the table: screened on 32 bins (O(m_s^3)), then verified on every bin (O(m_s res)).
 *               A ULA passes both, the unit square and an even-m uniform circle FB only, an odd circle or a random table neither.
 *   ERRORS      BAZ_MUSIC_E_INVALID for a failed check, m_s <= n, m_s > m or m_s < 2; BAZ_MUSIC_E_UNSUPPORTED when m_s K'
 *               exceeds 2^31; the previous mode stays in force after any error.
 *   OFF         is the reference bit for bit: a context that never called this, one set to (m, 0) and one switched on and off
 *               again run the same kernels with the same geometry.
 *   WHILE ON    mode changes and set_table take effect for items submitted after they return and are serialised against
 *               process*() (a batch sees the old mode / table or the new one).  set_table must pass the mode's checks, else it
 *               returns BAZ_MUSIC_E_INVALID and keeps the old table and mode.  process, process_device, process_device_on,
 *               reserve, sync, set_stream (forwarded), set_peak_mode, set_order_mode, set_refine_mode, set_power_mode, set_averaging / reset_averaging (forwarded), host_register / set_host_pinning work; every call
 *               is cut into chunks whose re-stacked items fit BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES (at least one item per chunk), and
 *               the host path stages its chunks through device buffers: its results equal the device path's bit for bit.
 *               uses_i8_scan answers for the inner context.  profile, stage_ms, refined_values / refined_items and the debug_
 *               taps that run stages (cov, evd, q, average, coarse_margin, coarse_fired, i8_margin, i8_stats) return
 *               BAZ_MUSIC_E_UNSUPPORTED, stage_name returns "".  table_image, bytes_per_item describe the full m-antenna table.
 * get_smoothing returns (m, 0) while off.  smoothing_check runs the checks on a table without a device: 0 or BAZ_MUSIC_E_INVALID
 * (also for m > BAZ_MUSIC_MAX_M, a NULL table, resolution 0); perm_out (m_s bytes, may be NULL) receives P (the identity without
 * FB).  set_smoothing and set_table use the same code. */
#define BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES (128u << 20)
BAZ_MUSIC_API int baz_music_set_smoothing(baz_music_ctx* ctx, uint32_t subarray, int forward_backward);
BAZ_MUSIC_API int baz_music_get_smoothing(const baz_music_ctx* ctx, uint32_t* subarray, int* forward_backward);
BAZ_MUSIC_API int baz_music_smoothing_check(uint32_t m, uint32_t resolution, const float* table_ri, uint32_t subarray,
                                            int forward_backward, uint8_t* perm_out);
/* OPT-IN extension, NOT reference behaviour: a per-item estimate of the NUMBER of emitters.  The reference fixes n at
 * construction (lib/baz_music_doa.cc:35-53, .cc:93); with the mode on the context's n becomes the LARGEST count n_max, each item
 * estimates its own count k in [0, n] from the eigenvalues of its covariance, uses a noise subspace of m - k eigenvectors and reports
 * k (ang, lvl) pairs followed by n - k pairs of (0, 0).  Ports and output format do not change; lvl is 1/d > 0 for every real entry,
 * so lvl == 0 marks a missing one (as in peak mode 1).  criterion: 0 = fixed n (the reference, the default), 1 = MDL, 2 = AIC
 * (Wax & Kailath 1985); anything else BAZ_MUSIC_E_INVALID.
 *   DEFINITION  N = nsamples / m snapshots; l_1 <= ... <= l_m the eigenvalues of the item's R (ties in the order of the Jacobi's
 *               ranking: lower column first), clamped l_i <- max(l_i, 2^-40 l_m).  For k = 0 .. n over the m - k smallest:
 *                 L(k) = -N (m - k) (mean(ln l) - ln(mean l)),  MDL(k) = L(k) + 1/2 k (2m - k) ln N,  AIC(k) = 2 L(k) + 2 k (2m - k);
 *               the count is the SMALLEST k that minimises the criterion.  Everything in fp64; the criterion does not change
 *               under R -> s R.  An item whose R is all zero or holds a NaN / Inf counts 0 and is otherwise treated as ever (a
 *               non-finite R: NaN spectrum).  Count 0: the projector is I, the spectrum 1 / ||a||^2, no pair is reported.
 *               tests/order_ref.py restates this in numpy.
 *   WHAT RUNS   the Jacobi epilogues decide (gr_baz_amd/csrc/order_kernels.hip.h holds the routine, music_kernels.hip.h the ORDER
 *               twins of evd_proj_kernel, cov4_evd_kernel and evd_proj_lds_kernel).  Orthogonal iteration yields no noise
 *               eigenvalues: from 5 antennas on EVERY item takes the Jacobi while the mode is on.  The scans run unchanged on
 *               projectors / signal vectors / noise vectors padded with zeros to a uniform shape; without the spectrum port, up to
 *               8 antennas run the full fp64 / int8 scan instead of the coarse-gated one (its gate reads n as a list length).  The
 *               int8 scan's bounds (|q_e| <= 1 + 2^-10, E4, E5) hold for a projector of any rank.  A small kernel then clears the
 *               entries at or beyond each item's count.  Mode 0 launches exactly the kernels it launched before the mode existed
 *               and is the reference bit for bit: a context never set, one set to 0, one switched on and off again.
 *   SCOPE       up to BAZ_MUSIC_FAST_M antennas (BAZ_MUSIC_E_UNSUPPORTED beyond), like peak mode.  Composes with peak mode (the k
 *               strongest local maxima) and with smoothing: the mode is forwarded to the inner context with N = this context's
 *               snapshot count K -- the K' re-stacked columns are not independent snapshots; the forward-backward-corrected
 *               penalty of the literature (Xu et al. 1994) is NOT applied.  profile, stage_ms and the debug_ taps keep working
 *               (debug_evd / debug_q return the variable-rank projector).  Up to 4 antennas the literal form near nulls carries
 *               m - 1 noise vectors: a count-0 item at a bin with ||a||^2 <= ~m 1e-8 max ||a||^2 (a table row that all but
 *               vanishes) gets the sum over the m - 1 smallest eigen-directions there.
 *   WHEN        set_order_mode takes effect for items submitted after it returns and is serialised against process*() like
 *               set_peak_mode: a batch sees the old mode or the new one.  The previous mode stays in force after any error.
 * last_orders: the counts of the items of the LAST process*() call in call order, at most `count` of them (a host-fed call cut into
 * chunks, or a smoothing call, reports all its items); blocks until that call is done; returns how many were written, or < 0.  A
 * call that ran with the mode off reports n for every item.  last_orders_device: the same bytes in HBM (one per item), valid until
 * the next process*() call, ordered on the context's stream; NULL before the first call.  order_estimate needs no device: the same
 * decision routine the kernels call, on `count` rows of m ascending eigenvalues with N = nsnap; BAZ_MUSIC_E_INVALID for m == 0,
 * m > BAZ_MUSIC_MAX_M, n_max >= m, nsnap == 0, a criterion other than 1 / 2 or a NULL array. */
BAZ_MUSIC_API int baz_music_set_order_mode(baz_music_ctx* ctx, int criterion);
BAZ_MUSIC_API int baz_music_get_order_mode(const baz_music_ctx* ctx, int* criterion);
BAZ_MUSIC_API int baz_music_last_orders(baz_music_ctx* ctx, uint8_t* out, uint32_t count);
BAZ_MUSIC_API const void* baz_music_last_orders_device(baz_music_ctx* ctx);
BAZ_MUSIC_API int baz_music_order_estimate(uint32_t m, uint32_t nsnap, uint32_t n_max, int criterion,
                                           const double* eigvals_ascending, uint32_t count, uint8_t* out);
/* OPT-IN extension, NOT reference behaviour: sub-bin angle refinement.  The reference reports angles on the steering grid,
 * ang = (float)(bin * 360 / resolution) (lib/baz_music_doa.cc:134,152).  Near an emitter the denominator d(theta) = ||G^H a(theta)||^2 is a
 * smooth null, d_min + c (theta - theta_0)^2 to leading order, so a parabola through d at the reported bin and its two neighbours locates
 * theta_0 far inside a bin (the fit is on d: the spectrum 1 / d is a Lorentzian there and fits a parabola badly).  mode: 0 = the
 * reference (the default), 1 = the parabolic null fit; anything else BAZ_MUSIC_E_INVALID.
 *   DEFINITION  for every reported entry (item, slot) with bin b, whichever picker produced it (the reference's top-n, peak mode 1,
 *               the emitter-count mode's truncation): y-, y0, y+ = the fp64 values of d at bins b - 1, b, b + 1 on the circle (the wrap of
 *               peak mode),
 *                 p = y- - y0,  q = y+ - y0
 *                 delta = (p - q) / (2 (p + q))    if p >= 0, q >= 0, p + q > 0 and all three values are finite
 *                 delta = 0                        otherwise (b on a flank, a plateau, next to a NaN / Inf)
 *               so |delta| <= 1/2, and  ang = (float)(((b + delta) mod resolution) * 360 / resolution)  evaluated in fp64 (b + delta < 0
 *               only at b = 0: one turn is added); a result that rounds to 360.0f is stored as 0.0f.  An entry with delta == 0 keeps
 *               exactly the ang bits of mode 0.  lvl and the spectrum port do not change by a single bit (lvl[i] == spectrum[b] still
 *               holds).  Missing entries -- missing peaks of peak mode 1, slots at or beyond an item's count in the emitter-count mode,
 *               the (0, 0) of .cc:95 -- stay (0, 0) whether or not lvl is wired.  tests/refine_ref.py restates this in numpy.
 *   THE VALUES  each of the three is formed the way the exact fp64 scan forms a value: the projector form a^H Q a in fp64, and the
 *               reference's literal form ||G^H a||^2 from the item's noise vectors where the projector form is at or below the table's
 *               threshold (~m 1e-8 max ||a||^2, see baz_music_refined_values).  Contexts whose scan runs the short form (one emitter from
 *               6 antennas, two from 9) keep no projector coefficients: there all three take the literal form.  In the emitter-count
 *               mode Q and G are the item's own variable-rank ones.  The int8 and f16 coarse forms are never used for these values.
 *   WHAT RUNS   one kernel (gr_baz_amd/csrc/refine_kernels.hip.h) after the merge / the picker / the truncation, one thread per entry;
 *               while the mode is on the pickers write into a staging buffer of the context and that kernel writes the caller's ang /
 *               lvl.  Steering rows come from an image that belongs to the table set in force: a batch sees the old table or the new
 *               one, for ang too.  Mode 0 launches exactly the kernels it launched before the mode existed and is the reference bit for
 *               bit: a context never set, one set to 0, one switched on and off again.
 *   SCOPE       up to BAZ_MUSIC_FAST_M antennas (BAZ_MUSIC_E_UNSUPPORTED beyond), like peak mode.  Meant to be used with peak mode 1:
 *               under the reference's top-n the entries after the first usually sit on a flank of the first one's null and stay put.
 *               Composes with the emitter-count mode and with smoothing (forwarded to the inner context).
 *   WHEN        set_refine_mode takes effect for items submitted after it returns and is serialised against process*() like
 *               set_peak_mode: a batch sees the old mode or the new one.  The previous mode stays in force after any error.
 * last_refine_offsets: delta of the entries of the LAST process*() call in call order ([item][slot]), at most `count` of them (a host-fed
 * call cut into chunks, or a smoothing call, reports all its items); blocks until that call is done; returns how many were written, or
 * < 0.  A call that ran with the mode off reports zeros.  (The float ang hides everything below ~2e-5 degrees; this tap does not.)  The
 * buffer behind it (8 n bytes per item) is allocated only by calls made with the mode on.  refine_estimate needs no device: the same decision routine the
 * kernel calls, on `count` triples (y-, y0, y+) at y3[3k .. 3k+2]; BAZ_MUSIC_E_INVALID for a NULL array with count > 0. */
BAZ_MUSIC_API int baz_music_set_refine_mode(baz_music_ctx* ctx, int mode);
BAZ_MUSIC_API int baz_music_get_refine_mode(const baz_music_ctx* ctx, int* mode);
BAZ_MUSIC_API int baz_music_last_refine_offsets(baz_music_ctx* ctx, double* out, uint32_t count);
BAZ_MUSIC_API int baz_music_refine_estimate(const double* y3, uint32_t count, double* delta_out);
/* OPT-IN extension, NOT reference behaviour: covariance averaging ACROSS the items of a stream.  The reference estimates every
 * item on its own, from the K = nsamples / m snapshots of that item (lib/baz_music_doa.cc:82-85).  With the mode on the output rate stays one
 * estimate per item and the covariance that is decomposed is a weighted mean over the last `window` items: a sliding window (forgetting == 1)
 * or exponential forgetting truncated at `window` taps (forgetting < 1).  window = W with 1 <= W <= BAZ_MUSIC_MAX_AVG_WINDOW, forgetting =
 * beta with 0 < beta <= 1; W == 1 is OFF whatever beta is (the default).
 *   DEFINITION  A context is one stream: its items are numbered t = 0, 1, ... in submission order across process*() calls since create, or
 *               since the last reset.  With R_t the item's plain covariance, exactly as computed with the mode off:
 *                 w_0 = 1, w_j = w_{j-1} beta (fp64);   c(t) = min(W, t + 1)
 *                 Rbar_t = (sum_{j = c(t)-1 .. 0} w_j R_{t-j}) inv_norm[c(t)],   inv_norm[c] = 1 / sum_{j < c} w_j   (summed j ascending)
 *               Each of the m^2 complex entries is accumulated OLDEST TAP FIRST from 0 with one fp64 FMA per tap and component and then
 *               multiplied once by inv_norm.  EVD, scan, pickers and every other mode run on Rbar_t exactly as they run on R_t with the
 *               mode off; ports, output format and the angle grid do not change.  The operation sequence of an output depends on (t, W,
 *               beta) alone, so AN ITEM'S BITS DO NOT DEPEND ON HOW THE STREAM WAS CUT into calls, chunks or passes, nor on whether a call
 *               was host-fed or device-resident (no running sum, nothing is ever subtracted).  The first W - 1 items of a stream average
 *               over the items there are.  tests/averaging_ref.py restates this in numpy.
 *               For beta == 1, Rbar_t is a scalar multiple of the plain covariance of the concatenated item [X_{t-c+1} .. X_t] (m x c K):
 *               what the reference itself computes for an item of c nsamples samples.  The projector ignores the scale, so the mode is
 *               held to the reference and to the per-path error bounds of that longer item, with no tolerance of its own.
 *   WHAT RUNS   two small kernels between the covariance and the EVD (gr_baz_amd/csrc/average_kernels.hip.h): average_kernel forms Rbar of
 *               the launch's items from their plain covariances and the history, average_history_kernel writes the history of the next
 *               launch.  The context keeps the last W - 1 plain covariances in device memory across calls (two buffers used in turn) and
 *               the stream position on the host.  Their time counts under BAZ_MUSIC_STAGE_COV.  At 4 antennas with K % 256 == 0, where
 *               covariance and EVD are otherwise one fused kernel, the two-kernel form runs while the mode is on (cov4_x4_kernel ->
 *               averaging -> evd_proj_kernel: the fused kernel's bits for the same R; stage_name(COV) says so).  OFF launches exactly the
 *               kernels it launched before the mode existed and is the reference bit for bit: a context never set, one set to W == 1, one
 *               switched on and off again.
 *   SCOPE       every antenna count, the 17 .. BAZ_MUSIC_MAX_M path included (the history runs from pass to pass).  Composes with peak mode
 *               and refinement (they read the spectrum / Q / G of the averaged problem), with the emitter-count mode -- the criterion's N
 *               becomes K n_eff, n_eff = (sum w)^2 / sum w^2 over the FULL window (W for a boxcar); the first W - 1 items of a stream use
 *               that same N although they average fewer items -- and with smoothing: the mode is forwarded to the inner context, which
 *               averages the re-stacked covariances (averaging and smoothing are both linear, so the order does not matter); the outer
 *               context keeps no history.  An item whose R holds a NaN / Inf POISONS the up to W items whose window contains it: they
 *               report (0, 0) and a NaN spectrum, as the poisoned item itself does with the mode off; reset_averaging ends that early.  An
 *               all-zero item is just a zero tap.  While the mode is on, debug_q, debug_coarse_margin and debug_i8_margin return
 *               BAZ_MUSIC_E_UNSUPPORTED (they would consume history); debug_cov keeps returning the plain R.
 *   WHEN        set_averaging takes effect for items submitted after it returns and is serialised against process*() like set_peak_mode:
 *               a batch sees the old mode or the new one.  It forgets the history whenever it changes W or beta (a call that changes
 *               neither keeps it).  set_smoothing forgets it too (the shape of R changes); set_table does not (covariances do not depend
 *               on the table); a launch sequence that fails does.  BAZ_MUSIC_E_INVALID for W == 0, W > BAZ_MUSIC_MAX_AVG_WINDOW, beta <= 0,
 *               beta > 1, a NaN beta or a NULL context; after an error the previous mode and history stay in force.
 * reset_averaging forgets the history: the next item is t = 0.  get_averaging returns (1, 1.0) for a context never set, else what was set.
 * averaging_weights needs no device: the routine the library fills its kernels' table with; w receives W weights, inv_norm W + 1 values
 * (inv_norm[0] = 0: no item has no tap), n_eff the effective number of items of a full window; each pointer may be NULL.
 * debug_average (device pointers, batch * m*m complex128 each, d_R_out != d_R_in): the averaging stage alone on caller-supplied covariances;
 * it advances the history exactly as a process call of `batch` items would.  The counterpart of debug_evd, but offered for every antenna count;
 * BAZ_MUSIC_E_UNSUPPORTED while the mode is off or smoothing is on. */
#define BAZ_MUSIC_MAX_AVG_WINDOW 64u
BAZ_MUSIC_API int baz_music_set_averaging(baz_music_ctx* ctx, uint32_t window, double forgetting);
BAZ_MUSIC_API int baz_music_get_averaging(const baz_music_ctx* ctx, uint32_t* window, double* forgetting);
BAZ_MUSIC_API int baz_music_reset_averaging(baz_music_ctx* ctx);
BAZ_MUSIC_API int baz_music_averaging_weights(uint32_t window, double forgetting, double* w, double* inv_norm, double* n_eff);
BAZ_MUSIC_API int baz_music_debug_average(baz_music_ctx* ctx, const void* d_R_in, uint32_t batch, void* d_R_out);
/* OPT-IN extension, NOT reference behaviour: a received-power estimate per reported entry.  lvl is the MUSIC pseudo-spectrum
 * 1 / ||G^H a||^2: it has no unit, depends on SNR and snapshot count and only ranks the entries of an item.  The Capon (minimum-variance)
 * estimate P = 1 / Re(a^H R^-1 a) is a power in the units of R; it needs only the covariance, no eigenvalues, projector or noise vectors, and
 * it is defined entry by entry, so it stays well-posed under the reference's top-n picker whose entries are usually neighbouring bins (a joint
 * least-squares estimate is singular there).  mode: 0 = off (the default, the reference), 1 = compute the estimates, every port bit for bit
 * unchanged, 2 = additionally the lvl port carries (float)P instead of 1 / d; anything else BAZ_MUSIC_E_INVALID.
 *   DEFINITION  for every reported REAL entry (item, slot) -- lvl != 0 after the merge, the peak picker or the count truncation:
 *                 b   the entry's bin on the steering grid -- the grid bin even with sub-bin refinement on (recovered from the staged,
 *                     unrefined ang as refine_kernel does it);
 *                 a   row b of the table in force for that batch, widened exactly from complex64 to fp64;
 *                 R   the m x m covariance the item's EVD decomposes: what baz_music_debug_cov returns; Rbar_t with averaging on; with
 *                     smoothing on the inner context's R, a taken from the first m_s columns, like every statement about that mode.
 *               P = 1 / Re(a^H R^-1 a) in fp64 by an UNPIVOTED LDL^H of R from the lower triangle as stored, the imaginary part of the
 *               diagonal ignored:
 *                 d_j  = Re R_jj - sum_{k<j} |L_jk|^2 d_k
 *                 L_ij = (R_ij - sum_{k<j} L_ik conj(L_jk) d_k) / d_j        (i > j)
 *                 z_i  = a_i - sum_{k<i} L_ik z_k
 *                 s    = sum_i |z_i|^2 / d_i
 *                 P    = 1 / s
 *               An item is DEGENERATE when some d_j is not finite or d_j <= BAZ_MUSIC_POWER_PIVOT_FLOOR (sum_i Re R_ii) / m (2^-40, the
 *               clamp of the emitter-count mode): an all-zero item, an item with K < m snapshots, an R that holds NaN or Inf.  All entries of
 *               a degenerate item get P = 0; an entry whose s is 0 or not finite gets P = 0; missing entries get 0.  P is linear in R:
 *               R -> sR gives sP, exactly so for s a power of two.  tests/power_ref.py restates this in numpy.
 *   RAW         P is the raw Capon estimate.  Its known finite-sample factor (K - m + 1) / K (it reads LOW by that factor) is NOT divided
 *               out, and the noise term sigma^2 / ||a||^2 it carries on top of the emitter's power is NOT subtracted.  No noise floor is
 *               estimated.
 *   MODE 2      lvl = (float)P.  ang and the spectrum do not change; entry order stays the pickers' order, by MUSIC strength; a missing
 *               entry stays (0, 0); a degenerate item's entries keep ang and report lvl = 0 (lvl[i] == spectrum[b] no longer holds).  With
 *               lvl == NULL mode 2 behaves as mode 1.
 *   WHAT RUNS   one kernel (gr_baz_amd/csrc/power_kernels.hip.h, on the solve of capon_solve.hip.h), the last launch of a sequence (after refinement where that is on): one
 *               item per group of 4 / 8 / 16 lanes, R read and factorised once per item.  While the mode is on the pickers write into the
 *               staging buffer refinement uses (one buffer with both on) and the final kernels write the caller's ang / lvl, every word
 *               once (refinement and mode 2 together: refine_kernel writes ang, power_kernel lvl).  Its time counts under
 *               BAZ_MUSIC_STAGE_MERGE.  At 4 antennas with K % 256 == 0 the fused covariance + EVD kernel keeps running and also stores
 *               its R (the tap of debug_cov).  Steering rows come from the image of the table set in force: a batch sees the old table
 *               or the new one, for P too.  Mode 0 launches exactly the kernels it launched before the mode existed, allocates nothing
 *               new and is the reference bit for bit: a context never set, one set to 0, one switched on and off again.
 *   SCOPE       up to BAZ_MUSIC_FAST_M antennas (BAZ_MUSIC_E_UNSUPPORTED beyond), like the other modes.  Composes with peak mode, the
 *               emitter-count mode, refinement and averaging; under smoothing it is forwarded to the inner context.
 *   WHEN        set_power_mode takes effect for items submitted after it returns and is serialised against process*() like
 *               set_peak_mode: a batch sees the old mode or the new one.  The previous mode stays in force after any error.
 * last_powers: P of the entries of the LAST process*() call in call order ([item][slot]), at most `count` of them (a host-fed
 * call cut into chunks, or a smoothing call, reports all its items); blocks until that call is done; returns how many were written, or
 * < 0.  A call that ran with the mode off reports zeros.  The buffer behind it (8 n bytes per item) is allocated only by calls made with
 * the mode on.  power_estimate needs no device: one R (m*m complex128, row-major, re / im interleaved) and `count` steering rows (m
 * complex64 each) give `count` powers by the definition above, the degeneracy rule and the s -> P step being the kernel's own text;
 * 1 <= m <= BAZ_MUSIC_MAX_M; BAZ_MUSIC_E_INVALID for m out of range or a NULL array with count > 0. */
#define BAZ_MUSIC_POWER_PIVOT_FLOOR (1.0 / 1099511627776.0)   /* 2^-40 */
BAZ_MUSIC_API int baz_music_set_power_mode(baz_music_ctx* ctx, int mode);
BAZ_MUSIC_API int baz_music_get_power_mode(const baz_music_ctx* ctx, int* mode);
BAZ_MUSIC_API int baz_music_last_powers(baz_music_ctx* ctx, double* out, uint32_t count);
BAZ_MUSIC_API int baz_music_power_estimate(uint32_t m, const double* R_ri, const float* a_ri, uint32_t count, double* out);
/* OPT-IN extension, NOT reference behaviour: the signal that arrives from every reported entry's direction, the other
 * emitters suppressed.  The Capon power of the power mode is the output power of the minimum-variance distortionless-response (MVDR)
 * beamformer w = R^-1 a / (a^H R^-1 a); this mode produces the weight vector itself and applies it to the item's snapshots on the device.
 * mode: 0 = off (the default, the reference), 1 = MVDR; loading: a finite double >= 0 (default 0), the diagonal loading in units of the
 * mean diagonal of R; anything else BAZ_MUSIC_E_INVALID and the previous setting stays in force.
 *   DEFINITION  for every reported REAL entry (item, slot) -- lvl != 0 after the merge, the peak picker or the count truncation -- with b,
 *               a and R taken as the power mode takes them (the GRID bin also under refinement; row b of the table in force, widened
 *               exactly; the covariance the item's EVD decomposes, what baz_music_debug_cov returns, Rbar_t with averaging on):
 *                 R_l  = R with loading (sum_i Re R_ii) / m added to the real diagonal (the trace summed in index order, the imaginary
 *                        part of the diagonal ignored)
 *               and in fp64, by the power mode's UNPIVOTED LDL^H of R_l from the lower triangle as stored, the same pivot rule against
 *               BAZ_MUSIC_POWER_PIVOT_FLOOR times the mean diagonal of R_l:
 *                 z_i  = a_i - sum_{k<i} L_ik z_k
 *                 s    = sum_i |z_i|^2 / d_i
 *                 u_i  = z_i / d_i - sum_{k>i} conj(L_ki) u_k
 *                 w    = u / s                                      (so that w^H a = 1)
 *                 y[c] = sum_{r<m} conj(w_r) x[c m + r]             (c = 0 .. K-1, K = nsamples / m)
 *               x: the item's OWN K snapshots, complex64 widened exactly, also under averaging (averaging changes R, not x); the sum in
 *               fp64 in the order r = 0 .. m-1, stored as complex64.  A DEGENERATE item (a failing pivot) gets w = 0 and y = 0 for all
 *               its entries; an entry whose s is 0 or not finite gets w = 0 and y = 0; a missing entry gets w = 0 and y = 0.  With
 *               loading > 0 an item with K < m snapshots is no longer degenerate (that is the point of loading); an all-zero item still
 *               is (its trace is 0).  R -> sR leaves w unchanged, exactly so for s a power of two.  tests/beam_ref.py restates this in
 *               numpy.  ang, lvl and the spectrum never change under this mode; the power mode keeps its own definition on the unloaded R.
 *   WHAT RUNS   two kernels (gr_baz_amd/csrc/beam_kernels.hip.h, the first on the solve of capon_solve.hip.h), the last launches of a sequence (behind refinement and the power mode
 *               where they are on): beam_weights_kernel, one item per group of 4 / 8 / 16 lanes, R read and factorised once per item; and
 *               beam_apply_kernel, which reads the batch's input a second time and writes n K complex64 per item.  While the mode is on
 *               the pickers write into the staging buffer refinement and the power mode use, and the final kernels write the caller's
 *               ang / lvl, every word once (with neither of those modes on: beam_weights_kernel).  Both launches count under
 *               BAZ_MUSIC_STAGE_MERGE.  At 4 antennas with K % 256 == 0 the fused covariance + EVD kernel keeps running and also stores
 *               its R (the tap of debug_cov).  A host-fed call applies every chunk's weights to the chunk's device copy of the input; on
 *               the zero-copy path (a small call on page-locked memory) the apply kernel reads the caller's mapped input a second time
 *               over the link.  Mode 0 launches exactly the kernels it launched before the mode existed, allocates nothing new and is the
 *               reference bit for bit: a context never set, one set to 0, one switched on and off again.
 *   SCOPE       up to BAZ_MUSIC_FAST_M antennas (BAZ_MUSIC_E_UNSUPPORTED beyond), like the other modes.  Composes with peak mode, the
 *               emitter-count mode (entries beyond an item's count are missing entries), refinement, the power mode and averaging.  It
 *               does NOT compose with baz_music_set_smoothing (the inner context works on re-stacked sub-array items: there is no
 *               m-antenna weight vector to apply): set_beam_mode(1, ..) while smoothing is on and set_smoothing(on) while this mode is on
 *               return BAZ_MUSIC_E_UNSUPPORTED, the setting already in force stays.
 *   WHEN        set_beam_mode takes effect for items submitted after it returns and is serialised against process*() like
 *               set_peak_mode: a batch sees the old setting or the new one.
 * last_beams: the beams of the first `items` items of the LAST process*() call in call order, [item][slot][K] complex64 (re / im
 * interleaved); covers all chunks of a host-fed call; blocks until that call is done; returns the number of items written, or < 0.  A call
 * that ran with the mode off reports zeros.  last_beams_device: the device buffer behind last_beams and its item count (NULL and 0 after a
 * call made with the mode off), for consumers that stay on the GPU; valid until the next process*(), set_* or destroy of the context;
 * ordered on the context's stream, it does not synchronise.  last_beam_weights: w as [item][slot][m] complex128, the call semantics of
 * last_beams.  The buffers (8 n K and 16 n m bytes per item of the call) are allocated only by calls made with the mode on;
 * baz_music_reserve pre-allocates them while the mode is on.  beam_weights needs no device: one R (m*m complex128, row-major, re / im
 * interleaved) and `count` steering rows (m complex64 each) give `count` weight vectors (m complex128 each) by the definition above, the
 * degeneracy rule and the s -> w step being the kernels' own text; 1 <= m <= BAZ_MUSIC_MAX_M; BAZ_MUSIC_E_INVALID for m out of range, a
 * loading that is negative or not finite, or a NULL array with count > 0. */
BAZ_MUSIC_API int baz_music_set_beam_mode(baz_music_ctx* ctx, int mode, double loading);
BAZ_MUSIC_API int baz_music_get_beam_mode(const baz_music_ctx* ctx, int* mode, double* loading);
BAZ_MUSIC_API int baz_music_last_beams(baz_music_ctx* ctx, float* out_ri, uint32_t items);
BAZ_MUSIC_API int baz_music_last_beams_device(baz_music_ctx* ctx, const void** d_beams, uint32_t* items);
BAZ_MUSIC_API int baz_music_last_beam_weights(baz_music_ctx* ctx, double* out_ri, uint32_t items);
BAZ_MUSIC_API int baz_music_beam_weights(uint32_t m, const double* R_ri, const float* a_ri, uint32_t count, double loading, double* w_ri);
/* OPT-IN extension, NOT reference behaviour: per-antenna gain / phase calibration.  On a real receiver every channel has
 * its own complex gain gamma_r: the snapshots are x = Gamma a(theta) s + noise with Gamma = diag(gamma).  The correction lives in the
 * TABLE, not in the data: MUSIC on the raw covariance with the rows gamma (.) a(theta) is exact under that model, while dividing the data
 * by gamma would colour the noise wherever the |gamma_r| differ.
 * set_calibration: gamma_ri = m complex64 (re / im interleaved), every one finite and nonzero, else BAZ_MUSIC_E_INVALID and the setting in
 * force stays; NULL = off (the default, the reference).
 *   DEFINITION  the table in force is a'_r(bin) = gamma_r a_r(bin), a = the table last given to create / set_table.  Both operands are
 *               widened exactly to fp64; each of the four products is exact (two 24-bit significands);
 *               re = g.re a.re - g.im a.im and im = g.re a.im + g.im a.re take one fp64 rounding each (the same with or without FMA
 *               contraction), then one round-to-nearest-even conversion to fp32.  Every numeric statement of this header then holds for
 *               the table a': parity with the reference, the per-path error bounds, the steering rows refinement, power and beam read.
 *               For the table a' the reference itself is the oracle.  gamma = all (1, 0) gives the bytes of a (1 a is exact; a component
 *               -0 may come back as +0).  calibration_apply is the host form, the kernel's own routine: table_ri = resolution x m
 *               complex64 -> out_ri likewise; needs no device; BAZ_MUSIC_E_INVALID for m == 0, m > BAZ_MUSIC_MAX_M, resolution == 0, a
 *               NULL array or a gamma entry that is zero or not finite.  tests/calib_ref.py restates it in numpy.
 *   WHAT RUNS   every device image of the table follows from the raw table on the device, which the first launch of a retune fills from
 *               the page-locked copy of the caller's table.  While a calibration is on that launch is table_calib_kernel
 *               (gr_baz_amd/csrc/calib_kernels.hip.h) instead of copy_words_kernel: the same zero-copy read over the link, times gamma
 *               (handed to the kernel by value), unit-stride 8-byte stores.  Nothing else in the builders changes, so the correction
 *               reaches every scan path and every mode at once, the 17 .. BAZ_MUSIC_MAX_M path included.  Off -- a context never set,
 *               one set to NULL, one switched on and off again -- launches exactly what it launched before the mode existed and every
 *               image and output is the reference's bit for bit.
 *   PERSISTENCE gamma stays in force across baz_music_set_table: the page-locked copy keeps holding the caller's table, and
 *               set_calibration is a retune of that table -- built into the shadow set, exchanged under the batch mutex, so a batch
 *               sees the old table image or the new one, never a mixture; it updates baz_music_last_retune_ms like set_table.
 *   SCOPE       every antenna count.  Composes with peak mode, the emitter-count mode, refinement, averaging, power and beam.  It does
 *               NOT compose with baz_music_set_smoothing (the re-stacked inner context presumes a shift-invariant array, which raw data
 *               under Gamma != c I does not give): set_calibration(non-NULL) while smoothing is on and set_smoothing(on) while a
 *               calibration is on return BAZ_MUSIC_E_UNSUPPORTED, the setting already in force stays.  baz_music_debug_table_image
 *               describes the calibrated table.
 * get_calibration: *on = 0 / 1; gamma_ri (may be NULL) receives the m values in force, (1, 0) each while off.
 *
 * Estimating gamma from a pilot -- one emitter at a known direction (ref = its row of the uncalibrated table), or a noise source
 * injected equally into all channels (ref = all (1, 0)).
 *   MODEL       a single pilot, noise white AT THE CHANNEL OUTPUTS: the covariance is P (Gamma p)(Gamma p)^H + sigma^2 I, whose
 *               principal eigenvector is exactly proportional to Gamma p whatever sigma^2 is.
 *   DEFINITION  R_t = the plain covariance of item t, exactly what baz_music_debug_cov returns (never the averaged one);
 *               Rbar = (1 / B) sum_t R_t in fp64, in the fixed two-level order of calib_kernels.hip.h (runs of consecutive items summed in
 *               ascending order, the runs' sums folded in ascending order, one multiplication by 1.0 / B; the cut is a function of
 *               (B, m) alone and nothing is accumulated atomically: the bits of Rbar depend on the input and (B, m) alone, and the
 *               host-fed and the device form give the same bits).  v = the unit eigenvector of the largest eigenvalue l1 of Rbar, by a
 *               cyclic Hermitian Jacobi in fp64 ON THE HOST (one m x m matrix is no work for the device; the batch's covariances and
 *               their mean are) from the upper triangle and the real diagonal as stored.  g_r = v_r / p_r, p = ref widened exactly; g
 *               times conj(g_0) / |g_0| with Im g_0 stored as exactly 0 (g_0 > 0); g scaled so that (1 / m) sum |g_r|^2 = 1.
 *               quality = l1 / Re tr(Rbar) (the trace summed in index order), in [1 / m, 1]: 1 for a pure pilot, about 1 / m for noise;
 *               the caller gates on it.  DEGENERATE -- Rbar holds a NaN or an Inf, its trace is not > 0, or v_0 == 0 --: BAZ_MUSIC_OK
 *               with quality = 0 and g = all (1, 0).  tests/calib_ref.py restates this on numpy.linalg.eigh.
 *   CALLS       calibrate: `batch` items from host memory, staged through a device buffer of the context chunk by chunk;
 *               calibrate_device: from device memory.  Both block, write gamma_ri (m complex128), *quality and, where Rbar_ri is not
 *               NULL, Rbar (m*m complex128, row-major), all host memory, and do NOT apply the result: round it to complex64 and hand it
 *               to set_calibration.  They consume no averaging history, touch none of the last_* taps and do not change the table; the
 *               covariance stage is the one debug_cov runs (at the fused shape the two-kernel form, as under averaging), in chunks of
 *               the context's covariance workspace (profiled under BAZ_MUSIC_STAGE_COV; cov_mean_kernel's launches under
 *               BAZ_MUSIC_STAGE_MERGE).  calibration_estimate is the routine they call on their Rbar; it needs no device.
 *   ERRORS      BAZ_MUSIC_E_INVALID for a ref entry that is zero or not finite, batch == 0, m out of range or a NULL pointer where one
 *               is required (Rbar_ri of calibrate* may be NULL); BAZ_MUSIC_E_UNSUPPORTED while smoothing is on. */
BAZ_MUSIC_API int baz_music_set_calibration(baz_music_ctx* ctx, const float* gamma_ri);
BAZ_MUSIC_API int baz_music_get_calibration(const baz_music_ctx* ctx, float* gamma_ri, int* on);
BAZ_MUSIC_API int baz_music_calibration_apply(uint32_t m, uint32_t resolution, const float* table_ri, const float* gamma_ri, float* out_ri);
BAZ_MUSIC_API int baz_music_calibrate(baz_music_ctx* ctx, const float* in_ri, uint32_t batch, const float* ref_ri, double* gamma_ri,
                                      double* quality, double* Rbar_ri);
BAZ_MUSIC_API int baz_music_calibrate_device(baz_music_ctx* ctx, const void* d_in, uint32_t batch, const float* ref_ri, double* gamma_ri,
                                             double* quality, double* Rbar_ri);
BAZ_MUSIC_API int baz_music_calibration_estimate(uint32_t m, const double* Rbar_ri, const float* ref_ri, double* gamma_ri, double* quality);
/* OPT-IN extension, NOT reference behaviour: a choice of spectrum ESTIMATOR.  MUSIC needs the emitter count n to split the
 * signal subspace from the noise subspace (with n too small the spectrum is wrong, not merely wider) and its 1 / ||G^H a||^2 has no unit.
 * The Capon (minimum-variance) and Bartlett (conventional beamformer) spectra need no count and no eigendecomposition and are powers in the
 * units of R over the whole circle.  kind: BAZ_MUSIC_ESTIMATOR_MUSIC (0, the default: the reference), _CAPON (1), _BARTLETT (2); anything
 * else BAZ_MUSIC_E_INVALID and the previous kind stays in force.
 *   DEFINITION  for kind 1 and 2 the item's R is taken exactly as the power mode takes it: the covariance baz_music_debug_cov returns,
 *               Rbar_t with averaging on, read from the lower triangle as stored, the imaginary part of the diagonal ignored.  a = row b
 *               of the table in force, widened exactly from complex64.  For every bin b:
 *                 Capon     P_C(b) = the power mode's P for row b: the same unpivoted LDL^H, the same BAZ_MUSIC_POWER_PIVOT_FLOOR degeneracy
 *                           rule, the same s -> P step.  A degenerate item's whole row is 0; a bin whose s is 0 or not finite is 0.
 *                 Bartlett  P_B(b) = q / (w w),  w = sum_i |a_i|^2,
 *                           y_i = sum_{j<i} R_ij a_j + Re(R_ii) a_i + sum_{j>i} conj(R_ji) a_j,  q = sum_i Re(conj(a_i) y_i),
 *                           all sums in index order; 0 when w == 0 or when q or w is not finite.  For unit-modulus rows this is
 *                           a^H R a / m^2: an emitter's power plus sigma^2 / m, the unit of P_C.
 *               Both are linear in R: R -> sR gives sP, exactly so for s a power of two.  The spectrum port carries (float)P(b) for
 *               every bin.  ang / lvl are taken FROM THOSE float32 VALUES AS STORED: with peak mode 0 by the reference's rule (the n
 *               largest values in descending order, the earlier bin first on ties, a value reported only if it is > 0, NaN never,
 *               missing entries (0, 0): lib/baz_music_doa.cc:95,129-141), with peak mode 1 the n strongest local maxima;
 *               lvl[i] == spectrum[bin_i] holds bit for bit.  n keeps its meaning as the number of reported entries (create's n < m
 *               rule stays).  The device evaluates P in fp64 in its own operation order (1 / d_i multiplied in; q over the lower
 *               triangle): a stored float32 is within one ulp_f32 of (float) of the host definition, zeros are exact.
 *               tests/spectrum_ref.py restates this in numpy.
 *   WHAT RUNS   the covariance kernels of the two-kernel frontend (also at 4 antennas with K % 256 == 0, as under averaging), the
 *               averaging stage where it is on, spectrum_scan_kernel (gr_baz_amd/csrc/spectrum_kernels.hip.h; its time counts under
 *               BAZ_MUSIC_STAGE_SCAN): a 256-thread workgroup factorises 64 / 32 / 16 items into LDS, then every lane takes one bin and
 *               walks the group's items; then a picker on the float32 spectrum (topn_spec_kernel, or peak_pick_kernel under peak mode
 *               1), then the power and beam kernels where those modes are on.  No EVD kernel, no MUSIC scan and no merge kernel is
 *               launched; baz_music_refined_values reports 0.  Without the spectrum port the scan writes a private spectrum of the
 *               context (baz_music_reserve sizes it while a kind is set).  Kind 0 launches exactly the kernels it launched before the
 *               mode existed, allocates nothing new and is the reference bit for bit: a context never set, one set to 0, one switched
 *               on and off again.
 *   SCOPE       up to BAZ_MUSIC_FAST_M antennas (BAZ_MUSIC_E_UNSUPPORTED beyond), like the other modes.  Composes with peak mode,
 *               averaging, calibration and retune (the table image in force for the batch), the power and beam modes (they read R and
 *               the staged entries) and the host-fed baz_music_process.  It does NOT compose with the emitter-count mode (no
 *               eigenvalues), refinement (the fit is on the MUSIC denominator) or smoothing: whichever of the two is set second returns
 *               BAZ_MUSIC_E_UNSUPPORTED and the setting already in force stays.
 *   WHEN        set_estimator takes effect for items submitted after it returns and is serialised against process*() like
 *               set_peak_mode: a batch sees the old kind or the new one.  The previous kind stays in force after any error.
 * spectrum_estimate needs no device: one R (m*m complex128, row-major, re / im interleaved) and `count` steering rows (m complex64 each)
 * give `count` values by the definition above -- kind 1 the bits of baz_music_power_estimate (the same routine), kind 2 the loop above;
 * 1 <= m <= BAZ_MUSIC_MAX_M; BAZ_MUSIC_E_INVALID for kind 0 or an unknown kind, m out of range or a NULL array with count > 0. */
#define BAZ_MUSIC_ESTIMATOR_MUSIC    0   /* the default: the reference */
#define BAZ_MUSIC_ESTIMATOR_CAPON    1
#define BAZ_MUSIC_ESTIMATOR_BARTLETT 2
BAZ_MUSIC_API int baz_music_set_estimator(baz_music_ctx* ctx, int kind);
BAZ_MUSIC_API int baz_music_get_estimator(const baz_music_ctx* ctx, int* kind);
BAZ_MUSIC_API int baz_music_spectrum_estimate(int kind, uint32_t m, const double* R_ri, const float* a_ri, uint32_t count, double* out);
/* OPT-IN extension, NOT reference behaviour: noise PRE-WHITENING with a known or measured noise covariance.  MUSIC and the
 * MDL / AIC emitter count assume a noise covariance sigma^2 I; channels of a real receiver differ in noise figure and gain setting and
 * neighbouring front ends share noise.  The calibration above corrects the signal model, this mode the noise model: with Rn = L L^H and
 * W = L^-1 the whitened snapshots W x have noise covariance I and steering vectors W a, so every stage runs in the whitened space.
 * set_noise_covariance: Rn_ri = m*m complex128, row-major, re / im interleaved; NULL = off (the default, the reference).  Rn is read as R
 * is read elsewhere: the lower triangle as stored, the imaginary part of the diagonal ignored.
 *   FACTOR      on the host in fp64: the unpivoted Cholesky factor Rn = L L^H (column by column, sums in index order), then W = L^-1 by
 *               substitution, row by row of W L = I.  W is lower triangular with a real positive diagonal (imaginary part exactly 0, the
 *               upper triangle exactly 0).  No normalisation is applied: R' is in units of the noise, and the caller may scale Rn.
 *               whitening_factor is the setter's own routine: Rn_ri -> W_ri (m*m complex128 each), needs no device.
 *   ERRORS      BAZ_MUSIC_E_INVALID for a non-finite entry of Rn_ri (any of the 2 m^2 numbers) and for a pivot d_j = Re Rn_jj -
 *               sum_{k<j} |L_jk|^2 that is not finite or is <= BAZ_MUSIC_POWER_PIVOT_FLOOR times the mean of the real diagonal (a
 *               rank-deficient or indefinite Rn).  After any error the previous setting stays in force.
 *   TABLE       the table in force is a'_r(b) = fl32(sum_{k <= r} W_rk a~_k(b)), a~ the entry of the table last given to create /
 *               set_table after the calibration where that is on (gamma first, then W), widened exactly.  The sum is fp64 from
 *               (+0, +0) with k ascending; each term is four fused multiply-adds, re = fma(W.re, a.re, re), re = fma(-W.im, a.im, re),
 *               im = fma(W.re, a.im, im), im = fma(W.im, a.re, im); one round-to-nearest conversion to fp32 per component.
 *               whiten_table is the host form, the kernel's own routine, bit for bit: table_ri = resolution x m complex64, W_ri = m*m
 *               complex128 (the upper triangle is not read) -> out_ri; needs no device; W = I returns the bytes of the table (a component
 *               -0 may come back as +0).  The mode persists across baz_music_set_table and baz_music_set_calibration; every numeric
 *               statement of this header then holds for the table a' and the covariance R'.
 *   COVARIANCE  the EVD decomposes R' = W R W^H per item in fp64, R = the plain covariance, or Rbar_t where averaging is on (average
 *               first, whiten second; the averaging history keeps plain covariances, so switching this mode does not touch it).  R is read
 *               as the Hermitian matrix its lower triangle describes; T_rj = sum_{k<=r} W_rk R_kj, then for r >= j
 *               R'_rj = sum_{k<=r} W_rk conj(T_jk), both from (+0, +0) with k ascending by the four fused multiply-adds above.  The full
 *               m x m matrix is written: upper triangle = conj(lower), the diagonal's imaginary part exactly +0.  An item touches no other
 *               item's data.  The emitter count reads the eigenvalues of R', refinement and the power mode read R' and a', the scans read
 *               the images of the whitened table.  baz_music_debug_cov keeps returning the plain R; debug_whiten runs the stage alone
 *               (d_R_in -> d_R_out, `batch` matrices of m*m complex128 in device memory, not overlapping) with the W in force and is
 *               BAZ_MUSIC_E_UNSUPPORTED while the mode is off.  tests/whiten_ref.py restates all of this in numpy.
 *   WHAT RUNS   table_whiten_kernel (gr_baz_amd/csrc/whiten_kernels.hip.h) takes the place of copy_words_kernel / table_calib_kernel as
 *               the first launch of a retune; every other image follows unchanged.  Between the covariance (or the averaging stage)
 *               and the EVD runs whiten_kernel<M> (2 .. 16 antennas) or whiten_wide_kernel twice (17 .. 64); their time counts under
 *               BAZ_MUSIC_STAGE_COV.  At 4 antennas with K % 256 == 0 the two-kernel frontend runs, as under averaging.  W travels with
 *               the table set: set_noise_covariance is a retune of the table in force into the shadow set, exchanged under the batch
 *               mutex, so a batch sees the old (table, W) or the new pair, never a mixture.  Off -- a context never set, one set to NULL,
 *               one switched on and off again -- launches exactly what it launched before the mode existed and every output is the
 *               reference's bit for bit.
 *   SCOPE       every antenna count 2 .. BAZ_MUSIC_MAX_M.  Composes with peak mode, the emitter-count mode, refinement, the power mode (by
 *               its own definition on R' and a'), averaging, calibration, retune and the host-fed baz_music_process.  It does NOT compose
 *               with smoothing (the whitened table is not shift invariant), the beam mode (its weights would apply to unwhitened
 *               snapshots) or estimator kinds 1 / 2 (Capon is invariant under the transform: nothing is gained): whichever of the two is
 *               set second returns BAZ_MUSIC_E_UNSUPPORTED and the setting already in force stays.
 * get_noise_covariance: *on = 0 / 1; Rn_ri (may be NULL) receives the Rn in force as given, the identity while off.
 * mean_covariance / _device: Rbar of `batch` items from host / device memory into Rbar_ri (m*m complex128, host memory): exactly the Rbar of
 * baz_music_calibrate's definition (the same routine, the same bits), without a pilot -- a noise-only capture becomes an Rn.  They block,
 * consume no averaging history and change nothing; BAZ_MUSIC_E_INVALID for batch == 0 or a NULL pointer, BAZ_MUSIC_E_UNSUPPORTED while
 * smoothing is on. */
BAZ_MUSIC_API int baz_music_set_noise_covariance(baz_music_ctx* ctx, const double* Rn_ri);
BAZ_MUSIC_API int baz_music_get_noise_covariance(const baz_music_ctx* ctx, double* Rn_ri, int* on);
BAZ_MUSIC_API int baz_music_whitening_factor(uint32_t m, const double* Rn_ri, double* W_ri);
BAZ_MUSIC_API int baz_music_whiten_table(uint32_t m, uint32_t resolution, const float* table_ri, const double* W_ri, float* out_ri);
BAZ_MUSIC_API int baz_music_debug_whiten(baz_music_ctx* ctx, const void* d_R_in, uint32_t batch, void* d_R_out);
BAZ_MUSIC_API int baz_music_mean_covariance(baz_music_ctx* ctx, const float* in_ri, uint32_t batch, double* Rbar_ri);
BAZ_MUSIC_API int baz_music_mean_covariance_device(baz_music_ctx* ctx, const void* d_in, uint32_t batch, double* Rbar_ri);
/* OPT-IN extension, NOT reference behaviour: BEAMSPACE MUSIC.  Every snapshot x of the m antennas is projected onto
 * B <= BAZ_MUSIC_FAST_M beams, y = T^H x, and the estimate runs in the B-dimensional space on the table a' = T^H a.  It is what opens
 * the opt-in modes of this header (peak mode, emitter count, refinement, power mode, the Capon / Bartlett estimators), which exist up
 * to BAZ_MUSIC_FAST_M antennas, to arrays of 17 .. BAZ_MUSIC_MAX_M antennas.  T_ri: T, m x B complex128, row-major [antenna r][beam b],
 * re / im interleaved.  B == 0 or T_ri == NULL switches the mode off (the default; off is the reference).
 *   PROJECTION  for every time column c of every item, x_r(c) = in[c*m + r]:
 *                 y_b(c) = fl32(sum_{r = 0 .. m-1} conj(T_rb) x_r(c))
 *               x widened exactly; the sum in fp64 from (+0, +0) with r ascending; each term the four fused multiply-adds
 *                 re = fma(wr, xr, re); re = fma(-wi, xi, re); im = fma(wr, xi, im); im = fma(wi, xr, im)
 *               with wr = Re T_rb, wi = -Im T_rb (the chain of the noise pre-whitening above); one round-to-nearest conversion per
 *               component.  y(b, c) = out[c*B + b]: an item of the shape (B, B K).  A batch is one flat (batch K) x m row-major matrix in
 *               and one (batch K) x B matrix out; a column never reads another column, so a non-finite sample poisons its own item
 *               only.  No special cases: overflow to +-inf on conversion is IEEE's.
 *   TABLE       the table in force for the inner context is the same routine applied to every row of the raw table (a table is laid out
 *               like an item with K = resolution).  With normalise != 0 a row's unrounded fp64 sums s_b are divided by
 *               nu = sqrt(sum_b (Re s_b)^2 + (Im s_b)^2) (accumulated with b ascending, re before im, by fma) before the conversion; a
 *               row whose nu is 0 or not finite becomes zeros.  normalise exists because plain MUSIC does not divide by ||a'||^2: a
 *               design whose out-of-sector rows nearly vanish (||T^H a|| << ||a||) shows huge pseudo-spectrum values there, which unit
 *               rows avoid.  Designs whose rows keep a fair share of their norm everywhere do not need it.
 *   PORTS       ang / lvl / spectrum are what a plain context of shape (B, n, B K, resolution) on the table a' produces for the items y,
 *               bit for bit (it is such a context that runs: gr_baz_amd/csrc/beamspace_kernels.hip.h projects, the inner context does the
 *               rest, int8 and f16-gated scans included).  ang is still bin*360/resolution of the caller's own table.
 *   VALIDITY    2 <= B <= min(m, BAZ_MUSIC_FAST_M), n < B, every antenna count 2 <= m <= BAZ_MUSIC_MAX_M; BAZ_MUSIC_E_INVALID otherwise, and
 *               for a non-finite entry of T or an all-zero column; the setting in force stays after any error.  MUSIC and the MDL / AIC
 *               count presume T^H T = I, so that white noise stays white.  THE SETTER DOES NOT ENFORCE IT; baz_music_beamspace_design
 *               delivers it.
 *   WHEN        like set_smoothing: the setter is serialised against process*() (a batch sees the old setting or the new one, never a
 *               mixture); set_table while the mode is on rebuilds a' with the T in force and forwards it (T survives retunes).
 *   COMPOSES    peak mode, emitter-count mode (N of the criterion is K), refinement, power mode, covariance averaging AND THE ESTIMATOR
 *               KIND are forwarded to the inner context and survive switching this mode on -- and off, where the plain path offers them:
 *               switching off on a context of more than BAZ_MUSIC_FAST_M antennas resets peak, emitter-count, refine and power mode and
 *               the estimator to their defaults, because the run-time-m kernels have none of them.  last_orders, last_refine_offsets,
 *               last_powers and their device forms answer for the inner context.  reserve, sync, set_stream, host_register /
 *               set_host_pinning work; every call is cut into chunks whose projected items fit BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES (at
 *               least one item per chunk), and the host-fed baz_music_process stages the same chunks through device buffers: the same
 *               bits as the device path.  uses_i8_scan answers for the inner context.
 *   REFUSES     with BAZ_MUSIC_E_UNSUPPORTED, in both orders, the setting in force staying: smoothing (two front-ends would compete for
 *               one inner context), calibration and noise pre-whitening (gamma o a -> T^H and W -> T^H are definable but not offered), the
 *               beam mode (its weights would be B-vectors; w = T w' is not offered).  profile, stage_ms, refined_values / refined_items
 *               and the debug_ taps that run stages return BAZ_MUSIC_E_UNSUPPORTED and stage_name returns "" while the mode is on, as
 *               under smoothing; table_image and bytes_per_item describe the full m-antenna table.
 *   OFF         never set, set to off, or switched on and off again: the kernels, launch counts and every port of a context before the
 *               mode existed, bit for bit; nothing is allocated.
 * get_beamspace: *B = 0 while off, else the B in force, T_out (m*B complex128, may be NULL, untouched while off) and *normalise.
 * debug_beamspace runs the projection alone with the T in force: d_in (batch items of m K complex64) -> d_out (batch K B complex64), device
 * memory, not overlapping; BAZ_MUSIC_E_UNSUPPORTED while the mode is off.
 * HOST FUNCTIONS (no device needed):
 *   beamspace_apply   the routine above over `columns` rows of m complex64 -> rows of B complex64 (items and tables alike; normalise
 *                     applies per row, as for tables); 1 <= B <= min(m, BAZ_MUSIC_FAST_M); the kernel runs the same text: the same bits.
 *   beamspace_design  C = sum of a_b a_b^H over the bins (bin_lo + i) mod resolution, i < bin_count, accumulated in fp64 and decomposed by
 *                     the cyclic Hermitian Jacobi of the calibration estimate; T_out (m x B) = the eigenvectors of the B largest
 *                     eigenvalues in descending order, unit norm, each scaled so that its largest-modulus component (lowest index on
 *                     ties) is real and positive; *captured_out (may be NULL) = the sum of those B eigenvalues / trace C.
 *                     BAZ_MUSIC_E_INVALID for bin_count == 0 or > resolution, B out of range, or a sector that is zero or not finite. */
BAZ_MUSIC_API int baz_music_set_beamspace(baz_music_ctx* ctx, uint32_t B, const double* T_ri, int normalise);
BAZ_MUSIC_API int baz_music_get_beamspace(const baz_music_ctx* ctx, uint32_t* B, double* T_out, int* normalise);
BAZ_MUSIC_API int baz_music_debug_beamspace(baz_music_ctx* ctx, const void* d_in, uint32_t batch, void* d_out);
BAZ_MUSIC_API int baz_music_beamspace_apply(uint32_t m, uint32_t B, const double* T_ri, int normalise, const float* in_ri, uint32_t columns,
                                            float* out_ri);
BAZ_MUSIC_API int baz_music_beamspace_design(uint32_t m, uint32_t resolution, const float* table_ri, uint32_t bin_lo, uint32_t bin_count,
                                             uint32_t B, double* T_out, double* captured_out);
/* OPT-IN extension, NOT reference behaviour: WIDEBAND (SUBBAND) MUSIC.  One steering table is right at one wavelength.
 * Behind a wide front end every item is cut into blocks of F samples, an F-point DFT per antenna separates S used subbands, the
 * estimator runs per subband on THAT subband's table, and the S spectra are combined into one row the pickers read (incoherent wideband
 * MUSIC).  With K = nsamples / m time columns per item, Q = K / F blocks.  The library never learns the sample rate: the caller lists
 * the DFT indices to use and supplies one table per index.  F == 0 switches the mode off (the default; off is the reference).
 *   PARAMETERS  2 <= F <= 64, F divides K; 1 <= S <= BAZ_MUSIC_MAX_SUBBANDS distinct DFT indices bins[s] = k_s in [0, F), used in the
 *               order given; tables_ri: S tables of resolution x m complex64 (the layout of baz_music_create's), table s for k_s;
 *               combine: BAZ_MUSIC_SUBBAND_HARMONIC or BAZ_MUSIC_SUBBAND_ARITHMETIC.
 *   TWIDDLES    W[s][t] = exp(-2 pi i ((k_s t) mod F) / F) / sqrt(F), complex128, computed once on the host: every component within
 *               2 ulp of the exact value, and the values 0 and +-fl64(1 / sqrt(F)) at (k_s t) mod F a multiple of F / 4 exactly those.
 *               baz_music_subband_twiddles returns them ([S][F], re / im interleaved).  Everything below is defined in terms of the W in
 *               force, so the device, baz_music_subband_apply and a restatement that takes W from the library agree bit for bit.
 *   CHANNELISER for item i, block q < Q, antenna r, with x(i, c, r) = in[i*nsamples + c*m + r]:
 *                 y_s(i, q, r) = fl32(sum_{t = 0 .. F-1} W[s][t] x(i, q F + t, r))
 *               x widened exactly; the sum in fp64 from (+0, +0) with t ascending; each term the four fused multiply-adds
 *                 re = fma(wr, xr, re); re = fma(-wi, xi, re); im = fma(wr, xi, im); im = fma(wi, xr, im)
 *               with wr = Re W[s][t], wi = Im W[s][t] (the chain of the noise pre-whitening and of the beamspace projection, along time
 *               instead of across antennas); one round-to-nearest conversion per component.  Device layout [s][item][q][r]: the items
 *               of subband s are one contiguous batch of ordinary items of shape (m, m Q).  A (block, antenna) pair reads no other, so
 *               a non-finite sample turns exactly the S outputs of its own (block, antenna) non-finite.
 *   PER SUBBAND an inner context of shape (m, n, m Q, resolution) on table s runs the fast path on subband s's items, its spectrum port
 *               wired: P_s(i, b), float32, what a plain context of that shape gives for those items bit for bit.
 *   COMBINE     harmonic:   P(i, b) = fl32(S / sum_s (1.0 / (double)P_s(i, b)))     (the sum of the subbands' MUSIC denominators)
 *               arithmetic: P(i, b) = fl32((sum_s (double)P_s(i, b)) / S)          (meant for the Capon / Bartlett powers)
 *               both sums from +0 with s ascending in plain IEEE fp64 additions, one division at the end; zeros, infinities and NaNs
 *               do what IEEE does with these formulas.
 *   PORTS       ang / lvl are picked from the combined float32 row: peak mode 0 by the reference's top-n rule (the strongest n bins by
 *               value, the earlier bin first on ties, a value reported only if > 0), peak mode 1 by the local-maximum picker;
 *               ang = bin*360/resolution, lvl = the combined word itself.  Port 2, where wired, carries the combined row.
 *   VALIDITY    2 <= m <= BAZ_MUSIC_FAST_M (17 .. BAZ_MUSIC_MAX_M antennas: BAZ_MUSIC_E_UNSUPPORTED); F, S, bins as above, finite tables,
 *               combine 0 or 1: BAZ_MUSIC_E_INVALID otherwise; what baz_music_create refuses for the shape (m, n, m Q, resolution)
 *               comes back as create's code.  The setting in force stays after any error.
 *   WHEN        both setters build the S inner contexts beside the running stream and exchange them under the batch lock: a batch sees
 *               all S old tables or all S new ones, never a mixture.  set_subband_tables keeps F, the bins and the rule and is a fresh
 *               set_subbands with the new tables (covariance-averaging histories start over); BAZ_MUSIC_E_UNSUPPORTED while off.
 *               baz_music_set_table while the mode is on replaces only this context's own table, the one "off" returns to.
 *   COMPOSES    peak mode acts on the combined row (the inner contexts stay at mode 0).  The estimator kind is forwarded to every inner
 *               context; so are covariance averaging with its weights and window, and its reset: each subband averages its own stream.
 *               reserve, sync, set_stream, host_register / set_host_pinning work; every call is cut into chunks whose channelised items
 *               and whose S private spectrum rows each fit BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES (at least one item per chunk), and the
 *               host-fed baz_music_process stages the same chunks through device buffers: the same bits as the device path.
 *   REFUSES     with BAZ_MUSIC_E_UNSUPPORTED, in both orders, the setting in force staying: smoothing, beamspace, calibration, noise
 *               pre-whitening, the emitter-count mode, refinement, power mode and beam mode.  profile, stage_ms, refined_values /
 *               refined_items and the debug_ taps that run stages return BAZ_MUSIC_E_UNSUPPORTED and stage_name returns "" while the
 *               mode is on, as under smoothing.
 *   OFF         never set, set to off, or switched on and off again: the kernels, launch counts and every port of a context before the
 *               mode existed, bit for bit; nothing is allocated.
 * get_subbands: *F = *S = 0 while off, else the setting in force; bins_out (S words, may be NULL, untouched while off), *combine.
 * debug_subbands runs the channeliser alone with the W in force: d_in (batch items) -> d_out (S batch Q m complex64, [s][item][q][r]),
 * device memory, not overlapping; BAZ_MUSIC_E_UNSUPPORTED while the mode is off.  debug_subband_combine runs the combine alone under the S and
 * the rule in force: d_spectra (S batch resolution float32, [s][item][bin]) -> d_out (batch resolution float32), likewise.
 * HOST FUNCTIONS (no device needed):
 *   subband_twiddles  W_out[S][F] complex128 for the bins given; BAZ_MUSIC_E_INVALID for F, S or bins out of range or repeated.
 *   subband_apply     the channeliser over `blocks` blocks of F x m complex64 (in_ri: [block][t][r]) with the W given (any S x F
 *                     complex128: a block window is a change of W) -> out_ri [s][block][r]; the kernel runs the same text. */
#define BAZ_MUSIC_MAX_SUBBANDS 32u
#define BAZ_MUSIC_SUBBAND_HARMONIC 0
#define BAZ_MUSIC_SUBBAND_ARITHMETIC 1
BAZ_MUSIC_API int baz_music_set_subbands(baz_music_ctx* ctx, uint32_t F, uint32_t S, const uint32_t* bins, const float* tables_ri, int combine);
BAZ_MUSIC_API int baz_music_set_subband_tables(baz_music_ctx* ctx, const float* tables_ri);
BAZ_MUSIC_API int baz_music_get_subbands(const baz_music_ctx* ctx, uint32_t* F, uint32_t* S, uint32_t* bins_out, int* combine);
BAZ_MUSIC_API int baz_music_debug_subbands(baz_music_ctx* ctx, const void* d_in, uint32_t batch, void* d_out);
BAZ_MUSIC_API int baz_music_debug_subband_combine(baz_music_ctx* ctx, const void* d_spectra, uint32_t batch, void* d_out);
BAZ_MUSIC_API int baz_music_subband_twiddles(uint32_t F, uint32_t S, const uint32_t* bins, double* W_out);
BAZ_MUSIC_API int baz_music_subband_apply(uint32_t m, uint32_t F, uint32_t S, const double* W_ri, const float* in_ri, uint32_t blocks,
                                          float* out_ri);
/* Statistic: how many (item, bin) values of the LAST process call were recomputed in the reference's literal form
 * ||G^H a||^2 because the projector form a^H Q a put them at or below ~m 1e-8 max||a||^2 (near-nulls of the noise
 * subspace, SNR >~ 55 dB); blocks until that call is done (a host-fed call cut into chunks reports their sum).
 * -1 on error.  See DESIGN.md 2 (near-nulls).  (The name is kept from round 1, which redid whole items.) */
BAZ_MUSIC_API int64_t baz_music_refined_values(baz_music_ctx* ctx);
/* The same number under its round-1 name (round 1 redid whole ITEMS; since round 2 the unit is one (item, bin) value, so
 * do not compare it with a batch size).  Past BAZ_MUSIC_FAST_M antennas only the matrix-core scan (n <= 8) counts; the
 * general wide scan evaluates the literal form near nulls per bin and keeps no count (0).  Without the spectrum port only values that could still enter
 * the top-n list are evaluated at all, so fewer are counted than with it. */
BAZ_MUSIC_API int64_t baz_music_refined_items(baz_music_ctx* ctx);
BAZ_MUSIC_API int baz_music_device_count(void);
BAZ_MUSIC_API int baz_music_device(const baz_music_ctx* ctx);

/* Host-fed path: page-locking of the CALLER's buffers.  baz_music_process() copies straight
 * between the caller's host memory and HBM; when that memory is pageable the runtime stages every copy through its own
 * bounce buffers (measured: 1.1e6 items/s pageable against 2.5e6 page-locked for 8-MiB calls of config 2).  A
 * scheduler's stream buffers live as long as the flowgraph and are handed to work() over and over, so they are worth
 * locking once:
 *   baz_music_host_register(ctx, p, bytes)   page-locks [p, p+bytes) for this context (hipHostRegister on exactly
 *       that range, or on its union with the registrations of this context it overlaps or touches: a buffer may be
 *       registered piecewise, and may map the same physical pages twice like GNU Radio's circular buffers; every
 *       request ends up inside ONE registration, because the runtime rejects copies that are only partly inside one).
 *       0 when the range is locked (or already was, also by its owner: hipHostMalloc / torch pinned memory);
 *       BAZ_MUSIC_E_HIP when the runtime refuses it (remembered; asked again after 1,024 further requests for it);
 *       BAZ_MUSIC_E_UNSUPPORTED when the context's limit (BAZ_MUSIC_PIN_LIMIT_MIB, default 4096) would be exceeded or
 *       the union would have to replace a registration another context shares.  A range that cannot be locked as
 *       a whole is left entirely pageable (its own registrations it touches are dropped); process() works on it either way.
 *       Registrations are process-wide and counted: a range inside another context's registration takes a share of
 *       that one (two blocks on one stream buffer), and the memory is unlocked when the last holder lets go.
 *   baz_music_set_host_pinning(ctx, 1)       makes baz_music_process() do that for the input and spectrum ranges of
 *       every call before it copies (a lookup per call once they are known).  Default 0: the caller must guarantee that the
 *       memory outlives the registration -- true for scheduler buffers, not for temporaries.
 *   (A call below 64 MiB of traffic (BAZ_MUSIC_SINGLE_MIB) whose input and spectrum are page-locked -- by this or by their owner -- runs
 *   without copies: the kernels address the caller's buffers over PCIe, hipHostGetDevicePointer; BAZ_MUSIC_ZERO_COPY=0
 *   keeps the copies.)
 *   baz_music_host_unregister_all(ctx)       gives up every registration (share) of this context (also done by destroy);
 *       call it before the buffers are unmapped (the host block does in stop()).
 *   baz_music_host_pinned_bytes(ctx)         bytes this context holds locked. */
BAZ_MUSIC_API int baz_music_host_register(baz_music_ctx* ctx, const void* p, size_t bytes);
BAZ_MUSIC_API int baz_music_set_host_pinning(baz_music_ctx* ctx, int enable);
BAZ_MUSIC_API int baz_music_host_unregister_all(baz_music_ctx* ctx);
BAZ_MUSIC_API uint64_t baz_music_host_pinned_bytes(baz_music_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* INCLUDED_BAZ_MUSIC_HIP_H */
