/* -*- c++ -*- */
/* MUSIC direction-of-arrival estimator block, MI355X (gfx950) implementation.
 *
 * Drop-in for gr-baz's block of the same name: the public surface below is the one declared in
 * /root/reference/lib/baz_music_doa.h:29-60 -- sptr typedef (:30), antenna_response_t /
 * array_response_t / doa_t (:32-34), the factory (:36), a gr::sync_block subclass with a private
 * constructor and friend factory (:38-43), work() (:48) and set_array_response() (:59) -- so the SWIG
 * stanza (swig/baz_swig.i:560-574), music_doa_helper.py and existing flowgraphs keep working.
 * What differs is private: instead of Armadillo temporaries the block owns one baz_music_ctx
 * (include/baz_music_hip.h) and marshals the scheduler's buffers across that C-ABI into the HIP
 * kernels.  There is no CPU arithmetic in this block.
 */
#ifndef INCLUDED_BAZ_MUSIC_DOA_H
#define INCLUDED_BAZ_MUSIC_DOA_H

#include <gnuradio/sync_block.h>
#include <gnuradio/thread/thread.h>

#include <complex>
#include <utility>
#include <vector>

struct baz_music_ctx;   /* include/baz_music_hip.h */

class baz_music_doa;
typedef boost::shared_ptr<baz_music_doa> baz_music_doa_sptr;

typedef std::vector<gr_complex> antenna_response_t;      /* one steering vector, length m */
typedef std::vector<antenna_response_t> array_response_t; /* resolution of those */
typedef std::pair<double, double> doa_t;                  /* (angle in degrees, strength) */

/* m antennas, n expected emitters (0 < n < m), nsamples complex samples per item (all antennas
 * interleaved, nsamples % m == 0), array_response = resolution x m steering table.
 * Throws std::invalid_argument on a bad configuration and std::runtime_error when no gfx950 device
 * can be opened (the reference only assert()s, lib/baz_music_doa.cc:45-50). */
baz_music_doa_sptr baz_make_music_doa(unsigned int m, unsigned int n, unsigned int nsamples,
                                      const array_response_t& array_response, unsigned int resolution);

class baz_music_doa : public gr::sync_block
{
private:
    friend baz_music_doa_sptr baz_make_music_doa(unsigned int m, unsigned int n, unsigned int nsamples,
                                                 const array_response_t& array_response,
                                                 unsigned int resolution);

    baz_music_doa(unsigned int m, unsigned int n, unsigned int nsamples,
                  const array_response_t& array_response, unsigned int resolution);

public:
    ~baz_music_doa();

    /* in:  input_items[0]  = noutput_items items of nsamples gr_complex
     * out: output_items[0] = ang (n floats/item), [1] = lvl (n floats/item, optional),
     *      [2] = spectrum (resolution floats/item, optional).
     * Processes ALL noutput_items and returns that count (the reference handles one item per call,
     * lib/baz_music_doa.cc:160; the produced streams are identical).  -1 on a fatal device error. */
    int work(int noutput_items, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items);

    /* Thread-safe table replacement (python: music_doa_helper.set_frequency). */
    void set_array_response(const array_response_t& array_response);
    /* Extension, off by default (not in the reference): emit the n strongest local maxima of the pseudo-spectrum
     * instead of the n strongest bins (baz_music_set_peak_mode, include/baz_music_hip.h). */
    void set_peak_mode(bool local_maxima);
    /* Extension, off by default (not in the reference): forward-backward averaging and/or spatial smoothing over subarrays
     * of `subarray` antennas, for coherent emitters (baz_music_set_smoothing, include/baz_music_hip.h); (m, false) is off.
     * Throws std::invalid_argument when the arguments or the array response do not allow the mode. */
    void set_smoothing(unsigned int subarray, bool forward_backward);
    /* Extension, off by default (not in the reference): per-item emitter count, 1 = MDL, 2 = AIC, 0 = the fixed n
     * (baz_music_set_order_mode, include/baz_music_hip.h): n becomes the largest count, an item with count k emits k pairs and
     * then (0, 0).  last_orders: the counts of the first `count` items of the last work() call. */
    void set_order_mode(int criterion);
    std::vector<unsigned char> last_orders(unsigned int count);
    /* Extension, off by default (not in the reference): move every reported angle off the steering grid by a parabolic fit of
     * the MUSIC denominator at its bin and the two neighbours (baz_music_set_refine_mode, include/baz_music_hip.h); meant to be
     * used with set_peak_mode(true).  lvl and the spectrum port do not change. */
    void set_refine_mode(bool parabolic);
    /* Extension, off by default (not in the reference): a Capon power estimate 1 / Re(a^H R^-1 a) per reported entry, in the units
     * of the covariance (baz_music_set_power_mode, include/baz_music_hip.h).  mode 1 computes them and leaves every port as it is,
     * mode 2 additionally puts them on the lvl port; last_powers: the estimates of the first `count` (item, slot) entries of the
     * last work() call in fp64. */
    void set_power_mode(int mode);
    std::vector<double> last_powers(unsigned int count);
    /* Extension, off by default (not in the reference): the spectrum estimator (baz_music_set_estimator, include/baz_music_hip.h).
     * kind 0 is MUSIC (the reference), 1 the Capon and 2 the Bartlett spectrum: powers in the units of the covariance for every bin,
     * no emitter count needed; ang / lvl are picked from the float32 spectrum. */
    void set_estimator(int kind);
    /* Extension, off by default (not in the reference): the MVDR beamformer output y = w^H X of every reported entry over the item's
     * own snapshots, w = R^-1 a / (a^H R^-1 a) (baz_music_set_beam_mode, include/baz_music_hip.h).  mode 1 computes them and leaves
     * every port as it is; loading >= 0 adds loading * mean diagonal to R's diagonal.  last_beams: the beams of the first `items`
     * items of the last work() call, [item][slot][K].  Not available while smoothing is on. */
    void set_beam_mode(int mode, double loading = 0.0);
    std::vector<gr_complex> last_beams(unsigned int items);
    /* Extension, off by default (not in the reference): every item's covariance becomes the weighted mean over the last `window`
     * items of the stream, weights forgetting^age (baz_music_set_averaging, include/baz_music_hip.h); window 1 is off.  The output
     * rate does not change.  reset_averaging forgets the history (start() does).  Throws std::invalid_argument unless
     * 1 <= window <= 64 and 0 < forgetting <= 1. */
    void set_averaging(unsigned int window, double forgetting);
    void reset_averaging();
    /* Extension, off by default (not in the reference): per-antenna gain / phase calibration -- the table in force becomes
     * gamma_r a_r(bin), across set_array_response too (baz_music_set_calibration, include/baz_music_hip.h).  An empty vector is off.
     * calibration(): the gains in force (empty while off).  calibrate_next arms an estimate from a pilot: the block copies the next
     * `items` items that pass through work() (across as many calls as it takes; their outputs are untouched), calls
     * baz_music_calibrate once with the pilot's ideal response `ref` and applies the result, rounded to complex64, only when its
     * quality is >= min_quality.  last_calibration_quality(): -1 while armed (and before the first estimate), else the quality of
     * the last estimate.  Not available while smoothing is on.  Throws std::invalid_argument for a vector that does not hold m
     * finite nonzero values, items == 0 or a min_quality outside [0, 1]. */
    void set_calibration(const std::vector<gr_complex>& gamma);
    std::vector<gr_complex> calibration();
    void calibrate_next(unsigned int items, const std::vector<gr_complex>& ref, double min_quality);
    double last_calibration_quality();
    /* Extension, off by default (not in the reference): noise pre-whitening -- with the noise covariance rn = L L^H (m*m values,
     * row-major; its lower triangle is read) the EVD decomposes W R W^H and the table in force becomes W a, W = L^-1, across
     * set_array_response and set_calibration too (baz_music_set_noise_covariance, include/baz_music_hip.h).  An empty vector is off.
     * noise_covariance(): the matrix in force (empty while off).  whiten_next arms a measurement: the block copies the next `items`
     * items that pass through work() (a noise-only capture; across as many calls as it takes; their outputs are untouched), calls
     * baz_music_mean_covariance once and hands the result to the setter.  last_whitening_status(): -1 while armed, 0 once applied
     * (and before the first measurement), else the error code of the step that failed (the setting in force stays).  Not available
     * while smoothing, the beam mode or an estimator other than MUSIC is on.  Throws std::invalid_argument for a vector that does
     * not hold m*m finite values of a positive definite matrix, or items == 0. */
    void set_noise_covariance(const std::vector<std::complex<double> >& rn);
    std::vector<std::complex<double> > noise_covariance();
    void whiten_next(unsigned int items);
    int last_whitening_status();
    /* Extension, off by default (not in the reference): beamspace MUSIC -- every snapshot is projected onto B <= 16 beams, y = T^H x
     * (T: m*B values, row-major [antenna][beam]), and the estimate runs on the table T^H a with every opt-in mode of this class, also
     * for 17 .. 64 antennas (baz_music_set_beamspace, include/baz_music_hip.h).  B = 0 is off.  set_beamspace_sector designs T for the
     * `bin_count` bins from `bin_lo` (wrapping) of the array response in force (baz_music_beamspace_design), sets it and returns the
     * captured fraction.  beamspace(): the T in force (m*B values; empty while off).  Not available while smoothing, a calibration,
     * noise pre-whitening or the beam mode is on.  Throws std::invalid_argument unless n < B <= min(m, 16), B >= 2 and T is finite
     * without an all-zero column. */
    void set_beamspace(const std::vector<std::complex<double> >& T, unsigned int B, bool normalise = false);
    double set_beamspace_sector(unsigned int bin_lo, unsigned int bin_count, unsigned int B, bool normalise = false);
    std::vector<std::complex<double> > beamspace();
    /* Extension, off by default (not in the reference): wideband (subband) MUSIC -- every item is cut into blocks of F samples, an
     * F-point DFT per antenna separates the used subbands `bins` (distinct DFT indices below F), the estimator runs per subband on
     * tables[s] and the spectra are combined (0: harmonic, the sum of the MUSIC denominators; 1: arithmetic) into the row the pickers
     * read (baz_music_set_subbands, include/baz_music_hip.h).  F = 0 is off.  set_subband_tables retunes all tables at once.
     * subbands(): F, combine, then the bins in force (empty while off).  Up to 16 antennas; not available while smoothing, beamspace,
     * a calibration, noise pre-whitening, the emitter-count mode, refinement, power mode or the beam mode is on.  Throws
     * std::invalid_argument unless 2 <= F <= 64 divides nsamples / m, the 1 .. 32 bins are distinct and below F, the tables are finite
     * and combine is 0 or 1. */
    void set_subbands(unsigned int F, const std::vector<unsigned int>& bins, const std::vector<array_response_t>& tables, int combine = 0);
    void set_subband_tables(const std::vector<array_response_t>& tables);
    std::vector<unsigned int> subbands();

    /* Page-locking of the scheduler's stream buffers (baz_music_set_host_pinning, include/baz_music_hip.h): work()
     * registers the ranges it is handed the first time it sees them, stop() and the destructor release them.  On by
     * default (BAZ_MUSIC_PIN_BUFFERS=0 turns it off): GNU Radio's buffers outlive every work() call.  A caller that
     * hands work() temporaries (the pybind stand-in does) must switch it off. */
    void set_pin_buffers(bool on);
    bool pin_buffers() const { return d_pin_buffers; }
    unsigned long long pinned_bytes() const;
    bool start();   /* gr::block::start */
    bool stop();    /* gr::block::stop: releases the page locks while the buffers still exist */

    unsigned int m() const { return d_m; }
    unsigned int n() const { return d_n; }
    unsigned int nsamples() const { return d_nsamples; }
    unsigned int resolution() const { return d_resolution; }
    array_response_t array_response();
    /* HIP device this instance's context lives on (see baz_music_doa_deal_device). */
    int device() const;

private:
    unsigned int d_m;
    unsigned int d_n;
    unsigned int d_nsamples;
    unsigned int d_resolution;
    array_response_t d_array_response;   /* host copy, guarded by d_mutex */
    gr::thread::mutex d_mutex;
    baz_music_ctx* d_ctx;                /* device-side state (table, workspace, stream) */
    bool d_pin_buffers;
    /* calibrate_next: guarded by d_cal_mutex (its own: work() must never wait for a retune that holds d_mutex) */
    gr::thread::mutex d_cal_mutex;
    unsigned int d_cal_want;            /* items to capture; 0: not armed */
    std::vector<gr_complex> d_cal_items; /* the items captured so far */
    std::vector<gr_complex> d_cal_ref;
    double d_cal_min_quality;
    double d_cal_quality;
    /* whiten_next: guarded by d_wh_mutex (its own, as d_cal_mutex is) */
    gr::thread::mutex d_wh_mutex;
    unsigned int d_wh_want;             /* items to capture; 0: not armed */
    std::vector<gr_complex> d_wh_items;  /* the items captured so far */
    int d_wh_status;
};

/* Placement rule of independent block instances (BASELINE config 4: 64 streams in one flowgraph; SURVEY.md 8e,
 * stream s -> GPU s mod G): the instance-th block made by this process goes to device instance % device_count;
 * -1 (= the current HIP device) when no gfx950 device is visible.  BAZ_MUSIC_DEVICE pins every instance instead. */
int baz_music_doa_deal_device(unsigned int instance, int device_count);

#endif /* INCLUDED_BAZ_MUSIC_DOA_H */
