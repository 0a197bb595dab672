/* -*- c++ -*- */
/* Host side of the MI355X MUSIC-DoA block: argument checking, table flattening and buffer
 * marshalling across the C-ABI (include/baz_music_hip.h).  Mirrors the roles of
 * /root/reference/lib/baz_music_doa.cc:29-33 (factory), :35-53 (constructor/ports/banner),
 * :60-70 (setter) and :72-161 (work); all arithmetic of :74-155 runs in the HIP kernels. */
#ifdef HAVE_CONFIG_H
#include "config.h"
#endif

#include <baz_music_doa.h>
#include <baz_music_hip.h>

#include <gnuradio/io_signature.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace {

/* resolution x m nested vectors -> the contiguous [bin][antenna] (re,im) float image of the ABI */
std::vector<float> flatten_response(const array_response_t& table, unsigned int m, unsigned int resolution)
{
    if (table.size() != resolution)
        throw std::invalid_argument("music_doa: array_response must have `resolution` rows");
    std::vector<float> flat((size_t)resolution * m * 2);
    for (unsigned int s = 0; s < resolution; ++s) {
        if (table[s].size() != m)
            throw std::invalid_argument("music_doa: every array_response row must have m entries");
        for (unsigned int t = 0; t < m; ++t) {
            flat[2 * ((size_t)s * m + t)] = table[s][t].real();
            flat[2 * ((size_t)s * m + t) + 1] = table[s][t].imag();
        }
    }
    return flat;
}

void check_config(unsigned int m, unsigned int n, unsigned int nsamples, unsigned int resolution)
{
    if (m == 0) throw std::invalid_argument("music_doa: m must be > 0");
    if (n == 0 || n >= m) throw std::invalid_argument("music_doa: need 0 < n < m");
    if (nsamples == 0 || (nsamples % m) != 0)
        throw std::invalid_argument("music_doa: nsamples must be a positive multiple of m");
    if (resolution == 0) throw std::invalid_argument("music_doa: resolution must be > 0");
}

}  // namespace

/* Independent block instances (BASELINE config 4: 64 streams in one flowgraph) are dealt over the node's GPUs
 * round-robin -- instance i -> device i mod G -- unless BAZ_MUSIC_DEVICE pins one; -1 = the current
 * HIP device when no gfx950 device is visible (create() then reports the error). */
int baz_music_doa_deal_device(unsigned int instance, int device_count)
{
    return device_count > 0 ? (int)(instance % (unsigned)device_count) : -1;
}

static int next_device()
{
    if (const char* v = getenv("BAZ_MUSIC_DEVICE")) return atoi(v);
    static std::atomic<unsigned> s_instances(0);
    return baz_music_doa_deal_device(s_instances.fetch_add(1), baz_music_device_count());
}

static long env_long(const char* name, long dflt, long lo, long hi)
{
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    char* end = NULL;
    const long x = strtol(v, &end, 10);
    if (end == v) return dflt;
    return x < lo ? lo : (x > hi ? hi : x);
}

baz_music_doa_sptr baz_make_music_doa(unsigned int m, unsigned int n, unsigned int nsamples,
                                      const array_response_t& array_response, unsigned int resolution)
{
    check_config(m, n, nsamples, resolution);   /* before the io_signature sizes are formed */
    return baz_music_doa_sptr(new baz_music_doa(m, n, nsamples, array_response, resolution));
}

baz_music_doa::baz_music_doa(unsigned int m, unsigned int n, unsigned int nsamples,
                             const array_response_t& array_response, unsigned int resolution)
    : gr::sync_block("music_doa",
                     gr::io_signature::make(1, 1, nsamples * sizeof(gr_complex)),
                     gr::io_signature::make3(1, 3, n * sizeof(float), n * sizeof(float),
                                             resolution * sizeof(float))),
      d_m(m), d_n(n), d_nsamples(nsamples), d_resolution(resolution),
      d_array_response(array_response), d_ctx(NULL), d_pin_buffers(false),
      d_cal_want(0), d_cal_min_quality(0.0), d_cal_quality(-1.0),
      d_wh_want(0), d_wh_status(0)
{
    const std::vector<float> flat = flatten_response(array_response, m, resolution);
    const int rc = baz_music_create(&d_ctx, m, n, nsamples, resolution, flat.data(), next_device());
    if (rc == BAZ_MUSIC_E_INVALID || rc == BAZ_MUSIC_E_UNSUPPORTED)
        throw std::invalid_argument(std::string("music_doa: ") + baz_music_strerror(rc));
    if (rc != BAZ_MUSIC_OK)
        throw std::runtime_error(std::string("music_doa: cannot open the gfx950 engine: ") + baz_music_strerror(rc));

    /* Scheduler hints.  The reference handles ONE item per work() call (.cc:74,160); here a call
     * is one launch sequence over all its items, so the block wants LARGE calls -- without giving up what the reference
     * guarantees: every item of a finite stream is processed, and an item is processed as soon as it has arrived.
     * GNU Radio sizes a buffer for 2 x (output multiple + history) items of every reader
     * (flat_flowgraph::allocate_buffer); the default is 64 KiB = 8 cfg2 items.  Two ways to ask for more:
     *   set_output_multiple(N)     also makes N the MINIMUM call: N items must have arrived before work() runs, and what
     *                              does not fill a last multiple when a finite source ends is never processed;
     *   set_history(H + 1)         declares H items of look-back the block never reads: the upstream buffer grows to
     *                              2 (H + 2) items, calls of up to ~H items form whenever the block is the bottleneck,
     *                              a single item is still a valid call, and nothing is lost at the end of a stream: the
     *                              runtime preloads the H look-back items as zeros (buffer_add_reader(.., history - 1)),
     *                              output i is computed from input i + H, i.e. from real item i.
     * The block uses the second: BAZ_MUSIC_INPUT_LOOKBACK = H (0 = none; default 2048 items, fewer where items are large:
     * H = 32 MiB / the larger of an input item and a spectrum row, between 8 and 2048 -- the doubly mapped circular buffers
     * are 2 (H + 2) items and must fit /dev/shm: config 2 gets 2048 (33.6 MB in, 59 MB spectrum), config 3 (144 KB rows)
     * 233, 64 antennas x 256 columns (128 KiB items) 256.  Round 5 doubled it: a host-fed call is one launch sequence that reads
     * its input over the link and then writes its spectrum over it, and its fixed costs shrink with the call -- config 2 with port 2 on
     * page-locked buffers: 2.05e6 items/s in 1,024-item calls, 2.24e6 in 2,048-item calls; without port 2 4.9e6 / 5.7e6
     * (profiles/r05_hostfed_calls.txt; cutting a call into overlapped sub-chunks LOSES on this stack, same file)), output multiple 1,
     * set_min_output_buffer(2 H) so that the output side admits the same calls (a call takes at most half a buffer).
     * BAZ_MUSIC_OUTPUT_MULTIPLE (1), BAZ_MUSIC_MIN_OUTPUT_BUFFER, BAZ_MUSIC_MAX_NOUTPUT (0 = no cap) override.
     * What the runtime makes of them (call sizes per work()) is modelled in gr_shim/gnuradio/flowgraph_model.h;
     * INTEGRATION.md 5 has the memory these requests cost and the measured rates. */
    const size_t big_item = std::max<size_t>((size_t)nsamples * sizeof(gr_complex), (size_t)resolution * sizeof(float));
    const long lookback_dflt = (long)std::max<size_t>(8, std::min<size_t>(2048, ((size_t)32 << 20) / big_item));
    const long lookback = env_long("BAZ_MUSIC_INPUT_LOOKBACK", lookback_dflt, 0, 1 << 20);
    const long multiple = env_long("BAZ_MUSIC_OUTPUT_MULTIPLE", 1, 1, 1 << 20);
    const long min_buffer = env_long("BAZ_MUSIC_MIN_OUTPUT_BUFFER", std::max(2 * lookback, multiple > 1 ? 8 * multiple : 0L), 0, 1L << 30);
    const long cap = env_long("BAZ_MUSIC_MAX_NOUTPUT", 0, 0, 1L << 30);
    set_history((unsigned)lookback + 1);
    set_output_multiple((int)multiple);
    if (min_buffer > 0) set_min_output_buffer(min_buffer);
    if (cap > 0) set_max_noutput_items((int)std::max(multiple, cap - cap % multiple));   /* the runtime does not round a cap */

    set_pin_buffers(env_long("BAZ_MUSIC_PIN_BUFFERS", 1, 0, 1) != 0);

    fprintf(stderr, "[%s<%li>] MUSIC DOA: M: %d, N: %d, # samples: %d, angular resolution: %d\n",
            name().c_str(), unique_id(), m, n, nsamples, resolution);
}

baz_music_doa::~baz_music_doa()
{
    baz_music_destroy(d_ctx);
}

int baz_music_doa::device() const { return baz_music_device(d_ctx); }

void baz_music_doa::set_pin_buffers(bool on)
{
    if (!on) (void)baz_music_host_unregister_all(d_ctx);
    (void)baz_music_set_host_pinning(d_ctx, on ? 1 : 0);
    d_pin_buffers = on;
}

unsigned long long baz_music_doa::pinned_bytes() const { return baz_music_host_pinned_bytes(d_ctx); }

bool baz_music_doa::start()
{
    (void)baz_music_reset_averaging(d_ctx);       /* a started flowgraph is a new stream */
    return true;
}

bool baz_music_doa::stop()
{
    (void)baz_music_host_unregister_all(d_ctx);   /* the flowgraph's buffers go away after this */
    return true;
}

void baz_music_doa::set_peak_mode(bool local_maxima)
{
    const int rc = baz_music_set_peak_mode(d_ctx, local_maxima ? 1 : 0);
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_peak_mode: ") + baz_music_strerror(rc));
}

void baz_music_doa::set_smoothing(unsigned int subarray, bool forward_backward)
{
    const int rc = baz_music_set_smoothing(d_ctx, subarray, forward_backward ? 1 : 0);
    if (rc == BAZ_MUSIC_E_INVALID)
        throw std::invalid_argument("music_doa: set_smoothing: subarray must satisfy n < subarray <= m, and the array response "
                                    "must be shift invariant (subarray < m) / centro-symmetric (forward_backward)");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_smoothing: ") + baz_music_strerror(rc));
}

void baz_music_doa::set_order_mode(int criterion)
{
    const int rc = baz_music_set_order_mode(d_ctx, criterion);
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: set_order_mode: criterion must be 0 (fixed n), 1 (MDL) or 2 (AIC)");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_order_mode: ") + baz_music_strerror(rc));
}

void baz_music_doa::set_refine_mode(bool parabolic)
{
    const int rc = baz_music_set_refine_mode(d_ctx, parabolic ? 1 : 0);
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_refine_mode: ") + baz_music_strerror(rc));
}

void baz_music_doa::set_power_mode(int mode)
{
    const int rc = baz_music_set_power_mode(d_ctx, mode);
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: set_power_mode: mode must be 0 (off), 1 (estimates) or 2 (estimates on the lvl port)");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_power_mode: ") + baz_music_strerror(rc));
}

void baz_music_doa::set_estimator(int kind)
{
    const int rc = baz_music_set_estimator(d_ctx, kind);
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: set_estimator: kind must be 0 (MUSIC), 1 (Capon) or 2 (Bartlett)");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_estimator: ") + baz_music_strerror(rc));
}

std::vector<double> baz_music_doa::last_powers(unsigned int count)
{
    std::vector<double> out(count);
    const int rc = baz_music_last_powers(d_ctx, out.data(), count);
    if (rc < 0) throw std::runtime_error(std::string("music_doa: last_powers: ") + baz_music_strerror(rc));
    out.resize((size_t)rc);
    return out;
}

void baz_music_doa::set_beam_mode(int mode, double loading)
{
    const int rc = baz_music_set_beam_mode(d_ctx, mode, loading);
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: set_beam_mode: mode must be 0 (off) or 1 (MVDR), loading finite and >= 0");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_beam_mode: ") + baz_music_strerror(rc));
}

std::vector<gr_complex> baz_music_doa::last_beams(unsigned int items)
{
    const size_t per = (size_t)d_n * (d_nsamples / d_m);
    std::vector<gr_complex> out((size_t)items * per);
    const int rc = baz_music_last_beams(d_ctx, reinterpret_cast<float*>(out.data()), items);
    if (rc < 0) throw std::runtime_error(std::string("music_doa: last_beams: ") + baz_music_strerror(rc));
    out.resize((size_t)rc * per);
    return out;
}

void baz_music_doa::set_averaging(unsigned int window, double forgetting)
{
    const int rc = baz_music_set_averaging(d_ctx, window, forgetting);
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: set_averaging: 1 <= window <= 64 and 0 < forgetting <= 1 are required");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_averaging: ") + baz_music_strerror(rc));
}

void baz_music_doa::reset_averaging()
{
    const int rc = baz_music_reset_averaging(d_ctx);
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: reset_averaging: no context");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: reset_averaging: ") + baz_music_strerror(rc));
}

void baz_music_doa::set_calibration(const std::vector<gr_complex>& gamma)
{
    if (!gamma.empty() && gamma.size() != d_m) throw std::invalid_argument("music_doa: set_calibration: gamma must hold m values (or none: off)");
    const int rc = baz_music_set_calibration(d_ctx, gamma.empty() ? NULL : reinterpret_cast<const float*>(gamma.data()));
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: set_calibration: every gain must be finite and nonzero");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_calibration: ") + baz_music_strerror(rc));
}

std::vector<gr_complex> baz_music_doa::calibration()
{
    std::vector<gr_complex> gamma(d_m);
    int on = 0;
    const int rc = baz_music_get_calibration(d_ctx, reinterpret_cast<float*>(gamma.data()), &on);
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: calibration: ") + baz_music_strerror(rc));
    if (!on) gamma.clear();
    return gamma;
}

void baz_music_doa::calibrate_next(unsigned int items, const std::vector<gr_complex>& ref, double min_quality)
{
    if (items == 0 || ref.size() != d_m || !(min_quality >= 0.0 && min_quality <= 1.0))
        throw std::invalid_argument("music_doa: calibrate_next: items > 0, m reference values and 0 <= min_quality <= 1 are required");
    for (unsigned int r = 0; r < d_m; ++r) {
        const float re = ref[r].real(), im = ref[r].imag();
        if (!(re - re == 0.0f) || !(im - im == 0.0f) || (re == 0.0f && im == 0.0f))
            throw std::invalid_argument("music_doa: calibrate_next: every reference value must be finite and nonzero");
    }
    gr::thread::scoped_lock guard(d_cal_mutex);
    d_cal_items.clear();
    d_cal_items.reserve((size_t)items * d_nsamples);
    d_cal_ref = ref;
    d_cal_min_quality = min_quality;
    d_cal_quality = -1.0;
    d_cal_want = items;
}

double baz_music_doa::last_calibration_quality()
{
    gr::thread::scoped_lock guard(d_cal_mutex);
    return d_cal_quality;
}

void baz_music_doa::set_noise_covariance(const std::vector<std::complex<double> >& rn)
{
    if (!rn.empty() && rn.size() != (size_t)d_m * d_m)
        throw std::invalid_argument("music_doa: set_noise_covariance: rn must hold m*m values, row-major (or none: off)");
    const int rc = baz_music_set_noise_covariance(d_ctx, rn.empty() ? NULL : reinterpret_cast<const double*>(rn.data()));
    if (rc == BAZ_MUSIC_E_INVALID)
        throw std::invalid_argument("music_doa: set_noise_covariance: rn must be finite, Hermitian positive definite and well above rank deficiency");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_noise_covariance: ") + baz_music_strerror(rc));
}

std::vector<std::complex<double> > baz_music_doa::noise_covariance()
{
    std::vector<std::complex<double> > rn((size_t)d_m * d_m);
    int on = 0;
    const int rc = baz_music_get_noise_covariance(d_ctx, reinterpret_cast<double*>(rn.data()), &on);
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: noise_covariance: ") + baz_music_strerror(rc));
    if (!on) rn.clear();
    return rn;
}

void baz_music_doa::set_beamspace(const std::vector<std::complex<double> >& T, unsigned int B, bool normalise)
{
    if (B != 0 && T.size() != (size_t)d_m * B)
        throw std::invalid_argument("music_doa: set_beamspace: T must hold m*B values, row-major [antenna][beam] (or B = 0: off)");
    const int rc = baz_music_set_beamspace(d_ctx, B, B ? reinterpret_cast<const double*>(T.data()) : NULL, normalise ? 1 : 0);
    if (rc == BAZ_MUSIC_E_INVALID)
        throw std::invalid_argument("music_doa: set_beamspace: n < B <= min(m, 16), B >= 2, and T finite without an all-zero column are required");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_beamspace: ") + baz_music_strerror(rc));
}

double baz_music_doa::set_beamspace_sector(unsigned int bin_lo, unsigned int bin_count, unsigned int B, bool normalise)
{
    std::vector<float> flat;
    {
        gr::thread::scoped_lock guard(d_mutex);
        flat = flatten_response(d_array_response, d_m, d_resolution);
    }
    std::vector<std::complex<double> > T((size_t)d_m * (B ? B : 1));
    double captured = 0.0;
    const int rc = baz_music_beamspace_design(d_m, d_resolution, flat.data(), bin_lo, bin_count, B, reinterpret_cast<double*>(T.data()), &captured);
    if (rc == BAZ_MUSIC_E_INVALID)
        throw std::invalid_argument("music_doa: set_beamspace_sector: 1 <= bin_count <= resolution and 1 <= B <= min(m, 16) are required");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_beamspace_sector: ") + baz_music_strerror(rc));
    set_beamspace(T, B, normalise);
    return captured;
}

std::vector<std::complex<double> > baz_music_doa::beamspace()
{
    uint32_t B = 0;
    int rc = baz_music_get_beamspace(d_ctx, &B, NULL, NULL);
    std::vector<std::complex<double> > T((size_t)d_m * B);
    if (rc == BAZ_MUSIC_OK && B) {
        uint32_t B2 = 0;
        rc = baz_music_get_beamspace(d_ctx, &B2, reinterpret_cast<double*>(T.data()), NULL);
        if (rc == BAZ_MUSIC_OK && B2 != B) T.clear();      /* (the setting changed in between: report it as off) */
    }
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: beamspace: ") + baz_music_strerror(rc));
    return T;
}

namespace {
/* S tables back to back, as baz_music_set_subbands takes them */
std::vector<float> flatten_subband_tables(const std::vector<array_response_t>& tables, unsigned int m, unsigned int resolution)
{
    std::vector<float> flat;
    flat.reserve(tables.size() * (size_t)resolution * m * 2);
    for (size_t s = 0; s < tables.size(); ++s) {
        const std::vector<float> one = flatten_response(tables[s], m, resolution);
        flat.insert(flat.end(), one.begin(), one.end());
    }
    return flat;
}
}  // namespace

void baz_music_doa::set_subbands(unsigned int F, const std::vector<unsigned int>& bins, const std::vector<array_response_t>& tables, int combine)
{
    if (F == 0) {
        const int rc = baz_music_set_subbands(d_ctx, 0, 0, NULL, NULL, 0);
        if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_subbands: ") + baz_music_strerror(rc));
        return;
    }
    if (bins.empty() || tables.size() != bins.size())
        throw std::invalid_argument("music_doa: set_subbands: one table per used subband is required");
    const std::vector<float> flat = flatten_subband_tables(tables, d_m, d_resolution);
    const std::vector<uint32_t> k(bins.begin(), bins.end());
    const int rc = baz_music_set_subbands(d_ctx, F, (uint32_t)k.size(), k.data(), flat.data(), combine);
    if (rc == BAZ_MUSIC_E_INVALID)
        throw std::invalid_argument("music_doa: set_subbands: 2 <= F <= 64 dividing nsamples / m, 1 .. 32 distinct bins below F, finite tables "
                                    "and combine 0 or 1 are required");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_subbands: ") + baz_music_strerror(rc));
}

void baz_music_doa::set_subband_tables(const std::vector<array_response_t>& tables)
{
    uint32_t S = 0;
    int rc = baz_music_get_subbands(d_ctx, NULL, &S, NULL, NULL);
    if (rc == BAZ_MUSIC_OK && S && tables.size() != S)
        throw std::invalid_argument("music_doa: set_subband_tables: one table per used subband is required");
    if (rc == BAZ_MUSIC_OK) {
        const std::vector<float> flat = flatten_subband_tables(tables, d_m, d_resolution);
        rc = flat.empty() ? BAZ_MUSIC_E_INVALID : baz_music_set_subband_tables(d_ctx, flat.data());
    }
    if (rc == BAZ_MUSIC_E_INVALID) throw std::invalid_argument("music_doa: set_subband_tables: S finite tables are required");
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: set_subband_tables: ") + baz_music_strerror(rc));
}

std::vector<unsigned int> baz_music_doa::subbands()
{
    uint32_t F = 0, S = 0, bins[BAZ_MUSIC_MAX_SUBBANDS] = {0};
    int combine = 0;
    const int rc = baz_music_get_subbands(d_ctx, &F, &S, bins, &combine);
    if (rc != BAZ_MUSIC_OK) throw std::runtime_error(std::string("music_doa: subbands: ") + baz_music_strerror(rc));
    std::vector<unsigned int> out;
    if (F) {
        out.push_back(F);
        out.push_back((unsigned int)combine);
        out.insert(out.end(), bins, bins + S);
    }
    return out;
}

void baz_music_doa::whiten_next(unsigned int items)
{
    if (items == 0) throw std::invalid_argument("music_doa: whiten_next: items > 0 is required");
    gr::thread::scoped_lock guard(d_wh_mutex);
    d_wh_items.clear();
    d_wh_items.reserve((size_t)items * d_nsamples);
    d_wh_status = -1;
    d_wh_want = items;
}

int baz_music_doa::last_whitening_status()
{
    gr::thread::scoped_lock guard(d_wh_mutex);
    return d_wh_status;
}

std::vector<unsigned char> baz_music_doa::last_orders(unsigned int count)
{
    std::vector<unsigned char> out(count);
    const int rc = baz_music_last_orders(d_ctx, out.data(), count);
    if (rc < 0) throw std::runtime_error(std::string("music_doa: last_orders: ") + baz_music_strerror(rc));
    out.resize((size_t)rc);
    return out;
}

void baz_music_doa::set_array_response(const array_response_t& array_response)
{
    const std::vector<float> flat = flatten_response(array_response, d_m, d_resolution);
    fprintf(stderr, "[%s<%li>] Updating array response\n", name().c_str(), unique_id());

    gr::thread::scoped_lock guard(d_mutex);
    const int rc = baz_music_set_table(d_ctx, flat.data());   /* serialised against work() inside */
    if (rc != BAZ_MUSIC_OK)
        throw std::runtime_error(std::string("music_doa: set_array_response: ") + baz_music_strerror(rc));
    d_array_response = array_response;
}

array_response_t baz_music_doa::array_response()
{
    gr::thread::scoped_lock guard(d_mutex);
    return d_array_response;
}

int baz_music_doa::work(int noutput_items, gr_vector_const_void_star& input_items,
                        gr_vector_void_star& output_items)
{
    if (noutput_items <= 0) return 0;
    if (input_items.empty() || output_items.empty()) return -1;

    /* input_items[0] points at the OLDEST look-back item (history() - 1 of them precede the item output 0 belongs to) */
    const float* in = static_cast<const float*>(input_items[0]) + (size_t)(history() - 1) * d_nsamples * 2;   /* gr_complex == (float re, float im) */
    float* ang = static_cast<float*>(output_items[0]);
    float* lvl = (output_items.size() > 1) ? static_cast<float*>(output_items[1]) : NULL;
    float* spectrum = (output_items.size() > 2) ? static_cast<float*>(output_items[2]) : NULL;

    const int rc = baz_music_process(d_ctx, in, (uint32_t)noutput_items, ang, lvl, spectrum);
    if (rc < 0) {
        fprintf(stderr, "[%s<%li>] MUSIC DOA: device error: %s (%s)\n", name().c_str(), unique_id(),
                baz_music_strerror(rc), baz_music_last_hip_error(d_ctx));
        return -1;   /* WORK_DONE */
    }

    /* calibrate_next: this call's items join the capture; once it is complete, one estimate, applied (to the calls after this one)
     * when its quality allows.  A failing estimate disarms and reports quality 0; the stream goes on. */
    gr::thread::scoped_lock guard(d_cal_mutex);
    if (d_cal_want) {
        const size_t have = d_cal_items.size() / d_nsamples;
        const size_t take = std::min<size_t>((size_t)noutput_items, d_cal_want - have);
        const gr_complex* items = reinterpret_cast<const gr_complex*>(in);
        d_cal_items.insert(d_cal_items.end(), items, items + take * d_nsamples);
        if (have + take == d_cal_want) {
            std::vector<double> gamma(2 * (size_t)d_m);
            double quality = 0.0;
            int rc2 = baz_music_calibrate(d_ctx, reinterpret_cast<const float*>(d_cal_items.data()), d_cal_want,
                                          reinterpret_cast<const float*>(d_cal_ref.data()), gamma.data(), &quality, NULL);
            if (rc2 == BAZ_MUSIC_OK && quality > 0.0 && quality >= d_cal_min_quality) {
                std::vector<float> g32(gamma.begin(), gamma.end());      /* complex128 -> complex64, round to nearest */
                rc2 = baz_music_set_calibration(d_ctx, g32.data());
            }
            if (rc2 != BAZ_MUSIC_OK) {
                fprintf(stderr, "[%s<%li>] MUSIC DOA: calibrate_next: %s\n", name().c_str(), unique_id(), baz_music_strerror(rc2));
                quality = 0.0;
            }
            d_cal_quality = quality;
            d_cal_want = 0;
            std::vector<gr_complex>().swap(d_cal_items);
        }
    }

    /* whiten_next: this call's items join the noise-only capture; once it is complete, their mean covariance becomes the noise
     * covariance in force (for the calls after this one).  A failure disarms and is reported by last_whitening_status(); the
     * setting in force stays and the stream goes on. */
    gr::thread::scoped_lock wguard(d_wh_mutex);
    if (d_wh_want) {
        const size_t have = d_wh_items.size() / d_nsamples;
        const size_t take = std::min<size_t>((size_t)noutput_items, d_wh_want - have);
        const gr_complex* items = reinterpret_cast<const gr_complex*>(in);
        d_wh_items.insert(d_wh_items.end(), items, items + take * d_nsamples);
        if (have + take == d_wh_want) {
            std::vector<double> rbar(2 * (size_t)d_m * d_m);
            int rc2 = baz_music_mean_covariance(d_ctx, reinterpret_cast<const float*>(d_wh_items.data()), d_wh_want, rbar.data());
            if (rc2 == BAZ_MUSIC_OK) rc2 = baz_music_set_noise_covariance(d_ctx, rbar.data());
            if (rc2 != BAZ_MUSIC_OK)
                fprintf(stderr, "[%s<%li>] MUSIC DOA: whiten_next: %s\n", name().c_str(), unique_id(), baz_music_strerror(rc2));
            d_wh_status = rc2;
            d_wh_want = 0;
            std::vector<gr_complex>().swap(d_wh_items);
        }
    }
    return noutput_items;
}
