"""MUSIC DOA helper -- python-3 counterpart of /root/reference/python/music_doa_helper.py.

Same public surface: unit_vect(theta), calculate_antenna_array_response(antenna_array,
angular_resolution, l) (:29-46) and class music_doa_helper(m, n, nsamples, angular_resolution,
frequency, array_spacing, antenna_array, output_spectrum=False) with set_frequency() (:48-103), used
by grc/baz_music_doa.xml:6-8.  The steering-table formula, wavelength, array scaling, the
nsamples % m check and the 2-or-3 output signature are the reference's (python-3 syntax).

With GNU Radio installed the class is a gr.hier_block2 wired exactly like the reference (:61-96).
Without it (this container) it is a plain object with the same attributes plus work(items), so the
helper -> baz.music_doa -> host block -> C-ABI -> HIP chain can be exercised end to end.
"""
import os

import numpy

try:                                    # real GNU Radio host
    from gnuradio import gr             # noqa: F401
    _HAVE_GR = True
except ImportError:                     # this container / the GPU box
    gr = None
    _HAVE_GR = False

C_LIGHT = 299792458.0                   # python/music_doa_helper.py:55


def unit_vect(theta):
    return numpy.array([numpy.cos(theta), numpy.sin(theta)])


def _fma(a, b, c):
    """round(a * b + c) in float64 without an fma instruction: the product exactly as p + e (Veltkamp / Dekker), the sum of the
    three terms by a compensated addition.  (Not correctly rounded in every halfway case; it is only ever used to CONFIRM a table
    bit for bit, so an error here can only send the helper to its per-element loop.)"""
    p = a * b
    ta, tb = 134217729.0 * a, 134217729.0 * b
    ah = ta - (ta - a)
    bh = tb - (tb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


# u0 a0 + u1 a1 as a BLAS dot of length two may round it: the second product fused onto the first, the first onto the second, or unfused
_TWO_TERM_FORMS = (lambda u0, a0, u1, a1: _fma(u1, a1, u0 * a0),
                   lambda u0, a0, u1, a1: _fma(u0, a0, u1 * a1),
                   lambda u0, a0, u1, a1: u0 * a0 + u1 * a1)


def _phase_by_element(antennas, angular_resolution, l, steps=None):
    """The reference's loop (python/music_doa_helper.py:35-41): one numpy.inner per (step, antenna)."""
    steps = range(0, angular_resolution) if steps is None else steps
    phase = numpy.empty((len(steps), len(antennas)), dtype=numpy.float64)
    for k, step in enumerate(steps):
        angle = (step * 360.0 / angular_resolution) * (numpy.pi / 180.0)
        u = unit_vect(angle)
        for t, antenna in enumerate(antennas):
            phase[k, t] = numpy.inner(antenna, u) / l
    return phase


def calculate_antenna_array_response(antenna_array, angular_resolution, l):
    """response[step][antenna] = exp(-j 2 pi (p_antenna . u(theta_step)) / l), theta_step =
    step*360/angular_resolution degrees (python/music_doa_helper.py:32-46).  Returns a list of lists of
    python complex, which is what baz.music_doa's vector<vector<gr_complex>> typemap takes.

    The reference forms every phase with its own numpy.inner call: 288,000 of them at 8 antennas x 36,000 bins, 0.4 - 1.1 s
    per retune -- next to a set_array_response that takes 0.24 ms.  Here ONE numpy.inner over all steps and
    antennas forms them (the same two-term dot product per element, by the same BLAS: bit-identical wherever it was tried,
    20 x faster).  It is accepted only when (i) a sample of 64 rows recomputed the reference's way agrees bit for bit and (ii)
    EVERY element agrees bit for bit with a deterministic restatement of the rounding the sample shows (fused either way, or
    unfused: _TWO_TERM_FORMS) -- a BLAS whose blocked product, thread partition or tail rounds some rows differently fails
    (ii); in every other case the whole table is formed per element.  BAZ_MUSIC_HELPER_PER_ELEMENT=1 forces that loop."""
    antennas = [numpy.asarray(a, dtype=numpy.float64) for a in antenna_array]
    res = int(angular_resolution)
    phase = None
    if (res > 0 and len(antennas) > 0 and all(a.shape == (2,) for a in antennas)
            and os.environ.get("BAZ_MUSIC_HELPER_PER_ELEMENT", "0") in ("", "0")):     # (=1: the reference's loop, whatever it costs)
        angle = (numpy.arange(res) * 360.0 / res) * (numpy.pi / 180.0)
        u = numpy.stack([numpy.cos(angle), numpy.sin(angle)], axis=1)
        A = numpy.stack(antennas)
        fast = numpy.inner(u, A) / l
        sample = sorted(set([0, res - 1] + [(k * 2654435761) % res for k in range(1, 63)]))
        by_element = _phase_by_element(antennas, res, l, sample)
        if numpy.array_equal(fast[sample].view(numpy.int64), by_element.view(numpy.int64)):
            # The sample says what ONE dot product of this BLAS rounds like.  The matrix product may still round some block,
            # thread partition or tail differently: the WHOLE table is therefore compared with a deterministic
            # restatement of that rounding -- whichever of the three two-term forms reproduces the sample -- and any differing
            # element sends the table through the per-element loop.
            for form in _TWO_TERM_FORMS:
                cand = form(u[:, 0:1], A[None, :, 0], u[:, 1:2], A[None, :, 1]) / l
                if numpy.array_equal(cand[sample].view(numpy.int64), by_element.view(numpy.int64)):
                    if numpy.array_equal(cand.view(numpy.int64), fast.view(numpy.int64)):
                        phase = fast
                    break
    if phase is None:
        phase = _phase_by_element(antennas, res, l)
    response = numpy.exp(-1j * 2.0 * numpy.pi * phase)
    return response.tolist()


def _banner(h):
    print("MUSIC DOA Helper: M: %d, N: %d, # samples: %d, steps of %f degress, lambda: %f, array: %s" % (
        h.m, h.n, h.nsamples, (360.0 / h.angular_resolution), h.l, str(h.antenna_array)))


def _configure(h, m, n, nsamples, angular_resolution, frequency, array_spacing, antenna_array):
    h.m = m
    h.n = n
    h.nsamples = nsamples
    h.angular_resolution = angular_resolution
    h.l = C_LIGHT / frequency
    h.antenna_array = [[array_spacing * x, array_spacing * y] for [x, y] in antenna_array]
    if (nsamples % m) != 0:
        raise Exception("nsamples must be multiple of m")


def _make_impl(h):
    from . import music_doa as _music_doa
    h.array_response = calculate_antenna_array_response(h.antenna_array, h.angular_resolution, h.l)
    h.impl = _music_doa(h.m, h.n, h.nsamples, h.array_response, h.angular_resolution)


def _retune(h, frequency):
    h.l = C_LIGHT / frequency
    h.array_response = calculate_antenna_array_response(h.antenna_array, h.angular_resolution, h.l)
    h.impl.set_array_response(h.array_response)
    if getattr(h, "_subbands", None) is not None:      # the subband mode stays in force: all S tables at the new carrier, at once
        h.impl.set_subband_tables(_subband_tables(h))


def _set_smoothing(h, subarray, forward_backward):
    # EXTENSION, no reference counterpart: forward-backward averaging / spatial smoothing of the covariance (coherent
    # emitters), see include/baz_music_hip.h.  Stays in force across set_frequency(): a retuned ULA is still a ULA.
    h.impl.set_smoothing(int(subarray), bool(forward_backward))


def _set_order_mode(h, criterion):
    # EXTENSION, no reference counterpart: per-item emitter count ("mdl" / "aic" / None), see include/baz_music_hip.h.
    # n becomes the largest count; an output row holds the item's own count of pairs, then (0, 0).
    modes = {None: 0, "mdl": 1, "aic": 2}
    if criterion not in modes:
        raise ValueError("order mode must be 'mdl', 'aic' or None, not %r" % (criterion,))
    h.impl.set_order_mode(modes[criterion])


def _set_refine_mode(h, parabolic):
    # EXTENSION, no reference counterpart: sub-bin angles by a parabolic fit of the MUSIC denominator at each reported bin and
    # its two neighbours, see include/baz_music_hip.h.  Stays in force across set_frequency().
    h.impl.set_refine_mode(bool(parabolic))


def _set_power_mode(h, mode):
    # EXTENSION, no reference counterpart: a Capon power estimate 1 / Re(a^H R^-1 a) per reported entry (1: behind last_powers(),
    # 2: also on the lvl port), see include/baz_music_hip.h.  Stays in force across set_frequency().
    if mode not in (0, 1, 2):
        raise ValueError("power mode must be 0, 1 or 2, not %r" % (mode,))
    h.impl.set_power_mode(int(mode))


ESTIMATORS = {"music": 0, "capon": 1, "bartlett": 2}


def estimator_kind(kind):
    """0 / 1 / 2 for 0 / 1 / 2 or "music" / "capon" / "bartlett" (any letter case); ValueError otherwise."""
    if isinstance(kind, str):
        if kind.lower() not in ESTIMATORS:
            raise ValueError("estimator must be 0, 1, 2 or one of %s, not %r" % (sorted(ESTIMATORS), kind))
        return ESTIMATORS[kind.lower()]
    if isinstance(kind, bool) or kind not in (0, 1, 2):
        raise ValueError("estimator must be 0, 1, 2 or one of %s, not %r" % (sorted(ESTIMATORS), kind))
    return int(kind)


def _set_estimator(h, kind):
    # EXTENSION, no reference counterpart: the Capon (1) or Bartlett (2) spectrum in place of MUSIC (0, the reference), see
    # include/baz_music_hip.h.  Stays in force across set_frequency().
    h.impl.set_estimator(estimator_kind(kind))
    h._estimator = estimator_kind(kind)


def _set_beam_mode(h, mode, loading):
    # EXTENSION, no reference counterpart: the MVDR beamformer output y = w^H X per reported entry over the item's own snapshots
    # (behind last_beams()), see include/baz_music_hip.h.  Stays in force across set_frequency().
    if mode not in (0, 1):
        raise ValueError("beam mode must be 0 or 1, not %r" % (mode,))
    if not (loading >= 0.0 and loading < float("inf")):
        raise ValueError("loading must be finite and >= 0, not %r" % (loading,))
    h.impl.set_beam_mode(int(mode), float(loading))


def _set_calibration(h, gamma):
    # EXTENSION, no reference counterpart: per-antenna gain / phase calibration, the table in force becomes gamma_r * a_r(bin), see
    # include/baz_music_hip.h.  Stays in force across set_frequency(): the library keeps gamma and applies it to every later table
    # (h.array_response stays the uncalibrated one).
    if gamma is None:
        h.impl.set_calibration([])
        return
    g = [complex(x) for x in numpy.asarray(gamma).reshape(-1)]
    if len(g) != h.m:
        raise ValueError("gamma must hold m = %d complex values" % h.m)
    h.impl.set_calibration(g)


def _calibrate_next(h, items, pilot_bin, ref, min_quality):
    # EXTENSION: estimate gamma from the next `items` items of the stream, which carry a pilot whose ideal response is row
    # `pilot_bin` of the helper's own uncalibrated table, or `ref` ([1] * m: a noise source injected equally into all channels).
    if (pilot_bin is None) == (ref is None):
        raise ValueError("give either pilot_bin or ref")
    if pilot_bin is not None:
        if not 0 <= int(pilot_bin) < h.angular_resolution:
            raise ValueError("pilot_bin must be a bin of the table, not %r" % (pilot_bin,))
        ref = h.array_response[int(pilot_bin)]
    p = [complex(x) for x in numpy.asarray(ref).reshape(-1)]
    if len(p) != h.m:
        raise ValueError("ref must hold m = %d complex values" % h.m)
    h.impl.calibrate_next(int(items), p, float(min_quality))


def _set_noise_covariance(h, rn):
    # EXTENSION, no reference counterpart: noise pre-whitening with the m x m noise covariance rn = L L^H: the EVD decomposes
    # W R W^H and the table in force becomes W a, W = L^-1, see include/baz_music_hip.h.  Stays in force across set_frequency()
    # and set_calibration() (h.array_response stays the caller's table).
    if rn is None:
        h.impl.set_noise_covariance([])
        return
    R = numpy.asarray(rn, dtype=numpy.complex128)
    if R.shape != (h.m, h.m):
        raise ValueError("rn must be an m x m = %d x %d complex matrix" % (h.m, h.m))
    h.impl.set_noise_covariance([complex(x) for x in R.reshape(-1)])


def _noise_covariance(h):
    rn = h.impl.noise_covariance()
    return numpy.asarray(rn, dtype=numpy.complex128).reshape(h.m, h.m) if len(rn) else None


def _set_beamspace(h, T, normalise):
    # EXTENSION, no reference counterpart: beamspace MUSIC -- every snapshot projected onto B <= 16 beams, y = T^H x, the estimate on
    # the table T^H a with every opt-in mode, also for 17 .. 64 antennas, see include/baz_music_hip.h.  Stays in force across
    # set_frequency() (h.array_response stays the caller's table).
    if T is None:
        h.impl.set_beamspace([], 0, False)
        return
    t = numpy.asarray(T, dtype=numpy.complex128)
    if t.ndim != 2 or t.shape[0] != h.m:
        raise ValueError("T must be an m x B = %d x B complex matrix" % h.m)
    h.impl.set_beamspace([complex(x) for x in t.reshape(-1)], int(t.shape[1]), bool(normalise))


def _set_beamspace_sector(h, bin_lo, bin_count, beams, normalise):
    # EXTENSION: T = the `beams` principal eigenvectors of sum a a^H over the sector's bins of the table in force; returns the
    # captured fraction of that sum's trace.
    return float(h.impl.set_beamspace_sector(int(bin_lo), int(bin_count), int(beams), bool(normalise)))


def _beamspace(h):
    t = h.impl.beamspace()
    return numpy.asarray(t, dtype=numpy.complex128).reshape(h.m, -1) if len(t) else None


def subband_offset(k, block):
    """o(k): the frequency offset of DFT index k of a `block`-point DFT in units of sample_rate / block: k below ceil(block / 2),
    k - block from there on."""
    return k if k < (block + 1) // 2 else k - block


def subband_bins(block, occupied=0.75):
    """The DFT indices the subband mode uses: all k with |o(k)| / block <= occupied / 2, ascending."""
    block = int(block)
    if block < 2 or not (0.0 <= occupied <= 1.0):
        raise ValueError("subbands need a block of at least 2 samples and 0 <= occupied <= 1")
    return [k for k in range(block) if abs(subband_offset(k, block)) / block <= occupied / 2]


def subband_wavelengths(frequency, sample_rate, block, bins):
    """The wavelength of every used subband: C / (frequency + o(k) sample_rate / block)."""
    return [C_LIGHT / (frequency + subband_offset(k, block) * sample_rate / block) for k in bins]


def _subband_tables(h):
    sample_rate, block, bins = h._subbands
    return [calculate_antenna_array_response(h.antenna_array, h.angular_resolution, l)
            for l in subband_wavelengths(C_LIGHT / h.l, sample_rate, block, bins)]


def _set_subbands(h, sample_rate, block, occupied, combine):
    # EXTENSION, no reference counterpart: wideband (subband) MUSIC -- a `block`-point DFT per antenna, the estimate per used subband
    # on the array response at THAT subband's wavelength, the spectra combined, see include/baz_music_hip.h.  Stays in force across
    # set_frequency(), which recomputes the S tables (h.array_response stays the centre table).
    if sample_rate is None:
        h.impl.set_subbands(0, [], [], 0)
        h._subbands = None
        return
    bins = subband_bins(block, occupied)
    if combine is None:
        combine = 0 if getattr(h, "_estimator", 0) == 0 else 1        # harmonic under MUSIC, arithmetic for the Capon / Bartlett powers
    combine = {"harmonic": 0, "arithmetic": 1}.get(combine, combine)
    if isinstance(combine, bool) or combine not in (0, 1):
        raise ValueError("combine must be 0 / 'harmonic', 1 / 'arithmetic' or None, not %r" % (combine,))
    previous = getattr(h, "_subbands", None)
    h._subbands = (float(sample_rate), int(block), bins)
    try:
        h.impl.set_subbands(int(block), bins, _subband_tables(h), int(combine))
    except Exception:
        h._subbands = previous
        raise


def _whiten_next(h, items):
    # EXTENSION: measure the noise covariance from the next `items` items of the stream (a noise-only capture: emitters off,
    # or the antennas terminated) and switch the whitening on with it.
    if int(items) <= 0:
        raise ValueError("items must be > 0, not %r" % (items,))
    h.impl.whiten_next(int(items))


def _set_averaging(h, window, forgetting):
    # EXTENSION, no reference counterpart: the covariance of every item averaged over the last `window` items of the stream
    # (weights forgetting ** age), see include/baz_music_hip.h.  Stays in force across set_frequency(): covariances do not
    # depend on the table, so the history survives a retune as well.
    h.impl.set_averaging(int(window), float(forgetting))


if _HAVE_GR:

    class music_doa_helper(gr.hier_block2):
        def __init__(self, m, n, nsamples, angular_resolution, frequency, array_spacing, antenna_array,
                     output_spectrum=False):
            _configure(self, m, n, nsamples, angular_resolution, frequency, array_spacing, antenna_array)
            if output_spectrum:
                output_sig = gr.io_signature3(3, 3, (gr.sizeof_float * n), (gr.sizeof_float * n),
                                              (gr.sizeof_float * angular_resolution))
            else:
                output_sig = gr.io_signature2(2, 2, (gr.sizeof_float * n), (gr.sizeof_float * n))
            gr.hier_block2.__init__(self, "music_doa_helper",
                                    gr.io_signature(1, 1, (gr.sizeof_gr_complex * nsamples)), output_sig)
            _banner(self)
            _make_impl(self)
            self.connect(self, self.impl)
            self.connect((self.impl, 0), (self, 0))
            self.connect((self.impl, 1), (self, 1))
            if output_spectrum:
                self.connect((self.impl, 2), (self, 2))

        def set_frequency(self, frequency):
            _retune(self, frequency)

        def set_smoothing(self, subarray, forward_backward=False):
            """Opt-in (not reference behaviour): FB averaging and/or smoothing over `subarray`-element subarrays;
            set_smoothing(m) switches it off.  Raises ValueError when the array response does not allow it."""
            _set_smoothing(self, subarray, forward_backward)

        def set_order_mode(self, criterion):
            """Opt-in (not reference behaviour): the number of emitters per item by "mdl" or "aic" (None: the fixed n)."""
            _set_order_mode(self, criterion)

        def set_refine_mode(self, parabolic=True):
            """Opt-in (not reference behaviour): angles between the grid's bins by a parabolic fit of the null (False: the
            reference's grid angles).  Best with the wrapped block's set_peak_mode(True)."""
            _set_refine_mode(self, parabolic)

        def set_power_mode(self, power_mode=1):
            """Opt-in (not reference behaviour): a Capon power estimate per reported entry, in the units of the covariance
            (1: behind last_powers(); 2: also on the lvl port; 0: off).  The constructor keeps the reference's signature."""
            _set_power_mode(self, power_mode)

        def set_estimator(self, kind):
            """Opt-in (not reference behaviour): the spectrum estimator, 0 / "music" (the reference), 1 / "capon" or
            2 / "bartlett": powers in the units of the covariance for every bin, no emitter count needed.  The constructor keeps
            the reference's signature."""
            _set_estimator(self, kind)

        def last_powers(self, count):
            """The float64 power estimates of the first `count` (item, slot) entries of the last work() call."""
            return numpy.asarray(self.impl.last_powers(int(count)), dtype=numpy.float64)

        def set_beam_mode(self, beam_mode=1, loading=0.0):
            """Opt-in (not reference behaviour): the MVDR beamformer output of every reported entry over the item's own snapshots,
            w = R^-1 a / (a^H R^-1 a) with `loading` times the mean diagonal added to R's diagonal (1: behind last_beams(); 0: off).
            Not available with set_smoothing.  The constructor keeps the reference's signature."""
            _set_beam_mode(self, beam_mode, loading)

        def last_beams(self, items):
            """The complex64 beams of the first `items` items of the last work() call, shape (items, n, K)."""
            return numpy.asarray(self.impl.last_beams(int(items)), dtype=numpy.complex64)

        def set_averaging(self, window, forgetting=1.0):
            """Opt-in (not reference behaviour): estimate every item from the covariances of the last `window` items, weighted
            forgetting ** age (window 1: off).  Raises ValueError unless 1 <= window <= 64 and 0 < forgetting <= 1."""
            _set_averaging(self, window, forgetting)

        def set_calibration(self, gamma):
            """Opt-in (not reference behaviour): per-antenna complex gains; the table in force becomes gamma_r * a_r(bin), also
            after set_frequency() (None: off).  Not available with set_smoothing."""
            _set_calibration(self, gamma)

        def calibration(self):
            """The complex64 gains in force, or None while off."""
            g = self.impl.calibration()
            return numpy.asarray(g, dtype=numpy.complex64) if len(g) else None

        def calibrate_next(self, items, pilot_bin=None, ref=None, min_quality=0.9):
            """Opt-in (not reference behaviour): estimate the gains from the next `items` items, which carry a pilot from the
            direction of bin `pilot_bin` of this helper's table (or with the ideal response `ref`; [1] * m: a noise source injected
            equally into all channels), and apply them when the estimate's quality (principal eigenvalue over trace) reaches
            `min_quality`.  last_calibration_quality(): -1 while waiting for the items."""
            _calibrate_next(self, items, pilot_bin, ref, min_quality)

        def last_calibration_quality(self):
            return float(self.impl.last_calibration_quality())

        def set_noise_covariance(self, rn):
            """Opt-in (not reference behaviour): noise pre-whitening with the m x m noise covariance `rn` (Hermitian positive
            definite), also after set_frequency() and set_calibration() (None: off).  Not available with set_smoothing, the beam
            mode or the Capon / Bartlett estimators."""
            _set_noise_covariance(self, rn)

        def noise_covariance(self):
            """The m x m complex128 noise covariance in force, or None while off."""
            return _noise_covariance(self)

        def set_beamspace(self, T, normalise=False):
            """Opt-in (not reference behaviour): beamspace MUSIC with the m x B matrix `T` (n < B <= min(m, 16); orthonormal
            columns), also after set_frequency() (None: off).  Opens every opt-in mode to 17 .. 64 antennas.  Not available with
            set_smoothing, a calibration, noise pre-whitening or the beam mode."""
            _set_beamspace(self, T, normalise)

        def set_beamspace_sector(self, bin_lo, bin_count, beams, normalise=False):
            """set_beamspace() with the T designed for the `bin_count` bins from `bin_lo` (wrapping) of the table in force;
            returns the captured fraction."""
            return _set_beamspace_sector(self, bin_lo, bin_count, beams, normalise)

        def beamspace(self):
            """The m x B complex128 matrix T in force, or None while off."""
            return _beamspace(self)

        def set_subbands(self, sample_rate, block, occupied=0.75, combine=None):
            """Opt-in (not reference behaviour): wideband MUSIC for a band that one array response does not fit -- items are cut into
            `block`-sample blocks, a DFT per antenna separates the subbands within `occupied` of the sampled band, each runs on the
            response at its own wavelength C / (frequency + offset sample_rate / block), and the spectra are combined ("harmonic",
            the default under MUSIC, or "arithmetic").  Stays in force across set_frequency().  set_subbands(None, 0): off."""
            _set_subbands(self, sample_rate, block, occupied, combine)

        def subbands(self):
            """(block, combine, bins) in force, or None while off."""
            v = list(self.impl.subbands())
            return (int(v[0]), int(v[1]), [int(k) for k in v[2:]]) if v else None

        def whiten_next(self, items):
            """Opt-in (not reference behaviour): measure the noise covariance from the next `items` items (a noise-only capture)
            and apply it.  last_whitening_status(): -1 while waiting for the items, 0 once applied, else the error code."""
            _whiten_next(self, items)

        def last_whitening_status(self):
            return int(self.impl.last_whitening_status())

else:

    class music_doa_helper(object):
        """GNU-Radio-less stand-in with the reference's constructor, attributes and set_frequency()."""

        def __init__(self, m, n, nsamples, angular_resolution, frequency, array_spacing, antenna_array,
                     output_spectrum=False):
            _configure(self, m, n, nsamples, angular_resolution, frequency, array_spacing, antenna_array)
            self.output_spectrum = bool(output_spectrum)
            # (itemsize, ...) of the ports the hier block would declare (:61-71)
            self.input_item_sizes = [8 * nsamples]
            self.output_item_sizes = [4 * n, 4 * n] + ([4 * angular_resolution] if output_spectrum else [])
            _banner(self)
            _make_impl(self)

        def set_frequency(self, frequency):
            _retune(self, frequency)

        def set_smoothing(self, subarray, forward_backward=False):
            """Opt-in (not reference behaviour): FB averaging and/or smoothing over `subarray`-element subarrays;
            set_smoothing(m) switches it off.  Raises ValueError when the array response does not allow it."""
            _set_smoothing(self, subarray, forward_backward)

        def set_order_mode(self, criterion):
            """Opt-in (not reference behaviour): the number of emitters per item by "mdl" or "aic" (None: the fixed n)."""
            _set_order_mode(self, criterion)

        def set_refine_mode(self, parabolic=True):
            """Opt-in (not reference behaviour): angles between the grid's bins by a parabolic fit of the null (False: the
            reference's grid angles).  Best with the wrapped block's set_peak_mode(True)."""
            _set_refine_mode(self, parabolic)

        def set_power_mode(self, power_mode=1):
            """Opt-in (not reference behaviour): a Capon power estimate per reported entry, in the units of the covariance
            (1: behind last_powers(); 2: also on the lvl port; 0: off).  The constructor keeps the reference's signature."""
            _set_power_mode(self, power_mode)

        def set_estimator(self, kind):
            """Opt-in (not reference behaviour): the spectrum estimator, 0 / "music" (the reference), 1 / "capon" or
            2 / "bartlett": powers in the units of the covariance for every bin, no emitter count needed.  The constructor keeps
            the reference's signature."""
            _set_estimator(self, kind)

        def last_powers(self, count):
            """The float64 power estimates of the first `count` (item, slot) entries of the last work() call."""
            return numpy.asarray(self.impl.last_powers(int(count)), dtype=numpy.float64)

        def set_beam_mode(self, beam_mode=1, loading=0.0):
            """Opt-in (not reference behaviour): the MVDR beamformer output of every reported entry over the item's own snapshots,
            w = R^-1 a / (a^H R^-1 a) with `loading` times the mean diagonal added to R's diagonal (1: behind last_beams(); 0: off).
            Not available with set_smoothing.  The constructor keeps the reference's signature."""
            _set_beam_mode(self, beam_mode, loading)

        def last_beams(self, items):
            """The complex64 beams of the first `items` items of the last work() call, shape (items, n, K)."""
            return numpy.asarray(self.impl.last_beams(int(items)), dtype=numpy.complex64)

        def set_averaging(self, window, forgetting=1.0):
            """Opt-in (not reference behaviour): estimate every item from the covariances of the last `window` items, weighted
            forgetting ** age (window 1: off).  Raises ValueError unless 1 <= window <= 64 and 0 < forgetting <= 1."""
            _set_averaging(self, window, forgetting)

        def set_calibration(self, gamma):
            """Opt-in (not reference behaviour): per-antenna complex gains; the table in force becomes gamma_r * a_r(bin), also
            after set_frequency() (None: off).  Not available with set_smoothing."""
            _set_calibration(self, gamma)

        def calibration(self):
            """The complex64 gains in force, or None while off."""
            g = self.impl.calibration()
            return numpy.asarray(g, dtype=numpy.complex64) if len(g) else None

        def calibrate_next(self, items, pilot_bin=None, ref=None, min_quality=0.9):
            """Opt-in (not reference behaviour): estimate the gains from the next `items` items, which carry a pilot from the
            direction of bin `pilot_bin` of this helper's table (or with the ideal response `ref`; [1] * m: a noise source injected
            equally into all channels), and apply them when the estimate's quality (principal eigenvalue over trace) reaches
            `min_quality`.  last_calibration_quality(): -1 while waiting for the items."""
            _calibrate_next(self, items, pilot_bin, ref, min_quality)

        def last_calibration_quality(self):
            return float(self.impl.last_calibration_quality())

        def set_noise_covariance(self, rn):
            """Opt-in (not reference behaviour): noise pre-whitening with the m x m noise covariance `rn` (Hermitian positive
            definite), also after set_frequency() and set_calibration() (None: off).  Not available with set_smoothing, the beam
            mode or the Capon / Bartlett estimators."""
            _set_noise_covariance(self, rn)

        def noise_covariance(self):
            """The m x m complex128 noise covariance in force, or None while off."""
            return _noise_covariance(self)

        def set_beamspace(self, T, normalise=False):
            """Opt-in (not reference behaviour): beamspace MUSIC with the m x B matrix `T` (n < B <= min(m, 16); orthonormal
            columns), also after set_frequency() (None: off).  Opens every opt-in mode to 17 .. 64 antennas.  Not available with
            set_smoothing, a calibration, noise pre-whitening or the beam mode."""
            _set_beamspace(self, T, normalise)

        def set_beamspace_sector(self, bin_lo, bin_count, beams, normalise=False):
            """set_beamspace() with the T designed for the `bin_count` bins from `bin_lo` (wrapping) of the table in force;
            returns the captured fraction."""
            return _set_beamspace_sector(self, bin_lo, bin_count, beams, normalise)

        def beamspace(self):
            """The m x B complex128 matrix T in force, or None while off."""
            return _beamspace(self)

        def set_subbands(self, sample_rate, block, occupied=0.75, combine=None):
            """Opt-in (not reference behaviour): wideband MUSIC for a band that one array response does not fit -- items are cut into
            `block`-sample blocks, a DFT per antenna separates the subbands within `occupied` of the sampled band, each runs on the
            response at its own wavelength C / (frequency + offset sample_rate / block), and the spectra are combined ("harmonic",
            the default under MUSIC, or "arithmetic").  Stays in force across set_frequency().  set_subbands(None, 0): off."""
            _set_subbands(self, sample_rate, block, occupied, combine)

        def subbands(self):
            """(block, combine, bins) in force, or None while off."""
            v = list(self.impl.subbands())
            return (int(v[0]), int(v[1]), [int(k) for k in v[2:]]) if v else None

        def whiten_next(self, items):
            """Opt-in (not reference behaviour): measure the noise covariance from the next `items` items (a noise-only capture)
            and apply it.  last_whitening_status(): -1 while waiting for the items, 0 once applied, else the error code."""
            _whiten_next(self, items)

        def last_whitening_status(self):
            return int(self.impl.last_whitening_status())

        def work(self, items):
            """Runs the wrapped block on (k, nsamples) complex64 items: returns (ang, lvl[, spectrum])."""
            produced, ang, lvl, spec = self.impl.work(numpy.ascontiguousarray(items, dtype=numpy.complex64),
                                                      3 if self.output_spectrum else 2)
            if produced != ang.shape[0]:
                raise RuntimeError("music_doa work() returned %d" % produced)
            return (ang, lvl, spec) if self.output_spectrum else (ang, lvl)
