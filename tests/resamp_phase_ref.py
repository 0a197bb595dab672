"""Pure-integer models of the fractional resampler's phase walk (gr_baz_amd/csrc/resamp_kernels.hip.h, baz_resamp_hip.hip).

Two models of the same walk, both on Python integers / `Fraction` only (no `long double`, no ctypes: they mean the same on any host):

X87Walk    the reference's recurrence (lib/baz_fractional_resampler_cc.cc: constructor, msg handler, setters, both branches of
           general_work).  Its `long double` members are x87 extended numbers: a 64-bit significand.  Every operation the
           reference performs on them -- the quotient num/denom, (i + frac)/1e9, d * d_mu_inc, s = d_mu + d_mu_inc, s += d_mu_adj,
           s - floor(s) -- is done exactly on Fractions and then rounded to 64 significant bits, to nearest, ties to even (`rn`).
           Conversions INTO long double (double, float, integers below 2^64) are exact.  (float)d_mu is one rounding to 24 bits,
           imu = rint((float)mu * 128) in float32 (the product is exact).  The exponent range is not modelled: every value that
           occurs lies between 2^-1074 and 2^63.
FixedWalk  the library's documented model: every quantity converted to 64.64 fixed point (truncated below 2^-64), output o read
           off the closed form P_0 = first, P_o = first + inc + adj + (o - 1) * inc in 128-bit integers, ii = floor(P_o),
           mu = rn_float(frac(P_o)) * 2^-64, the end-of-input rule of process_device_locked, and the `exact` flag as the library
           computes it.  `exact_conversion_only` is the flag rule of the library before its correction (conversions only), kept so
           that the tests can show what that rule missed.

The bound on the distance between the two
-----------------------------------------
Write T = (samples consumed so far) + mu for the total phase of a model (mu alone wraps; T does not; the two differences are the
same number whenever both models consumed the same count).  One step of the walk adds the increment in force:

  * FixedWalk adds inc_f = floor(inc * 2^64) / 2^64 exactly: d_inc = inc - inc_f lies in [0, 2^-64), and is 0 for every ratio that
    is a multiple of 2^-64 (every `double` ratio >= 2^-11).  The same holds for a phase (d_mu) and, with a sign, for an
    adjustment (d_adj = |adj_x87 - adj_f|: the library forms d * from_fixed(inc_f), rounds it to 64 bits, truncates it to 2^-64).
  * X87Walk adds inc exactly and then ROUNDS the sum to 64 significant bits.  A sum s >= 1 whose integer part has k bits keeps
    64 - k fraction bits, so the rounding moves it by at most half a unit of the last kept fraction bit, 2^(k-65); a sum below 1
    keeps every bit down to 2^-64 at least (at most 2^-65).  s - floor(s) is exact for s >= 0.

So after o steps, with the step's own quantities in force,

    |T_x87 - T_fixed|  <=  d_mu + sum over the o steps of [ d_inc + 2^(k-65)  (+ d_adj + 2^(k'-65) on a step with an adjustment) ]

where k = bit length of floor(inc) + 1 bounds the integer bits of mu + inc (mu < 1) and k' = bit length of
floor(inc) + 2 + floor(|adj|) those of the sum with the adjustment; on the first step of a call with a pending set_mu the new mu
(which may be >= 1) enters both.  A set_mu replaces the accumulated difference by its own d_mu.  `PhaseBound` accumulates exactly
this, a priori, from the parameters alone.

When the roundings stop.  A sum with k integer bits leaves mu on the grid 2^(k-64).  If the increment lies on that grid too, every
later sum with at most k integer bits is exact: the grid of mu only coarsens.  A constant `double` ratio >= 2^-11 lies on the grid
of every sum it can produce (53 significant bits against 64 - k with k <= exponent + 2), and mu + inc takes at most two integer
bit counts (floor(inc) and floor(inc) + 1), so AT MOST TWO sums of the whole stream round, and for such a stream

    |T_x87 - T_fixed|  <=  d_mu + 2^(k-64)       for every o   (`constant_double_bound`),

a constant offset: e.g. phase 0.001 (last bit 2^-60) with ratio 17.3 (k = 5: 59 fraction bits kept) is off by 2^-60 from output 1
on, for ever.  A quotient ratio (num/denom, the ppb pair) has 64 significant bits of its own: it is off the kept grid of most sums,
every sum may round, and the difference grows like o * (d_inc + 2^(k-65)).

The `exact` flag follows from the same reasoning: if, at a call, the phase in force, the increment and the adjustment are all
multiples of 2^(k-64), k the largest integer bit count a sum of this call can reach, then every sum of the call is exact and the two
walks are the same walk.  The rule is conservative: it takes k from the largest sum the call could form (first + inc, that plus
adj, or (1 - 2^-64) + inc) and judges by the lowest set bit of each quantity, so it may say 0 where no sum happened to round; and
it says 0 for every ratio that is not a `double` value (a quotient rounded to 64 bits, the ppb pair): the low bits of such a ratio
are rounding noise, and whether they happen to be zeros is not something to build on.

Phase exactly 1.0 (allowed by the constructor): the reference reads tap row 128 at ii, the closed form reads row 0 at ii + 1.  The
two are the same filter for every table whose row 128 is row 0 shifted by one sample (the MMSE table: both are pure delays).
`canonical` maps (ii, 128) to (ii + 1, 0) for comparisons that hold under that condition.
"""
from fractions import Fraction

import numpy as np

NTAPS, NSTEPS = 8, 128
ONE64 = 1 << 64
MASK64 = ONE64 - 1
RATIO_MIN = Fraction(1, 2048)
RATIO_MAX = Fraction(1 << 31)


class Invalid(ValueError):
    """BAZ_RESAMP_E_INVALID / the reference's std::out_of_range."""


class Unsupported(ValueError):
    """BAZ_RESAMP_E_UNSUPPORTED: a ratio outside [2^-11, 2^31]."""


def rn(x, bits=64):
    """x (Fraction or int) rounded to `bits` significant bits, to nearest, ties to even; exact Fraction."""
    x = Fraction(x)
    if x == 0:
        return x
    neg = x < 0
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()            # 2^(e-1) < n/d < 2^(e+1)
    if (n << max(0, -e)) < (d << max(0, e)):       # n/d < 2^e
        e -= 1                                     # now 2^e <= n/d < 2^(e+1)
    sh = bits - 1 - e                              # n/d * 2^sh lies in [2^(bits-1), 2^bits)
    if sh >= 0:
        q, r = divmod(n << sh, d)
    else:
        q, r = divmod(n, d << -sh)
        d <<= -sh
    if 2 * r > d or (2 * r == d and (q & 1)):
        q += 1
    v = Fraction(q << -sh, 1) if sh < 0 else Fraction(q, 1 << sh)
    return -v if neg else v


def floor_(x):
    return x.numerator // x.denominator


def imu_of(mu):
    """rint((float)mu * 128) in float32 for an exact mu in [0, 1]: one rounding to 24 bits, an exact product, ties to even."""
    return int(round(rn(mu, 24) * NSTEPS))         # round(Fraction) rounds halves to even


def canonical(ii, imu):
    """(ii, 128) -> (ii + 1, 0): the same filter for tables whose row 128 is row 0 shifted by one sample."""
    ii = np.asarray(ii, dtype=np.int64).copy()
    imu = np.asarray(imu, dtype=np.int64).copy()
    top = imu == NSTEPS
    ii[top] += 1
    imu[top] = 0
    return ii, imu


def check_ratio(r):
    if not r > 0:
        raise Invalid("resampling ratio must be > 0")
    if not (RATIO_MIN <= r <= RATIO_MAX):
        raise Unsupported("ratio outside [2^-11, 2^31]")


def interp_f32(x, ii, imu, table):
    """out[o] = sum_k x[ii_o + k] * table[imu_o][7 - k], float32 multiply then float32 add, k ascending (the interpolator's
    loop, no fma), vectorised over the outputs.  x complex64 (L,), -> complex64 (len(ii),)."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    ii = np.asarray(ii, dtype=np.int64)
    imu = np.asarray(imu, dtype=np.int64)
    t = np.asarray(table, dtype=np.float32)
    re = np.zeros(ii.shape[0], np.float32)
    im = np.zeros(ii.shape[0], np.float32)
    for k in range(NTAPS):
        w = t[imu, NTAPS - 1 - k]
        re = (re + xr[ii + k] * w).astype(np.float32)
        im = (im + xi[ii + k] * w).astype(np.float32)
    out = np.empty(ii.shape[0], np.complex64)
    out.real, out.imag = re, im
    return out


# ------------------------------------------------------------------------------------------------ the reference's walk
class X87Walk:
    """State and methods named after the reference block; all values exact Fractions with 64-bit significands."""

    def __init__(self, phase_shift, ratio, num=0, denom=0):
        r = Fraction(ratio) if denom == 0 else rn(Fraction(int(num), int(denom)))          # (long double)num / (long double)denom
        if not r > 0 or not (0 <= phase_shift <= 1):
            raise Invalid("resampling ratio must be > 0 and phase shift in [0, 1]")
        check_ratio(r)
        self.d_mu = Fraction(phase_shift)
        self.d_mu_inc = r
        self.d_update = self.d_update_mu = self.d_update_mu_adj = False
        self.d_mu_inc_update = self.d_mu_update = self.d_mu_adj = Fraction(0)
        self.sums_rounded = 0                      # how many sums of the walk were not exact (diagnostic)

    def set_mu(self, mu):
        self.d_mu_update, self.d_update_mu = Fraction(mu), True

    def _set_ratio(self, r):
        check_ratio(r)
        self.d_mu_inc_update, self.d_update = r, True

    def set_resamp_ratio(self, r):
        self._set_ratio(Fraction(r))

    def set_resamp_ratio_rational(self, num, denom):
        if denom != 0:
            self._set_ratio(rn(Fraction(int(num), int(denom))))

    def set_resamp_ratio_ppb(self, whole, frac):
        self._set_ratio(rn(rn(Fraction(int(whole)) + Fraction(frac)) / Fraction(10 ** 9)))   # ((long double)i + frac) / 1e9

    def adjust(self, d):
        self.d_mu_adj, self.d_update_mu_adj = rn(Fraction(d) * self.d_mu_inc), True           # (long double)d * d_mu_inc

    def mu(self):
        return float(rn(self.d_mu, 53))

    def resamp_ratio(self):
        return float(rn(self.d_mu_inc, 53))

    def _step(self, s_exact):
        s = rn(s_exact)
        self.sums_rounded += s != s_exact
        return s

    def work(self, noutput, rr=None):
        """One general_work(): -> (ii int64[noutput], imu int64[noutput], consumed).  rr: the second input (float32 ratio per
        input sample) selects the two-input branch, which ignores the pending setters like the reference does."""
        ii = 0
        iis, imus = np.zeros(noutput, np.int64), np.zeros(noutput, np.int64)
        for oo in range(noutput):
            if rr is None and self.d_update_mu:
                self.d_mu, self.d_update_mu = self.d_mu_update, False
            iis[oo], imus[oo] = ii, imu_of(self.d_mu)
            if rr is None:
                if self.d_update:
                    self.d_mu_inc, self.d_update = self.d_mu_inc_update, False
                s = self._step(self.d_mu + self.d_mu_inc)
                if self.d_update_mu_adj:
                    s = self._step(s + self.d_mu_adj)
                    self.d_update_mu_adj = False
            else:
                self.d_mu_inc = Fraction(float(rr[ii]))
                s = self._step(self.d_mu + self.d_mu_inc)
            f = floor_(s)
            self.d_mu = rn(s - f)                  # exact for s >= 0
            ii += f
            if ii < 0:
                raise Invalid("the walk steps before in[0]")
        return iis, imus, ii


# ------------------------------------------------------------------------------------------------ the library's walk
def to_fixed(v):
    """Non-negative 64-bit-significand value -> (64.64 integer, exact?): truncation below 2^-64."""
    p = v * ONE64
    f = floor_(p)
    return f, f == p


def to_fixed_signed(v):
    f, ex = to_fixed(abs(v))
    return (-f if v < 0 else f), ex


def from_fixed(f):
    """(long double)hi + (long double)lo / 2^64: one rounding to 64 bits."""
    return rn(Fraction(f, ONE64))


def _ctz(v):
    v = abs(v)
    return 1 << 30 if v == 0 else (v & -v).bit_length() - 1


def sums_stay_exact(first, inc, adj):
    """The library's rule for one call (64.64 integers): first, inc and adj all multiples of 2^(k-64), k the integer bit count
    of the largest sum the call can form -- first + inc, that plus adj, or (1 - 2^-64) + inc on a later step."""
    top = max(first + inc, first + inc + adj, MASK64 + inc) >> 64
    return min(_ctz(first), _ctz(inc), _ctz(adj)) >= top.bit_length()


def is_double(r):
    return rn(r, 53) == r


class FixedWalk:
    def __init__(self, phase_shift, ratio, num=0, denom=0):
        r = Fraction(ratio) if denom == 0 else rn(Fraction(int(num), int(denom)))
        if not r > 0 or not (0 <= phase_shift <= 1):
            raise Invalid("ratio <= 0 or phase shift outside [0, 1]")
        check_ratio(r)
        self.exact_conversion_only = True
        self.mu_fx = self._conv(Fraction(phase_shift))
        self.inc_fx = self._conv(r)
        self.update = self.update_mu = self.update_mu_adj = False
        self.inc_update = self.mu_update = self.adj_fx = 0
        self.exact = self.exact_conversion_only and is_double(r) and sums_stay_exact(self.mu_fx, self.inc_fx, 0)

    def _conv(self, v, signed=False):
        f, ex = to_fixed_signed(v) if signed else to_fixed(v)
        if not ex:
            self.exact = self.exact_conversion_only = False
        return f

    def set_mu(self, mu):
        if not mu >= 0:
            raise Invalid("mu < 0")
        self.mu_update, self.update_mu = self._conv(Fraction(mu)), True

    def _set_ratio(self, r):
        check_ratio(r)
        if not is_double(r):                       # a rounded quotient: 64 significant bits, off the grid of its own sums
            self.exact = False
        self.inc_update, self.update = self._conv(r), True

    def set_resamp_ratio(self, r):
        self._set_ratio(Fraction(r))

    def set_resamp_ratio_rational(self, num, denom):
        if denom != 0:
            self._set_ratio(rn(Fraction(int(num), int(denom))))

    def set_resamp_ratio_ppb(self, whole, frac):
        self._set_ratio(rn(rn(Fraction(int(whole)) + Fraction(frac)) / Fraction(10 ** 9)))

    def adjust(self, d):
        self.adj_fx, self.update_mu_adj = self._conv(rn(Fraction(d) * from_fixed(self.inc_fx)), signed=True), True

    @property
    def mu_exact(self):
        return Fraction(self.mu_fx, ONE64)

    def mu(self):
        return float(rn(from_fixed(self.mu_fx), 53))

    def resamp_ratio(self):
        return float(rn(from_fixed(self.inc_fx), 53))

    def work(self, ninput, noutput):
        """process_device_locked(): -> (ii int64[n], imu int64[n], consumed), n <= noutput what `ninput` samples allow."""
        empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
        if noutput == 0:
            return empty
        first = self.mu_update if self.update_mu else self.mu_fx
        inc = self.inc_update if self.update else self.inc_fx
        adj = self.adj_fx if self.update_mu_adj else 0
        step1 = first + inc + adj
        if step1 < 0:
            raise Invalid("the walk steps before in[0]")
        if ninput < NTAPS:
            return empty
        limit = (ninput - (NTAPS - 1)) << 64
        if first >= limit:
            return empty
        n = 1
        if noutput > 1 and step1 < limit:
            k = (limit - 1 - step1) // inc
            n = noutput if k >= noutput - 2 else k + 2
        pend = step1 + (n - 1) * inc
        if (pend >> 64) > 0xFFFFFFFF * 2048:
            raise Invalid("input index out of range")
        if not sums_stay_exact(first, inc, adj):
            self.exact = False
        iis, imus = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for o in range(n):
            p = first if o == 0 else step1 + (o - 1) * inc
            iis[o] = p >> 64
            imus[o] = imu_of(Fraction(p & MASK64, ONE64))
        self.update = self.update_mu = self.update_mu_adj = False
        self.inc_fx = inc
        self.mu_fx = pend & MASK64
        return iis, imus, pend >> 64


# ------------------------------------------------------------------------------------------------ the a-priori bound
def _half_unit(int_bound):
    """Half a unit of the last fraction bit an x87 sum keeps when its integer part is at most `int_bound`."""
    return Fraction(1, 1 << (65 - int(int_bound).bit_length()))


class PhaseBound:
    """Accumulates the bound of the module docstring for a pair of walks driven through the same events.  Call `call(n)` BEFORE
    both walks work on a call of n outputs (it reads their pending state); `value` then bounds |T_x87 - T_fixed| after it."""

    def __init__(self, x87, fixed):
        self.a, self.b = x87, fixed
        self.value = abs(x87.d_mu - fixed.mu_exact)

    def call(self, n):
        a, b = self.a, self.b
        if n == 0:
            return self.value
        mu_hi = floor_(a.d_mu)                      # 1 only for a constructor phase of exactly 1.0
        if a.d_update_mu:
            self.value = abs(a.d_mu_update - Fraction(b.mu_update, ONE64))
            mu_hi = floor_(a.d_mu_update)
        inc = a.d_mu_inc_update if a.d_update else a.d_mu_inc
        inc_f = Fraction(b.inc_update if b.update else b.inc_fx, ONE64)
        d_inc = abs(inc - inc_f)
        hi = floor_(inc)
        self.value += d_inc + _half_unit(mu_hi + hi + 1)
        if a.d_update_mu_adj:
            self.value += abs(a.d_mu_adj - Fraction(b.adj_fx, ONE64)) + _half_unit(mu_hi + hi + 2 + floor_(abs(a.d_mu_adj)))
        self.value += (n - 1) * (d_inc + _half_unit(hi + 1))
        return self.value


def constant_double_bound(phase, ratio):
    """|T_x87 - T_fixed| for a stream with a constant double ratio >= 2^-11 and no events, for every output count."""
    d_mu = Fraction(phase) - Fraction(to_fixed(Fraction(phase))[0], ONE64)
    return d_mu + 2 * _half_unit(floor_(Fraction(ratio)) + 1)
