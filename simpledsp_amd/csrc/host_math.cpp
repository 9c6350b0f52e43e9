// host_math.cpp -- the cold, host-side part of the path: size helpers, the run-time twiddle
// precompute that replaces the reference's compile-time tables, Butterworth section design and
// filter preload.  Double precision, runs once per plan / per filter.
#include "sdsp_hip_internal.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

namespace sdsp_hip
{
thread_local std::string g_last_error;

int fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

// W_n^j = cos(2 pi j / n) - i * sgn * sin(2 pi j / n), sgn = +1 forward, -1 reverse.
// Same construction idea as the reference's calc_trigs (fft.h:148-194): only the first quadrant
// is evaluated with libm, the other three are exact mirror images, so cos(90 deg) is exactly 0
// and conjugate-symmetric entries are bit-identical.  (The reference does this at compile time
// for every stage row; one row of n entries is all the GPU kernels need: row i of the
// reference table is this row sampled with stride n / 2^(i+1).)
void make_twiddles(uint32_t n, int direction, std::vector<double> &out)
{
    out.assign(2 * (size_t)n, 0.0);
    const double sgn = direction == SDSP_HIP_REVERSE ? -1.0 : 1.0;
    if (n == 1) {
        out[0] = 1.0;
        return;
    }
    if (n == 2) {
        out[0] = 1.0;
        out[2] = -1.0;
        return;
    }
    const uint32_t quarter = n / 4;
    std::vector<double> cq(quarter + 1), sq(quarter + 1);
    cq[0] = 1.0;
    sq[0] = 0.0;
    cq[quarter] = 0.0;
    sq[quarter] = 1.0;
    for (uint32_t j = 1; j < quarter; j++) {
        // same argument recipe as fft.h:169 (double), then long-double libm so that the value
        // rounded to double is the correctly rounded one GCC's constant folder produces
        const double rad = 2 * M_PI * j / n;
        cq[j] = (double)cosl((long double)rad);
        sq[j] = (double)sinl((long double)rad);
    }
    for (uint32_t m = 0; m < n; m++) {
        const uint32_t q = m / quarter, r = m % quarter;
        double c, s;
        switch (q) {
        case 0: c = cq[r]; s = sq[r]; break;
        case 1: c = -cq[quarter - r]; s = sq[quarter - r]; break;
        case 2: c = -cq[r]; s = -sq[r]; break;
        default: c = cq[quarter - r]; s = -sq[quarter - r]; break;
        }
        out[2 * (size_t)m] = c;
        out[2 * (size_t)m + 1] = -sgn * s;
    }
}

// The same row correctly rounded: make_twiddles forms the angle 2 pi j / n in double as the reference does, which leaves entries up
// to 1.85 units of 2^-53 from W_n^j (the angle's own rounding, worst near pi / 2).  Here the angle is reduced to the first octant in
// integers, formed and evaluated in long double and rounded once; the other octants are exact mirror images.  The double-precision
// kernels' own tables (thread twiddles, W_2N, the sub-transforms' rows) are built from this row; the row a plan reports
// (sdsp_hip_fft_plan_get_twiddles) stays the reference's.
void make_twiddles_rounded(uint32_t n, int direction, std::vector<double> &out)
{
    if (n < 4) {
        make_twiddles(n, direction, out);
        return;
    }
    out.assign(2 * (size_t)n, 0.0);
    const double sgn = direction == SDSP_HIP_REVERSE ? -1.0 : 1.0;
    const long double step = 3.14159265358979323846264338327950288L / (2.0L * (long double)n); // pi / 2 in units of 1 / n
    for (uint32_t m = 0; m < n; m++) {
        const uint64_t four = 4ull * m;
        const uint32_t quad = (uint32_t)(four / n);
        uint64_t rem = four % n; // angle = (quad + rem / n) pi / 2
        const bool swap = 2 * rem > n;
        if (swap)
            rem = n - rem;
        const long double th = (long double)rem * step;
        double c = (double)cosl(th), s = (double)sinl(th);
        if (swap)
            std::swap(c, s);
        double re, im; // exp(-i (quad pi / 2 + th)) = (-i)^quad (c - i s)
        switch (quad) {
        case 0: re = c; im = -s; break;
        case 1: re = -s; im = -c; break;
        case 2: re = -c; im = s; break;
        default: re = s; im = c; break;
        }
        out[2 * (size_t)m] = re + 0.0; // no negative zeros
        out[2 * (size_t)m + 1] = sgn * im + 0.0;
    }
}

// set_lp_coeff / set_hp_coeff: casc_2o_iir.h:168-194 and :140-166.  Expression order kept so
// the coefficients equal the reference's doubles.
static int design_lp_hp(uint32_t m, double f0, double fs, double gain_in, bool high, double *a,
                        double *b, double *gain)
{
    if (m == 0 || m % 2 != 0 || m > SDSP_HIP_MAX_SECTIONS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "M must be even! (and <= SDSP_HIP_MAX_SECTIONS)");
    if (!a || !b || !gain)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    double g = gain_in;
    const double e0 = 2 * M_PI * f0 / fs;
    for (uint32_t k = 0; k < m; k++) {
        const double dk = 2 * std::sin((2 * k + 1) * M_PI / (4.0 * m));
        const double t = dk * std::sin(e0) / 2;
        const double beta = (1 - t) / (1 + t) / 2;
        const double gamma = (0.5 + beta) * std::cos(e0);
        const double alpha = high ? (0.5 + beta + gamma) / 4 : (0.5 + beta - gamma) / 4;
        g *= 2 * alpha;
        b[3 * k + 0] = 1.0;
        b[3 * k + 1] = high ? -2.0 : 2.0;
        b[3 * k + 2] = 1.0;
        a[3 * k + 0] = 1.0;
        a[3 * k + 1] = -2 * gamma;
        a[3 * k + 2] = 2 * beta;
    }
    *gain = g;
    return SDSP_HIP_OK;
}

int design_lp(uint32_t m, double f0, double fs, double gain_in, double *a, double *b, double *gain)
{
    return design_lp_hp(m, f0, fs, gain_in, false, a, b, gain);
}

int design_hp(uint32_t m, double f0, double fs, double gain_in, double *a, double *b, double *gain)
{
    return design_lp_hp(m, f0, fs, gain_in, true, a, b, gain);
}

// set_bp_coeff: casc_2o_iir.h:82-138 -- m/2 pole pairs, two sections each, numerator [1,0,-1]
int design_bp(uint32_t m, double f0, double fs, double q, double gain_in, double *a, double *b,
              double *gain)
{
    if (m == 0 || m % 2 != 0 || m > SDSP_HIP_MAX_SECTIONS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "M must be even! (and <= SDSP_HIP_MAX_SECTIONS)");
    if (!a || !b || !gain)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    double g = gain_in;
    const double e0 = 2 * M_PI * f0 / fs;
    const double de = 2 * std::tan(e0 / (2 * q)) / std::sin(e0);
    for (uint32_t k = 0; k < m / 2; k++) {
        const double d = 2 * std::sin((2 * k + 1) * M_PI / (2.0 * m));
        const double aa = (1 + de * de / 4.0) * 2 / d / de;
        const double dk = std::sqrt(de * d / (aa + std::sqrt(aa * aa - 1)));
        const double bb = d * de / dk / 2.0;
        const double w = bb + std::sqrt(bb * bb - 1);
        const double th = std::tan(e0 / 2.0);
        const double e[2] = { 2.0 * std::atan(th / w), 2.0 * std::atan(w * th) };
        const double sc = std::sqrt(1 + (w - 1 / w) / dk * (w - 1 / w) / dk);
        double alpha[2];
        for (int h = 0; h < 2; h++) {
            const double t = dk * std::sin(e[h]) / 2.0;
            const double beta = (1 - t) / (1 + t) / 2.0;
            const double gamma = (0.5 + beta) * std::cos(e[h]);
            alpha[h] = (0.5 - beta) * sc / 2.0;
            const uint32_t s = 2 * k + h;
            b[3 * s + 0] = 1.0;
            b[3 * s + 1] = 0.0;
            b[3 * s + 2] = -1.0;
            a[3 * s + 0] = 1.0;
            a[3 * s + 1] = -2 * gamma;
            a[3 * s + 2] = 2 * beta;
        }
        g *= 4 * alpha[0] * alpha[1];
    }
    *gain = g;
    return SDSP_HIP_OK;
}

// Band-stop design -- the reference's README lists it as TODO (README.md:15); no reference code exists,
// so this is a new design in the same parameterisation as set_bp_coeff (centre f0, quality q ->
// -3 dB width f0/q, Butterworth prototype of order m): the band-stop frequency transformation
// s = tan(e0/2q) (z^2 - 1) / (z^2 - 2 cos(e0) z + 1) applied to each prototype pole p gives the
// quadratic (p - B) z^2 - 2 p c z + (p + B) = 0; its two roots (and their conjugates, from p*) are
// the poles of two sections.  Every section has the zero pair e^{+-j e0} (numerator [1, -2c, 1]);
// the gain normalises each section to 1 at DC.  Checked against scipy.signal.butter(btype='bandstop').
int design_bs(uint32_t m, double f0, double fs, double q, double gain_in, double *a, double *b,
              double *gain)
{
    if (m == 0 || m % 2 != 0 || m > SDSP_HIP_MAX_SECTIONS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "M must be even! (and <= SDSP_HIP_MAX_SECTIONS)");
    if (!a || !b || !gain)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    using cplx = std::complex<double>;
    double g = gain_in;
    const double e0 = 2 * M_PI * f0 / fs;
    const double c = std::cos(e0);
    const double bw = std::tan(e0 / (2 * q));
    for (uint32_t k = 0; k < m / 2; k++) {
        const double th = (2 * k + 1) * M_PI / (2.0 * m);
        const cplx p(-std::sin(th), std::cos(th));
        const cplx qa = p - bw, qb = -2.0 * p * c, qc = p + bw;
        const cplx disc = std::sqrt(qb * qb - 4.0 * qa * qc);
        const cplx z[2] = { (-qb + disc) / (2.0 * qa), (-qb - disc) / (2.0 * qa) };
        for (int h = 0; h < 2; h++) {
            const uint32_t s = 2 * k + h;
            a[3 * s + 0] = 1.0;
            a[3 * s + 1] = -2 * z[h].real();
            a[3 * s + 2] = std::norm(z[h]);
            b[3 * s + 0] = 1.0;
            b[3 * s + 1] = -2 * c;
            b[3 * s + 2] = 1.0;
            g *= (1 + a[3 * s + 1] + a[3 * s + 2]) / (2 - 2 * c);
        }
    }
    *gain = g;
    return SDSP_HIP_OK;
}

// firwin's construction, shared by design_fir and the filter-bank prototype: the ideal responses of the pass bands (left, right
// edges as fractions of Nyquist) times the SYMMETRIC window of `taps` points, scaled to `gain` at DC / Nyquist / the first band's centre
static void windowed_sinc(uint64_t taps, const double (*bands)[2], int nb, int window_kind, double gain, double *h)
{
    auto sinc = [](double x) { return x == 0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x); };
    const double alpha = 0.5 * (taps - 1);
    for (uint64_t i = 0; i < taps; i++) {
        const double m = i - alpha;
        double v = 0;
        for (int bnd = 0; bnd < nb; bnd++)
            v += bands[bnd][1] * sinc(bands[bnd][1] * m) - bands[bnd][0] * sinc(bands[bnd][0] * m);
        double w = 1.0;
        if (taps > 1) {
            const double c1 = std::cos(2 * M_PI * i / (taps - 1));
            switch (window_kind) {
            case SDSP_HIP_WINDOW_RECT: w = 1.0; break;
            case SDSP_HIP_WINDOW_HANN: w = 0.5 - 0.5 * c1; break;
            case SDSP_HIP_WINDOW_HAMMING: w = 0.54 - 0.46 * c1; break;
            default: w = 0.42 - 0.5 * c1 + 0.08 * std::cos(4 * M_PI * i / (taps - 1)); break;
            }
        }
        h[i] = v * w;
    }
    const double left = bands[0][0], right = bands[0][1];
    const double scale_frequency = left == 0 ? 0.0 : (right == 1 ? 1.0 : 0.5 * (left + right));
    double s = 0;
    for (uint64_t i = 0; i < taps; i++)
        s += h[i] * std::cos(M_PI * (i - alpha) * scale_frequency);
    for (uint64_t i = 0; i < taps; i++)
        h[i] = h[i] / s * gain;
}

// FIR design -- the reference's README.md:16 TODO; no reference code.  Windowed-sinc (Hamming) design,
// the same construction as scipy.signal.firwin (which the tests pin it to): ideal band responses
// sum(right sinc(right m) - left sinc(left m)) over the pass bands, times the symmetric Hamming window,
// scaled to unit gain at DC / Nyquist / the band centre.  lp, hp take the cutoff f0; bp, bs take
// centre f0 and q with edges f0 -+ f0/(2q) (width f0/q as in set_bp_coeff, without frequency warping).
int design_fir(uint32_t taps, int filter_type, double f0, double fs, double q, double gain_in, double *h)
{
    if (taps == 0 || taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_MAX_TAPS]");
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    const double nyq = fs / 2;
    double lo = 0, hi = 0; // the band that defines the filter, as fractions of Nyquist
    bool pass_zero = false;
    switch (filter_type) {
    case SDSP_HIP_FILTER_LOW_PASS: lo = 0; hi = f0 / nyq; pass_zero = true; break;
    case SDSP_HIP_FILTER_HIGH_PASS: lo = f0 / nyq; hi = 1; pass_zero = false; break;
    case SDSP_HIP_FILTER_BAND_PASS: lo = (f0 - f0 / (2 * q)) / nyq; hi = (f0 + f0 / (2 * q)) / nyq; pass_zero = false; break;
    case SDSP_HIP_FILTER_BAND_STOP: lo = (f0 - f0 / (2 * q)) / nyq; hi = (f0 + f0 / (2 * q)) / nyq; pass_zero = true; break;
    default: return fail(SDSP_HIP_ERR_INVALID_ARG, "filter_type must be low_pass, high_pass, band_pass or band_stop");
    }
    const bool band = filter_type == SDSP_HIP_FILTER_BAND_PASS || filter_type == SDSP_HIP_FILTER_BAND_STOP;
    if (!(fs > 0) || !(band ? (lo > 0 && hi < 1 && lo < hi) : (f0 > 0 && f0 < nyq)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "cutoff frequencies must lie strictly between 0 and fs/2");
    const bool pass_nyquist = filter_type == SDSP_HIP_FILTER_HIGH_PASS || filter_type == SDSP_HIP_FILTER_BAND_STOP;
    if (pass_nyquist && taps % 2 == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "a filter that passes fs/2 needs an odd number of taps");
    // pass bands as (left, right) pairs
    double bands[2][2];
    int nb = 0;
    if (filter_type == SDSP_HIP_FILTER_LOW_PASS) { bands[nb][0] = 0; bands[nb++][1] = hi; }
    else if (filter_type == SDSP_HIP_FILTER_HIGH_PASS) { bands[nb][0] = lo; bands[nb++][1] = 1; }
    else if (filter_type == SDSP_HIP_FILTER_BAND_PASS) { bands[nb][0] = lo; bands[nb++][1] = hi; }
    else { bands[nb][0] = 0; bands[nb++][1] = lo; bands[nb][0] = hi; bands[nb++][1] = 1; }
    (void)pass_zero;
    windowed_sinc(taps, bands, nb, SDSP_HIP_WINDOW_HAMMING, gain_in, h);
    return SDSP_HIP_OK;
}

// the polyphase filter bank's prototype: the same construction with one pass band [0, cutoff] and any of the four windows
int windowed_sinc_lowpass(uint64_t taps, double cutoff, int window_kind, double *h)
{
    const double bands[1][2] = { { 0.0, cutoff } };
    windowed_sinc(taps, bands, 1, window_kind, 1.0, h);
    return SDSP_HIP_OK;
}

// preload_filter: casc_2o_iir.h:197-214.  DC propagates section to section only for low_pass
// (and band_stop, which also passes DC; not in the reference).
int preload(uint32_t m, int filter_type, const double *a, const double *b, double gain,
            double value, double *mem)
{
    if (m == 0 || m % 2 != 0 || m > SDSP_HIP_MAX_SECTIONS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "M must be even! (and <= SDSP_HIP_MAX_SECTIONS)");
    if (!mem || ((filter_type == SDSP_HIP_FILTER_LOW_PASS || filter_type == SDSP_HIP_FILTER_BAND_STOP) && (!a || !b)))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null pointer");
    double v = value * gain;
    std::memset(mem, 0, sizeof(double) * 3 * (m + 1));
    for (int i = 0; i < 3; i++)
        mem[i] = v;
    if (filter_type == SDSP_HIP_FILTER_LOW_PASS || filter_type == SDSP_HIP_FILTER_BAND_STOP) {
        for (uint32_t j = 1; j < m + 1; j++) {
            v /= 1 + a[3 * (j - 1) + 1] + a[3 * (j - 1) + 2];
            v *= b[3 * (j - 1) + 0] + b[3 * (j - 1) + 1] + b[3 * (j - 1) + 2];
            for (int i = 0; i < 3; i++)
                mem[3 * j + i] = v;
        }
    }
    return SDSP_HIP_OK;
}
// forward-backward filtering: the steady state of a cascade per unit input and scipy's default edge
namespace
{
int check_cascade(uint32_t m, int kind, const double *a, const double *b)
{
    if (m == 0 || m % 2 != 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "M must be even!");
    if (m > SDSP_HIP_MAX_SECTIONS)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "at most SDSP_HIP_MAX_SECTIONS (16) sections are compiled in");
    if (kind < SDSP_HIP_IIR_GENERIC || kind > SDSP_HIP_IIR_BP)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "unknown IIR kind");
    if (!a || (kind == SDSP_HIP_IIR_GENERIC && !b))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "coefficient pointer is null");
    return SDSP_HIP_OK;
}

// b1 / b2 of section j as the kind's process body uses them: the folded numerators 1+2+1, 1-2+1, 1+0-1
void numerator(int kind, const double *b, uint32_t j, double *b1, double *b2)
{
    switch (kind) {
    case SDSP_HIP_IIR_LP: *b1 = 2.0, *b2 = 1.0; break;
    case SDSP_HIP_IIR_HP: *b1 = -2.0, *b2 = 1.0; break;
    case SDSP_HIP_IIR_BP: *b1 = 0.0, *b2 = -1.0; break;
    default: *b1 = b[3 * j + 1], *b2 = b[3 * j + 2]; break;
    }
}
} // namespace

int iir_steady_state(uint32_t m, int kind, const double *a, const double *b, double gain, double *s)
{
    if (int rc = check_cascade(m, kind, a, b))
        return rc;
    if (!s)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    for (uint32_t j = 0; j < m; j++)
        if (1.0 + a[3 * j + 1] + a[3 * j + 2] == 0.0)
            return fail(SDSP_HIP_ERR_INVALID_ARG, "a section has 1 + a1 + a2 == 0 (a pole at z = 1): it has no steady state");
    s[0] = gain;
    for (uint32_t j = 0; j < m; j++) {
        double b1, b2;
        numerator(kind, b, j, &b1, &b2);
        s[j + 1] = s[j] * (1.0 + b1 + b2) / (1.0 + a[3 * j + 1] + a[3 * j + 2]);
    }
    return SDSP_HIP_OK;
}

int filtfilt_default_padlen(uint32_t m, int kind, const double *a, const double *b, uint32_t *padlen)
{
    if (int rc = check_cascade(m, kind, a, b))
        return rc;
    if (!padlen)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    uint32_t zb = 0, za = 0;
    for (uint32_t j = 0; j < m; j++) {
        double b1, b2;
        numerator(kind, b, j, &b1, &b2);
        zb += b2 == 0.0;
        za += a[3 * j + 2] == 0.0;
    }
    *padlen = 3 * (2 * m + 1 - std::min(zb, za));
    return SDSP_HIP_OK;
}

// inverse STFT synthesis window: env[r] = sum over ascending k of w[r + k hop]^2, in double
int istft_synthesis(uint32_t n, uint32_t hop, const double *w, int norm, double *g, double *env_min, double *env_max)
{
    if (!sdsp_hip_is_power_of_2(n))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "n_fft must be a power of 2");
    if (hop == 0 || hop > n)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "hop must be in [1, n_fft]");
    if (!w || !g)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "window or output pointer is null");
    if (norm != SDSP_HIP_ISTFT_NORMALIZED && norm != SDSP_HIP_ISTFT_RAW)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "norm must be SDSP_HIP_ISTFT_NORMALIZED or SDSP_HIP_ISTFT_RAW");
    std::vector<double> env(hop, 0.0);
    for (uint32_t i = 0; i < n; i++) // i ascending: each env[r] sums its k in ascending order
        env[i % hop] += w[i] * w[i];
    double lo = env[0], hi = env[0];
    for (uint32_t r = 1; r < hop; r++) {
        lo = std::min(lo, env[r]);
        hi = std::max(hi, env[r]);
    }
    if (env_min)
        *env_min = lo;
    if (env_max)
        *env_max = hi;
    if (norm == SDSP_HIP_ISTFT_NORMALIZED && !(lo > 1e-10 * hi))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the window breaks the NOLA condition at this hop (min of the squared-window overlap-add "
                                              "<= 1e-10 x its max): overlap-add cannot be normalised; use a shorter hop, another "
                                              "window or SDSP_HIP_ISTFT_RAW");
    for (uint32_t i = 0; i < n; i++)
        g[i] = norm == SDSP_HIP_ISTFT_RAW ? w[i] : w[i] / env[i % hop];
    return SDSP_HIP_OK;
}
// minimum-norm least-squares solution x (n) of A x = b, A (r x n, row-major), by a one-sided Jacobi singular value decomposition of
// the taller of A and A^T: columns of B are rotated until they are orthogonal (B V = U S), singular values below eps max(r, n) S_max
// are dropped, and x = A^+ b is assembled from what is left.  Backward stable; the systems here have at most 2 P - 1 rows.
// Cost per sweep: min(r, n)^2 / 2 column pairs of max(r, n) elements, a few sweeps -- over all residues of a prototype O(P^2 L) per sweep
// (minutes on one thread only at the extreme P = 64, L = 2^20).
void min_norm_solve(const std::vector<double> &a, size_t r, size_t n, const std::vector<double> &b, std::vector<double> &x)
{
    const bool transposed = n >= r; // B = A^T (n x r), else B = A (r x n)
    const size_t rows = transposed ? n : r, cols = transposed ? r : n;
    std::vector<double> w(rows * cols), v(cols * cols, 0.0); // column-major: column k at [k rows, (k + 1) rows)
    for (size_t i = 0; i < r; i++)
        for (size_t j = 0; j < n; j++)
            (transposed ? w[i * rows + j] : w[j * rows + i]) = a[i * n + j];
    for (size_t k = 0; k < cols; k++)
        v[k * cols + k] = 1.0;
    const double eps = 2.220446049250313e-16;
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (size_t p = 0; p + 1 < cols; p++) {
            for (size_t q = p + 1; q < cols; q++) {
                double *wp = &w[p * rows], *wq = &w[q * rows];
                double alpha = 0, beta = 0, gamma = 0;
                for (size_t i = 0; i < rows; i++) {
                    alpha += wp[i] * wp[i];
                    beta += wq[i] * wq[i];
                    gamma += wp[i] * wq[i];
                }
                if (gamma == 0.0 || std::fabs(gamma) <= eps * std::sqrt(alpha * beta))
                    continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (size_t i = 0; i < rows; i++) {
                    const double xp = wp[i], xq = wq[i];
                    wp[i] = c * xp - s * xq;
                    wq[i] = s * xp + c * xq;
                }
                double *vp = &v[p * cols], *vq = &v[q * cols];
                for (size_t i = 0; i < cols; i++) {
                    const double xp = vp[i], xq = vq[i];
                    vp[i] = c * xp - s * xq;
                    vq[i] = s * xp + c * xq;
                }
            }
        }
        if (!rotated)
            break;
    }
    std::vector<double> s2(cols);
    double s2max = 0;
    for (size_t k = 0; k < cols; k++) {
        double acc = 0;
        for (size_t i = 0; i < rows; i++)
            acc += w[k * rows + i] * w[k * rows + i];
        s2[k] = acc;
        s2max = std::max(s2max, acc);
    }
    const double cut = eps * static_cast<double>(std::max(r, n));
    x.assign(n, 0.0);
    for (size_t k = 0; k < cols; k++) {
        if (!(s2[k] > cut * cut * s2max))
            continue;
        // transposed: A^+ = U S^-1 V^T with w_k = s_k u_k: x += w_k (v_k . b) / s_k^2; else A^+ = V S^-1 U^T: x += v_k (w_k . b) / s_k^2
        double dot = 0;
        if (transposed) {
            for (size_t i = 0; i < r; i++)
                dot += v[k * cols + i] * b[i];
            for (size_t j = 0; j < n; j++)
                x[j] += w[k * rows + j] * (dot / s2[k]);
        } else {
            for (size_t i = 0; i < r; i++)
                dot += w[k * rows + i] * b[i];
            for (size_t j = 0; j < n; j++)
                x[j] += v[k * cols + j] * (dot / s2[k]);
        }
    }
}

// the dual prototype of the polyphase synthesis banks: one small system per residue t0 of the hop
int pfb_dual_prototype(uint32_t m, uint32_t p, uint32_t hop, const double *h, double *g)
{
    if (!h || !g)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null prototype pointer");
    if (m < 2 || p == 0 || p > SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL || static_cast<uint64_t>(m) * p > SDSP_HIP_PFB_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "need m >= 2, 1 <= p <= SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL and p m <= SDSP_HIP_PFB_MAX_TAPS");
    if (hop == 0 || hop > m)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "hop must be in [1, m]");
    const int64_t len = static_cast<int64_t>(m) * p;
    double worst = 0;
    std::vector<double> a, b, x;
    for (uint32_t t0 = 0; t0 < hop; t0++) {
        const size_t n = static_cast<size_t>((len - t0 + hop - 1) / hop); // unknowns g[t0 + i hop]
        a.clear();
        b.clear();
        for (int64_t k = 1 - static_cast<int64_t>(p); k < static_cast<int64_t>(p); k++) {
            const size_t at = a.size();
            a.resize(at + n, 0.0);
            bool any = false;
            for (size_t i = 0; i < n; i++) {
                const int64_t q = static_cast<int64_t>(t0) + static_cast<int64_t>(i) * hop + k * m;
                if (q >= 0 && q < len && h[q] != 0.0) {
                    a[at + i] = h[q];
                    any = true;
                }
            }
            if (any) {
                b.push_back(k == 0 ? 1.0 : 0.0);
            } else { // a row that is identically zero: nothing to solve, and nothing can make its k = 0 right-hand side
                a.resize(at);
                if (k == 0)
                    worst = std::max(worst, 1.0);
            }
        }
        const size_t r = b.size();
        x.assign(n, 0.0);
        if (r)
            min_norm_solve(a, r, n, b, x);
        for (size_t i = 0; i < r; i++) {
            double acc = 0;
            for (size_t j = 0; j < n; j++)
                acc += a[i * n + j] * x[j];
            worst = std::max(worst, std::fabs(acc - b[i]));
        }
        for (size_t i = 0; i < n; i++)
            g[t0 + i * hop] = x[i];
    }
    if (!(worst <= 1e-9))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the analysis prototype has no dual of its own support at this hop (perfect-reconstruction "
                                              "residual above 1e-9): use a shorter hop or another prototype");
    return SDSP_HIP_OK;
}
} // namespace sdsp_hip

using namespace sdsp_hip;

extern "C" {

const char *sdsp_hip_last_error_string(void) { return g_last_error.c_str(); }
// SDSP_HIP_SOURCE_HASH: sha256 over csrc/ and include/ at build time (simpledsp_amd/build.py); the Python loader compares
// it with the sources beside the library and refuses a stale .so
#ifndef SDSP_HIP_SOURCE_HASH
#define SDSP_HIP_SOURCE_HASH "unhashed"
#endif
const char *sdsp_hip_version(void) { return "sdsp-hip 0.3 (gfx950) src:" SDSP_HIP_SOURCE_HASH; }

// fft.h:12-19
unsigned sdsp_hip_log2(unsigned num)
{
    unsigned r = 0;
    while ((num >>= 1) > 0u)
        r++;
    return r;
}
// fft.h:21-28
unsigned sdsp_hip_log4(unsigned num)
{
    unsigned r = 0;
    while ((num >>= 2) > 0u)
        r++;
    return r;
}
// fft.h:31-37
int sdsp_hip_is_power_of_2(unsigned num) { return num != 0 && (num & (num - 1)) == 0; }
// fft.h:40-43
int sdsp_hip_is_power_of_4(unsigned num)
{
    return sdsp_hip_is_power_of_2(num) && (sdsp_hip_log2(num) % 2 == 0);
}
// fft.h:217-236, as a digit loop
unsigned sdsp_hip_digit_reverse(unsigned n, unsigned base, unsigned x)
{
    const unsigned bits = sdsp_hip_log2(base);
    const unsigned digits = bits ? sdsp_hip_log2(n) / bits : 0;
    unsigned r = 0;
    for (unsigned d = 0; d < digits; d++) {
        r = (r << bits) | (x & (base - 1));
        x >>= bits;
    }
    return r;
}

int sdsp_hip_calc_twiddles(unsigned n, int direction, double *out)
{
    if (!sdsp_hip_is_power_of_2(n))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "FFT size must be a power of 2!");
    if (!out || (direction != SDSP_HIP_FORWARD && direction != SDSP_HIP_REVERSE))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bad argument");
    std::vector<double> w;
    make_twiddles(n, direction, w);
    std::memcpy(out, w.data(), sizeof(double) * w.size());
    return SDSP_HIP_OK;
}

int sdsp_hip_iir_design_lp(uint32_t m, double f0, double fs, double gain_in, double *a, double *b, double *gain)
{
    return design_lp(m, f0, fs, gain_in, a, b, gain);
}
int sdsp_hip_iir_design_hp(uint32_t m, double f0, double fs, double gain_in, double *a, double *b, double *gain)
{
    return design_hp(m, f0, fs, gain_in, a, b, gain);
}
int sdsp_hip_iir_design_bp(uint32_t m, double f0, double fs, double q, double gain_in, double *a, double *b, double *gain)
{
    return design_bp(m, f0, fs, q, gain_in, a, b, gain);
}
int sdsp_hip_iir_design_bs(uint32_t m, double f0, double fs, double q, double gain_in, double *a, double *b, double *gain)
{
    return design_bs(m, f0, fs, q, gain_in, a, b, gain);
}
int sdsp_hip_fir_design(uint32_t taps, int filter_type, double f0, double fs, double q, double gain_in, double *h)
{
    return design_fir(taps, filter_type, f0, fs, q, gain_in, h);
}
int sdsp_hip_iir_preload(uint32_t m, int filter_type, const double *a, const double *b, double gain, double value, double *mem)
{
    return preload(m, filter_type, a, b, gain, value, mem);
}
int sdsp_hip_resample_design(uint32_t taps, uint32_t up, uint32_t down, double *h)
{
    if (up == 0 || down == 0 || up > SDSP_HIP_RESAMPLE_MAX_FACTOR || down > SDSP_HIP_RESAMPLE_MAX_FACTOR)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "up and down must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    if (up == 1 && down == 1)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "up = down = 1 changes no rate: there is no band to protect");
    const uint32_t r = up > down ? up : down;
    return design_fir(taps, SDSP_HIP_FILTER_LOW_PASS, 1.0 / r, 2.0, 0.0, static_cast<double>(up), h);
}
int sdsp_hip_resample_out_samples(uint32_t up, uint32_t down, uint64_t samples, uint64_t *out)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *out = 0;
    if (up == 0 || down == 0 || up > SDSP_HIP_RESAMPLE_MAX_FACTOR || down > SDSP_HIP_RESAMPLE_MAX_FACTOR)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "up and down must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    uint32_t a = up, b = down;
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    const uint32_t q = down / a;
    if (samples % q)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be a multiple of down / gcd(up, down)");
    *out = samples / q * (up / a);
    return SDSP_HIP_OK;
}
// e^(+2 pi i a / 2^32) for a 32-bit phase word.  The reduction is in integers: the quadrant is a's top two bits, and inside the
// quadrant the angle is folded to [0, pi / 4] before libm sees it, so the four axis values are exact and every other value has
// the relative accuracy of libm on a small argument.
static void ddc_unit_phase(uint32_t a, double *re, double *im)
{
    const uint32_t quadrant = a >> 30, r = a & 0x3fffffffu;
    const double scale = 2 * M_PI / 4294967296.0;
    double c, s;
    if (r <= 0x20000000u) {
        c = std::cos(scale * r);
        s = std::sin(scale * r);
    } else { // cos(pi / 2 - t) = sin(t)
        c = std::sin(scale * (0x40000000u - r));
        s = std::cos(scale * (0x40000000u - r));
    }
    switch (quadrant) {
    case 0: *re = c; *im = s; break;
    case 1: *re = -s; *im = c; break;
    case 2: *re = -c; *im = -s; break;
    default: *re = s; *im = -c; break;
    }
}
int sdsp_hip_ddc_phase_word(double cycles_per_sample, uint32_t *fcw)
{
    if (!fcw)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *fcw = 0;
    if (!(cycles_per_sample >= -0.5 && cycles_per_sample <= 0.5)) // NaN included
        return fail(SDSP_HIP_ERR_INVALID_ARG, "frequency must be in [-0.5, 0.5] cycles per sample");
    // the scaling is exact; ties go to the even word (Python's round); -2^31 .. 2^31 wraps to the 32-bit word
    const int64_t w = static_cast<int64_t>(std::nearbyint(cycles_per_sample * 4294967296.0));
    *fcw = static_cast<uint32_t>(static_cast<uint64_t>(w) & 0xffffffffull);
    return SDSP_HIP_OK;
}
int sdsp_hip_ddc_band_taps(uint32_t taps, const double *h, uint32_t fcw, double *g)
{
    if (!h || !g)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null pointer");
    if (taps == 0 || taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_FIR_MAX_TAPS]");
    for (uint32_t k = 0; k < taps; k++) {
        double c, s;
        ddc_unit_phase(k * fcw, &c, &s); // k fcw mod 2^32: unsigned wrap-around
        g[2 * k] = h[k] * c;
        g[2 * k + 1] = h[k] * s;
    }
    return SDSP_HIP_OK;
}
int sdsp_hip_ddc_oscillator(double *coarse, double *fine)
{
    if (!coarse || !fine)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    for (uint32_t a = 0; a < 65536; a++) { // the conjugates: e^(-2 pi i a / 65536) and e^(-2 pi i a / 2^32)
        double c, s;
        ddc_unit_phase(a << 16, &c, &s);
        coarse[2 * a] = c;
        coarse[2 * a + 1] = -s;
        ddc_unit_phase(a, &c, &s);
        fine[2 * a] = c;
        fine[2 * a + 1] = -s;
    }
    return SDSP_HIP_OK;
}
int sdsp_hip_pll_oscillator(double *coarse, double *fine)
{
    if (!coarse || !fine)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    for (uint32_t a = 0; a < 2048; a++) { // the conjugates: e^(-2 pi i a / 2^11) and e^(-2 pi i a / 2^22)
        double c, s;
        ddc_unit_phase(a << 21, &c, &s);
        coarse[2 * a] = c;
        coarse[2 * a + 1] = -s;
        ddc_unit_phase(a << 10, &c, &s);
        fine[2 * a] = c;
        fine[2 * a + 1] = -s;
    }
    return SDSP_HIP_OK;
}
int sdsp_hip_pll_gains(double bn, double zeta, double amplitude, int mode, double *alpha, double *beta)
{
    if (!alpha || !beta)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *alpha = *beta = 0.0;
    if (mode != SDSP_HIP_PLL_CROSS && mode != SDSP_HIP_PLL_BPSK && mode != SDSP_HIP_PLL_QPSK)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "mode must be SDSP_HIP_PLL_CROSS, SDSP_HIP_PLL_BPSK or SDSP_HIP_PLL_QPSK");
    if (!(std::isfinite(bn) && bn > 0.0 && std::isfinite(zeta) && zeta > 0.0 && std::isfinite(amplitude) && amplitude > 0.0))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bn, zeta and amplitude must be finite and > 0");
    const double theta = bn / (zeta + 1.0 / (4.0 * zeta)), d = 1.0 + 2.0 * zeta * theta + theta * theta;
    const double kd = mode == SDSP_HIP_PLL_CROSS ? amplitude : mode == SDSP_HIP_PLL_BPSK ? amplitude * amplitude : amplitude * std::sqrt(2.0);
    *alpha = 4.0 * zeta * theta / (d * kd * (2.0 * M_PI));
    *beta = 4.0 * theta * theta / (d * kd * (2.0 * M_PI));
    return SDSP_HIP_OK;
}
// symbol-timing recovery banks: L a power of two in [1, 128], T in [1, 64], L T <= 4096
static int timing_check_shape(uint32_t phases, uint32_t taps)
{
    if (phases == 0 || phases > SDSP_HIP_TIMING_MAX_PHASES || (phases & (phases - 1)))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "phases must be a power of 2 in [1, SDSP_HIP_TIMING_MAX_PHASES]");
    if (taps == 0 || taps > SDSP_HIP_TIMING_MAX_TAPS || static_cast<uint64_t>(phases) * taps > SDSP_HIP_TIMING_MAX_TABLE)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps per phase must be in [1, SDSP_HIP_TIMING_MAX_TAPS] and phases * taps <= SDSP_HIP_TIMING_MAX_TABLE");
    return SDSP_HIP_OK;
}
int sdsp_hip_timing_step(double sps, uint64_t *step0)
{
    if (!step0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *step0 = 0;
    if (!(sps >= 2.0 && sps <= 128.0)) // NaN included
        return fail(SDSP_HIP_ERR_INVALID_ARG, "samples per symbol must be in [2, 128]");
    // the scaling is exact; ties go to the even word (Python's round)
    *step0 = static_cast<uint64_t>(std::nearbyint(sps * 2147483648.0));
    return SDSP_HIP_OK;
}
// every half step is at least step0 - 2^31, so at most n = ceil(S 2^32 / (step0 - 2^31)) strobes start below S (the first at t >= 0); a
// call that begins on a symbol strobe has (n + 1) / 2 of them
static uint64_t timing_max_out_of(uint64_t step0, uint64_t samples)
{
    const uint64_t least = step0 - (1ull << 31), n = ((samples << 32) + least - 1) / least; // samples < 2^31: below 2^63
    return (n + 1) / 2;
}
int sdsp_hip_timing_max_out_for(uint64_t step0, uint64_t samples, uint64_t *n)
{
    if (!n)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *n = 0;
    if (step0 < SDSP_HIP_TIMING_MIN_STEP || step0 > SDSP_HIP_TIMING_MAX_STEP)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "step0 must be in [2^32, 2^38]");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    *n = timing_max_out_of(step0, samples);
    return SDSP_HIP_OK;
}
int sdsp_hip_timing_gains(double bn, double zeta, double kd, double sps, double *alpha, double *beta)
{
    if (!alpha || !beta)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *alpha = *beta = 0.0;
    if (!(std::isfinite(bn) && bn > 0.0 && std::isfinite(zeta) && zeta > 0.0 && std::isfinite(kd) && kd > 0.0 && std::isfinite(sps) && sps > 0.0))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "bn, zeta, kd and sps must be finite and > 0");
    const double theta = bn / (zeta + 1.0 / (4.0 * zeta)), d = 1.0 + 2.0 * zeta * theta + theta * theta;
    *alpha = 4.0 * zeta * theta / (d * kd) * sps / 2.0;
    *beta = 4.0 * theta * theta / (d * kd) * sps / 2.0;
    return SDSP_HIP_OK;
}
int sdsp_hip_timing_design(uint32_t phases, uint32_t taps, double sps, double rolloff, double *h)
{
    if (int rc = timing_check_shape(phases, taps))
        return rc;
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    if (!(std::isfinite(sps) && sps > 0.0))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "samples per symbol must be finite and > 0");
    if (!(rolloff > 0.0 && rolloff <= 1.0))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "rolloff must be in (0, 1]");
    const uint64_t n = static_cast<uint64_t>(phases) * taps;
    const double centre = 0.5 * static_cast<double>(n - 1), per_symbol = sps * phases, b = rolloff;
    double sum = 0.0;
    for (uint64_t j = 0; j < n; j++) {
        const double tau = (static_cast<double>(j) - centre) / per_symbol; // in symbols
        const double u = 4.0 * b * tau;
        double v;
        if (tau == 0.0)
            v = 1.0 - b + 4.0 * b / M_PI;
        else if (std::fabs(std::fabs(u) - 1.0) < 1e-9) // |tau| = 1 / (4 b): the limit, exact to the second order of the distance
            v = b / std::sqrt(2.0) * ((1.0 + 2.0 / M_PI) * std::sin(M_PI / (4.0 * b)) + (1.0 - 2.0 / M_PI) * std::cos(M_PI / (4.0 * b)));
        else
            v = (std::sin(M_PI * tau * (1.0 - b)) + u * std::cos(M_PI * tau * (1.0 + b))) / (M_PI * tau * (1.0 - u * u));
        h[j] = v;
        sum += v;
    }
    for (uint64_t j = 0; j < n; j++)
        h[j] *= static_cast<double>(phases) / sum;
    return SDSP_HIP_OK;
}
int sdsp_hip_ddc_out_samples(uint32_t down, uint64_t samples, uint64_t *out)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *out = 0;
    if (down == 0 || down > SDSP_HIP_RESAMPLE_MAX_FACTOR)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "down must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    if (samples % down)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be a multiple of down");
    *out = samples / down;
    return SDSP_HIP_OK;
}
int sdsp_hip_duc_out_samples(uint32_t up, uint64_t samples, uint64_t *out)
{
    if (!out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *out = 0;
    if (up == 0 || up > SDSP_HIP_RESAMPLE_MAX_FACTOR)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "up must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    if (samples > (1ull << 62) / up)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples times up must stay below 2^62");
    *out = samples * up;
    return SDSP_HIP_OK;
}
// arbitrary-ratio resampler banks: L a power of two in [1, 1024] and L T <= SDSP_HIP_FIR_MAX_TAPS
static int arb_check_shape(uint32_t phases, uint32_t taps)
{
    if (phases == 0 || phases > SDSP_HIP_ARB_MAX_PHASES || (phases & (phases - 1)))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "phases must be a power of 2 in [1, SDSP_HIP_ARB_MAX_PHASES]");
    if (taps == 0 || static_cast<uint64_t>(phases) * taps > SDSP_HIP_FIR_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps per phase must be >= 1 and phases * taps <= SDSP_HIP_FIR_MAX_TAPS");
    return SDSP_HIP_OK;
}
int sdsp_hip_arb_step(double in_per_out, uint64_t *step)
{
    if (!step)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *step = 0;
    if (!(in_per_out >= 1.0 / 1024 && in_per_out <= 1024.0)) // NaN included
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input samples per output sample must be in [1 / 1024, 1024]");
    // the scaling is exact; ties go to the even word (Python's round)
    *step = static_cast<uint64_t>(std::nearbyint(in_per_out * 4294967296.0));
    return SDSP_HIP_OK;
}
int sdsp_hip_arb_out_samples(uint64_t step, uint64_t time, uint64_t samples, uint64_t *n_out, uint64_t *next_time)
{
    if (!n_out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *n_out = 0;
    if (next_time)
        *next_time = 0;
    if (step < SDSP_HIP_ARB_MIN_STEP || step > SDSP_HIP_ARB_MAX_STEP)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "step must be in [2^22, 2^42]");
    if (time >= (1ull << 63))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "time must be below 2^63");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    const uint64_t end = samples << 32; // < 2^63
    uint64_t n = 0, next = time - end;
    if (time < end) {
        n = (end - time + step - 1) / step; // < 2^63 + 2^42
        next = time + n * step - end;       // < step: n step < end - time + step
    }
    if (n >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "the call would produce 2^31 or more outputs per channel");
    *n_out = n;
    if (next_time)
        *next_time = next;
    return SDSP_HIP_OK;
}
int sdsp_hip_arb_design(uint32_t phases, uint32_t taps, double max_in_per_out, double *h)
{
    if (int rc = arb_check_shape(phases, taps))
        return rc;
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    if (!(max_in_per_out >= 1.0 / 1024 && max_in_per_out <= 1024.0))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "input samples per output sample must be in [1 / 1024, 1024]");
    if (phases == 1 && max_in_per_out <= 1.0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "one phase and a ratio <= 1 change no rate downwards: there is no band to protect");
    const double cutoff = (max_in_per_out > 1.0 ? 1.0 / max_in_per_out : 1.0) / phases;
    return design_fir(phases * taps, SDSP_HIP_FILTER_LOW_PASS, cutoff, 2.0, 0.0, static_cast<double>(phases), h);
}
int sdsp_hip_arb_tables(uint32_t phases, uint32_t taps, const double *h, double *table_h, double *table_d)
{
    if (int rc = arb_check_shape(phases, taps))
        return rc;
    if (!h || !table_h || !table_d)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null pointer");
    const uint64_t n = static_cast<uint64_t>(phases) * taps;
    for (uint32_t p = 0; p < phases; p++)
        for (uint32_t k = 0; k < taps; k++) {
            const uint64_t i = static_cast<uint64_t>(k) * phases + p;
            table_h[static_cast<uint64_t>(p) * taps + k] = h[i];
            table_d[static_cast<uint64_t>(p) * taps + k] = (i + 1 < n ? h[i + 1] : 0.0) - h[i];
        }
    return SDSP_HIP_OK;
}
// CIC decimator banks: 1 <= N <= 8, 2 <= R <= 16384, M in {1, 2}, N M R <= SDSP_HIP_CIC_MAX_HISTORY
static int cic_check_shape(uint32_t order, uint32_t down, uint32_t delay)
{
    if (order == 0 || order > SDSP_HIP_CIC_MAX_ORDER)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "order must be in [1, SDSP_HIP_CIC_MAX_ORDER]");
    if (down < 2 || down > SDSP_HIP_CIC_MAX_DOWN)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "down must be in [2, SDSP_HIP_CIC_MAX_DOWN]");
    if (delay != 1 && delay != 2)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "delay must be 1 or 2");
    if (static_cast<uint64_t>(order) * down * delay > SDSP_HIP_CIC_MAX_HISTORY)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "order * delay * down must be <= SDSP_HIP_CIC_MAX_HISTORY");
    return SDSP_HIP_OK;
}
// (R M)^N in exact integers: at most 8192^8 = 2^104 within the history limit
static unsigned __int128 cic_gain(uint32_t order, uint32_t down, uint32_t delay)
{
    unsigned __int128 g = 1;
    for (uint32_t s = 0; s < order; s++)
        g *= static_cast<uint64_t>(down) * delay;
    return g;
}
int sdsp_hip_cic_growth(uint32_t order, uint32_t down, uint32_t delay, uint32_t *bits)
{
    if (!bits)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *bits = 0;
    if (int rc = cic_check_shape(order, down, delay))
        return rc;
    uint32_t b = 0;
    for (unsigned __int128 v = cic_gain(order, down, delay) - 1; v; v >>= 1)
        b++;
    *bits = b;
    return SDSP_HIP_OK;
}
int sdsp_hip_cic_out_samples(uint32_t down, uint64_t position, uint64_t samples, uint64_t *n_out)
{
    if (!n_out)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *n_out = 0;
    if (down < 2 || down > SDSP_HIP_CIC_MAX_DOWN)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "down must be in [2, SDSP_HIP_CIC_MAX_DOWN]");
    if (samples >= (1ull << 31))
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be below 2^31");
    *n_out = (position % down + samples) / down; // floor((position + S) / R) - floor(position / R) without the sum's overflow
    return SDSP_HIP_OK;
}
int sdsp_hip_cic_unity_scale(uint32_t order, uint32_t down, uint32_t delay, double *scale)
{
    if (!scale)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *scale = 0.0;
    if (int rc = cic_check_shape(order, down, delay))
        return rc;
    const unsigned __int128 g = cic_gain(order, down, delay);
    // (double)g with one rounding: g has at most 105 bits; its top 64 bits, with a sticky bit for the rest, round to 53 bits as the
    // whole does, and the power-of-two scaling back is exact
    uint32_t shift = 0;
    unsigned __int128 top = g;
    bool sticky = false;
    while (top >> 64) {
        sticky = sticky || (top & 1);
        top >>= 1;
        shift++;
    }
    uint64_t t = static_cast<uint64_t>(top);
    if (sticky)
        t |= 1; // shift > 0 means t has 64 significant bits: bit 0 lies below the rounding position and its half-way bit
    *scale = 1.0 / std::ldexp(static_cast<double>(t), static_cast<int>(shift));
    return SDSP_HIP_OK;
}
int sdsp_hip_cic_taps(uint32_t order, uint32_t down, uint32_t delay, uint64_t *h)
{
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    if (int rc = cic_check_shape(order, down, delay))
        return rc;
    const uint64_t box = static_cast<uint64_t>(down) * delay;
    uint64_t len = 1;
    h[0] = 1;
    std::vector<uint64_t> sum; // running sums of the stage before, sum[k] = h[0] + .. + h[k - 1], mod 2^64
    for (uint32_t s = 0; s < order; s++) {
        sum.assign(len + 1, 0);
        for (uint64_t k = 0; k < len; k++)
            sum[k + 1] = sum[k] + h[k];
        const uint64_t next = len + box - 1;
        for (uint64_t k = 0; k < next; k++) { // h'[k] = h[k - box + 1] + .. + h[k] over the indices that exist
            const uint64_t hi = k + 1 < len ? k + 1 : len, lo = k + 1 > box ? k + 1 - box : 0;
            h[k] = sum[hi] - sum[lo];
        }
        len = next;
    }
    return SDSP_HIP_OK;
}
// CIC interpolator banks: the decimator's shape limits with R the up-sampling; the gain of every polyphase branch is
// R^(N - 1) M^N = (R M)^N / R, at most 2^92
int sdsp_hip_cic_interp_growth(uint32_t order, uint32_t up, uint32_t delay, uint32_t *bits)
{
    if (!bits)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *bits = 0;
    if (int rc = cic_check_shape(order, up, delay))
        return rc;
    uint32_t b = 0;
    for (unsigned __int128 v = cic_gain(order, up, delay) / up - 1; v; v >>= 1)
        b++;
    *bits = b;
    return SDSP_HIP_OK;
}
int sdsp_hip_cic_interp_unity_scale(uint32_t order, uint32_t up, uint32_t delay, double *scale)
{
    if (!scale)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *scale = 0.0;
    if (int rc = cic_check_shape(order, up, delay))
        return rc;
    // (double)g with one rounding, as in sdsp_hip_cic_unity_scale: the top 64 bits with a sticky bit for the rest
    unsigned __int128 top = cic_gain(order, up, delay) / up;
    uint32_t shift = 0;
    bool sticky = false;
    while (top >> 64) {
        sticky = sticky || (top & 1);
        top >>= 1;
        shift++;
    }
    uint64_t t = static_cast<uint64_t>(top);
    if (sticky)
        t |= 1;
    *scale = 1.0 / std::ldexp(static_cast<double>(t), static_cast<int>(shift));
    return SDSP_HIP_OK;
}
int sdsp_hip_stft_window(int kind, uint32_t n, double *w)
{
    if (!w)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    if (kind < SDSP_HIP_WINDOW_RECT || kind > SDSP_HIP_WINDOW_BLACKMAN)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "window kind must be SDSP_HIP_WINDOW_RECT / HANN / HAMMING / BLACKMAN");
    if (n == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "a window needs at least one point");
    // periodic (scipy fftbins = True): the first n points of the symmetric window of n + 1
    const double two_pi = 2 * M_PI;
    for (uint32_t k = 0; k < n; k++) {
        const double c1 = std::cos(two_pi * k / n);
        switch (kind) {
        case SDSP_HIP_WINDOW_RECT: w[k] = 1.0; break;
        case SDSP_HIP_WINDOW_HANN: w[k] = 0.5 - 0.5 * c1; break;
        case SDSP_HIP_WINDOW_HAMMING: w[k] = 0.54 - 0.46 * c1; break;
        default: w[k] = 0.42 - 0.5 * c1 + 0.08 * std::cos(2.0 * two_pi * k / n); break;
        }
    }
    return SDSP_HIP_OK;
}
int sdsp_hip_stft_frames(uint32_t hop, uint64_t samples, uint64_t *frames)
{
    if (!frames)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *frames = 0;
    if (hop == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "hop must be >= 1");
    if (samples % hop)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be a multiple of hop");
    *frames = samples / hop;
    return SDSP_HIP_OK;
}
int sdsp_hip_pfb_frames(uint32_t hop, uint64_t samples, uint64_t *frames) { return sdsp_hip_stft_frames(hop, samples, frames); }
int sdsp_hip_pfb_prototype(int window_kind, uint32_t m, uint32_t p, double *h)
{
    if (!h)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    if (window_kind < SDSP_HIP_WINDOW_RECT || window_kind > SDSP_HIP_WINDOW_BLACKMAN)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "window kind must be SDSP_HIP_WINDOW_RECT / HANN / HAMMING / BLACKMAN");
    if (m < 2 || p == 0 || p > SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL || static_cast<uint64_t>(m) * p > SDSP_HIP_PFB_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "need m >= 2, 1 <= p <= SDSP_HIP_PFB_MAX_TAPS_PER_CHANNEL and p m <= SDSP_HIP_PFB_MAX_TAPS");
    return windowed_sinc_lowpass(static_cast<uint64_t>(m) * p, 1.0 / m, window_kind, h);
}
int sdsp_hip_pfb_dual_prototype(uint32_t m, uint32_t p, uint32_t hop, const double *h, double *g)
{
    return pfb_dual_prototype(m, p, hop, h, g);
}
int sdsp_hip_welch_frames(uint32_t n_fft, uint32_t hop, uint64_t position, uint64_t samples, uint64_t *frames)
{
    if (!frames)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *frames = 0;
    if (n_fft == 0 || hop == 0)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "n_fft and hop must be >= 1");
    if (samples > ~0ull - position)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "position + samples overflows");
    // segments m with m hop + N <= P: 0 for P < N, else (P - N) / hop + 1; the call counts those ending in (position, position + S]
    auto ended = [&](uint64_t p) { return p < n_fft ? 0 : (p - n_fft) / hop + 1; };
    *frames = ended(position + samples) - ended(position);
    return SDSP_HIP_OK;
}
int sdsp_hip_istft_synthesis_window(uint32_t n_fft, uint32_t hop, const double *window, int norm, double *g)
{
    return istft_synthesis(n_fft, hop, window, norm, g, nullptr, nullptr);
}
int sdsp_hip_iir_steady_state(uint32_t sections, int kind, const double *a, const double *b, double gain, double *s)
{
    return iir_steady_state(sections, kind, a, b, gain, s);
}
int sdsp_hip_filtfilt_default_padlen(uint32_t sections, int kind, const double *a, const double *b, uint32_t *padlen)
{
    return filtfilt_default_padlen(sections, kind, a, b, padlen);
}
// I0(x) for x >= 0 by its power series sum ((x / 2)^k / k!)^2: every term positive, so nothing cancels; ends when a term no longer
// changes the sum
static double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; k++) {
        term *= q / (static_cast<double>(k) * k);
        const double next = sum + term;
        if (next == sum)
            break;
        sum = next;
    }
    return sum;
}
int sdsp_hip_beam_delay_taps(double tau, double weight, uint32_t taps, double beta, uint32_t *delay, double *g)
{
    if (!delay || !g)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "null output pointer");
    *delay = 0;
    if (taps == 0 || taps > SDSP_HIP_BEAM_MAX_TAPS)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "taps must be in [1, SDSP_HIP_BEAM_MAX_TAPS]");
    if (!std::isfinite(tau) || !std::isfinite(weight) || !std::isfinite(beta))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "tau, weight and beta must be finite");
    if (tau < 0.0 || tau >= static_cast<double>(SDSP_HIP_BEAM_MAX_DELAY))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "tau must be in [0, SDSP_HIP_BEAM_MAX_DELAY)");
    if (beta < 0.0)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "beta must be >= 0");
    if (taps == 1) { // the nearest whole sample
        *delay = static_cast<uint32_t>(std::floor(tau + 0.5));
        g[0] = weight;
        return SDSP_HIP_OK;
    }
    const double d = std::floor(tau), mu = tau - d;
    const double c0 = static_cast<double>((taps - 1) / 2), half = 0.5 * (static_cast<double>(taps) + 1.0), i0b = bessel_i0(beta);
    double sum = 0.0;
    for (uint32_t t = 0; t < taps; t++) {
        const double u = static_cast<double>(t) - c0 - mu, r = u / half, pu = M_PI * u;
        const double arg = 1.0 - r * r;
        const double w = bessel_i0(beta * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
        g[t] = (u == 0.0 ? 1.0 : std::sin(pu) / pu) * w;
        sum += g[t];
    }
    if (!(std::fabs(sum) > 0.0) || !std::isfinite(sum))
        return fail(SDSP_HIP_ERR_INVALID_ARG, "the window leaves taps that sum to zero: nothing to scale to the weight");
    for (uint32_t t = 0; t < taps; t++)
        g[t] = g[t] / sum * weight;
    *delay = static_cast<uint32_t>(d);
    return SDSP_HIP_OK;
}
}
