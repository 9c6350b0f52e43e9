// sdsp::fft_cols_plan (include/sdsp/fft_cols.h) on a 3 x 64 x 33 cube: every column of every cube through the host entry, in float and
// in double, against the direct double DFT X[k] = sum_p v[p] e^(-2 pi i p k / n) computed here -- a forward plan in place, the reverse
// plan on its result (which must return the input), and a windowed, shifted power plan out of place.  Tolerances are the transform
// tolerances of the suite: float 1e-6 normwise per column, double 4 n eps of the column's largest |X|; a power is held to
// (2 tol + tol^2) max |X|^2 plus 4 ulp.  Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/fft_cols.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <exception>
#include <limits>
#include <random>
#include <vector>

namespace
{
constexpr std::uint64_t kBatch = 3, kWidth = 33;
constexpr std::uint32_t kN = 64;
const double kPi = std::acos(-1.0);

template <typename real_t> int run()
{
    using cd = std::complex<double>;
    const bool f64 = sizeof(real_t) == 8;
    const double eps = static_cast<double>(std::numeric_limits<real_t>::epsilon());
    const double tol = f64 ? 4.0 * kN * eps : 1e-6;
    std::mt19937 gen(31);
    std::normal_distribution<double> gauss(0.0, 1.0);
    const std::size_t elems = static_cast<std::size_t>(kBatch * kN * kWidth);
    std::vector<real_t> x(2 * elems);
    for (real_t &v : x)
        v = static_cast<real_t>(gauss(gen));
    std::vector<double> win(kN);
    for (std::uint32_t p = 0; p < kN; p++)
        win[p] = static_cast<double>(static_cast<real_t>(0.5 - 0.5 * std::cos(2.0 * kPi * p / kN)));
    auto at = [&](const std::vector<real_t> &a, std::uint64_t b, std::uint32_t p, std::uint64_t r) {
        const std::size_t i = static_cast<std::size_t>((b * kN + p) * kWidth + r);
        return cd(static_cast<double>(a[2 * i]), static_cast<double>(a[2 * i + 1]));
    };
    // the direct transforms: plain and windowed
    std::vector<cd> want(elems), want_w(elems);
    for (std::uint64_t b = 0; b < kBatch; b++)
        for (std::uint64_t r = 0; r < kWidth; r++)
            for (std::uint32_t k = 0; k < kN; k++) {
                cd s(0.0, 0.0), sw(0.0, 0.0);
                for (std::uint32_t p = 0; p < kN; p++) {
                    const double ang = -2.0 * kPi * static_cast<double>((p * k) % kN) / kN;
                    const cd w(std::cos(ang), std::sin(ang)), v = at(x, b, p, r);
                    const cd vw(static_cast<double>(static_cast<real_t>(v.real() * win[p])),
                                static_cast<double>(static_cast<real_t>(v.imag() * win[p])));
                    s += v * w;
                    sw += vw * w;
                }
                const std::size_t i = static_cast<std::size_t>((b * kN + k) * kWidth + r);
                want[i] = s;
                want_w[i] = sw;
            }
    auto col_max = [&](const std::vector<cd> &a, std::uint64_t b, std::uint64_t r) {
        double m = 0.0;
        for (std::uint32_t k = 0; k < kN; k++)
            m = std::max(m, std::abs(a[static_cast<std::size_t>((b * kN + k) * kWidth + r)]));
        return m;
    };

    // forward, in place
    sdsp::fft_cols_plan<real_t> fwd(kN, kWidth);
    std::vector<real_t> y = x;
    fwd.exec_host(y.data(), y.data(), kBatch);
    double worst = 0.0;
    for (std::uint64_t b = 0; b < kBatch; b++)
        for (std::uint64_t r = 0; r < kWidth; r++) {
            double err = 0.0, nrm = 0.0;
            const double m = col_max(want, b, r);
            for (std::uint32_t k = 0; k < kN; k++) {
                const std::size_t i = static_cast<std::size_t>((b * kN + k) * kWidth + r);
                const double d = std::abs(at(y, b, k, r) - want[i]);
                err = f64 ? std::max(err, d / m) : err + d * d;
                nrm += std::norm(want[i]);
            }
            worst = std::max(worst, f64 ? err : std::sqrt(err / nrm));
        }
    // reverse undoes it
    sdsp::fft_cols_plan<real_t> rev(kN, kWidth, SDSP_HIP_REVERSE);
    std::vector<real_t> z = y;
    rev.exec_host(z.data(), z.data(), kBatch);
    double back = 0.0, xmax = 0.0;
    for (std::size_t i = 0; i < x.size(); i++) {
        back = std::max(back, std::fabs(static_cast<double>(z[i]) - static_cast<double>(x[i])));
        xmax = std::max(xmax, std::fabs(static_cast<double>(x[i])));
    }
    back /= xmax;
    // window, shift, power: out of place
    sdsp::fft_cols_plan<real_t> dop(kN, kWidth, SDSP_HIP_FORWARD, SDSP_HIP_FFT_COLS_POWER, true);
    dop.set_window(win);
    std::vector<real_t> pw(elems, real_t(-1));
    dop.exec_host(x.data(), pw.data(), kBatch);
    double pworst = 0.0; // in units of the bound
    for (std::uint64_t b = 0; b < kBatch; b++)
        for (std::uint64_t r = 0; r < kWidth; r++) {
            const double m = col_max(want_w, b, r);
            for (std::uint32_t k = 0; k < kN; k++) {
                const double ref = std::norm(want_w[static_cast<std::size_t>((b * kN + k) * kWidth + r)]);
                const double got = static_cast<double>(pw[static_cast<std::size_t>((b * kN + (k + kN / 2) % kN) * kWidth + r)]);
                const double bound = (2.0 * tol + tol * tol) * m * m + 4.0 * eps * ref;
                pworst = std::max(pworst, std::fabs(got - ref) / bound);
            }
        }
    const sdsp_hip_fft_cols_plan_info info = dop.info();
    const bool ok = worst <= tol && back <= 2.0 * tol && pworst <= 1.0 && info.n == kN && info.width == kWidth
                    && info.windowed == 1 && info.shift == 1 && info.output == SDSP_HIP_FFT_COLS_POWER && dop.launches(kBatch) == 1;
    std::printf("fft_cols_plan<%s>: %llu x %u x %llu, kernel %s, tile %u columns, %u threads, lds %u: forward err %.3g (tol %.3g), round trip "
                "%.3g, power %.3g of its bound: %s\n",
                f64 ? "double" : "float", static_cast<unsigned long long>(kBatch), kN, static_cast<unsigned long long>(kWidth), info.kernel,
                info.tile_columns, info.threads, info.lds_bytes, worst, tol, back, pworst, ok ? "within tolerance" : "OUT OF TOLERANCE");
    return ok ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>() | run<double>();
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &ex) {
        std::printf("no usable device: %s\n", ex.what());
        return 3;
    }
}
