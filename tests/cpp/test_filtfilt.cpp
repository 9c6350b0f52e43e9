// sdsp::filtfilt_bank (include/sdsp/filtfilt.h) against a double Direct-Form-I forward-backward filter written out in this program
// (odd extension of scipy's default length, steady-state initial conditions), on the host entry and on device pointers.  Exit 0 = pass,
// 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/filtfilt.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kSections = 4;
constexpr std::uint64_t kChannels = 5, kSamples = 1000;

// one pass of the cascade over e, every age of level j starting at s_j e[0]
std::vector<double> cascade(const std::vector<double> &e, const std::array<double, 3 * kSections> &a, double gain,
                            const std::array<double, kSections + 1> &s)
{
    std::vector<double> cur(e.size());
    for (std::size_t n = 0; n < e.size(); n++)
        cur[n] = e[n] * gain;
    for (std::uint32_t j = 0; j < kSections; j++) {
        const double a1 = a[3 * j + 1], a2 = a[3 * j + 2];
        double x1 = s[j] * e[0], x2 = x1, y1 = s[j + 1] * e[0], y2 = y1;
        for (std::size_t n = 0; n < cur.size(); n++) {
            const double x = cur[n];
            const double y = x + 2.0 * x1 + x2 - a1 * y1 - a2 * y2; // the low-pass numerator 1 + 2 z^-1 + z^-2
            x2 = x1;
            x1 = x;
            y2 = y1;
            y1 = y;
            cur[n] = y;
        }
    }
    return cur;
}

std::vector<double> filtfilt_ref(const double *x, std::uint64_t len, const std::array<double, 3 * kSections> &a, double gain,
                                 const std::array<double, kSections + 1> &s, std::uint32_t pad)
{
    std::vector<double> e;
    for (std::uint32_t i = 0; i < pad; i++)
        e.push_back(2.0 * x[0] - x[pad - i]);
    e.insert(e.end(), x, x + len);
    for (std::uint32_t i = 0; i < pad; i++)
        e.push_back(2.0 * x[len - 1] - x[len - 2 - i]);
    std::vector<double> u = cascade(e, a, gain, s);
    std::reverse(u.begin(), u.end());
    std::vector<double> w = cascade(u, a, gain, s);
    std::reverse(w.begin(), w.end());
    return std::vector<double>(w.begin() + pad, w.begin() + pad + static_cast<std::ptrdiff_t>(len));
}

template <typename real_t> int run(double tol)
{
    sdsp::filtfilt_bank<kSections, real_t> bank;
    bank.set_lp_coeff(2e3, 48e3);
    const sdsp_hip_filtfilt_plan_info info = bank.info();
    std::mt19937 gen(7);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::vector<real_t> x(kChannels * kSamples);
    double walk = 0.0;
    for (auto &v : x)
        v = static_cast<real_t>(walk += 0.1 * dist(gen));
    std::vector<real_t> host = x, dev_out(x.size());
    bank.process_host(host.data(), kChannels, kSamples);
    void *d = nullptr;
    sdsp::detail::check(sdsp_hip_malloc(&d, x.size() * sizeof(real_t), 0));
    sdsp::detail::check(sdsp_hip_memcpy_h2d(d, x.data(), x.size() * sizeof(real_t), 0));
    bank.process(static_cast<real_t *>(d), kChannels, kSamples, kSamples);
    sdsp::detail::check(sdsp_hip_memcpy_d2h(dev_out.data(), d, x.size() * sizeof(real_t), 0));
    sdsp_hip_free(d, 0);
    const std::array<double, kSections + 1> s = bank.steady_state();
    double worst = 0.0, peak = 0.0;
    bool same = true;
    for (std::uint64_t c = 0; c < kChannels; c++) {
        std::vector<double> xc(kSamples);
        for (std::uint64_t i = 0; i < kSamples; i++)
            xc[i] = static_cast<double>(x[c * kSamples + i]);
        const std::vector<double> want = filtfilt_ref(xc.data(), kSamples, bank.a(), bank.gain(), s, info.padlen);
        for (std::uint64_t i = 0; i < kSamples; i++) {
            worst = std::max(worst, std::fabs(static_cast<double>(host[c * kSamples + i]) - want[i]));
            peak = std::max(peak, std::fabs(want[i]));
            same = same && host[c * kSamples + i] == dev_out[c * kSamples + i];
        }
    }
    std::printf("filtfilt_bank<%u, %s>: padlen %u, kernel %s, rel err %.3e, host == device %s\n", kSections,
                sizeof(real_t) == 8 ? "double" : "float", info.padlen, info.kernel, worst / peak, same ? "yes" : "NO");
    return (worst <= tol * peak && same && info.padlen == 27) ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(1e-4) | run<double>(1e-12);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
