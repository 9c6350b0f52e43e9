// sdsp::arb_resampler_bank (include/sdsp/arb_resample.h) against the textbook form computed here in double -- the piecewise-linear
// prototype evaluated at (k + f / 2^32) L, times x -- block by block on the host entry with blocks of irregular length (empty and
// shorter than the history included) and a step that changes in mid-stream: real and I/Q input.  f64 is held within
// 1e-12 max_p sum_k |h[k L + p]| max|x| of the double result, f32 within 1e-6 of the largest output.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/arb_resample.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kPhases = 32, kTaps = 16, kChannels = 3;
constexpr std::uint64_t kBlocks[] = { 1, 0, 3, 100, 2, 300, 9, 700 };

template <typename real_t> int run(bool cplx, double tol, bool absolute)
{
    const std::size_t width = cplx ? 2 : 1;
    std::mt19937 gen(11);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<real_t> x(kChannels * total * width);
    for (real_t &v : x)
        v = static_cast<real_t>(dist(gen));
    const std::uint64_t steps[2] = { sdsp::arb_step(0.7317), sdsp::arb_step(2.37) };
    sdsp::arb_resampler_bank<real_t> bank(kPhases, kTaps, steps[1], kChannels, cplx, true);
    bank.set_default_coeff(2.37);
    bank.set_step(steps[0]);
    bank.set_time(steps[0] / 3);
    const std::vector<double> &h = bank.coeff();
    double xmax = 0.0, phase_sum = 0.0;
    for (std::uint32_t p = 0; p < kPhases; p++) {
        double s = 0.0;
        for (std::uint32_t k = 0; k < kTaps; k++)
            s += std::fabs(h[k * kPhases + p]);
        phase_sum = std::max(phase_sum, s);
    }
    for (real_t v : x)
        xmax = std::max(xmax, std::fabs(static_cast<double>(v)));
    // the prototype joined by straight lines, zero behind its last tap
    auto proto = [&](double u) {
        const std::size_t n = h.size(), j = static_cast<std::size_t>(u);
        const double a = j < n ? h[j] : 0.0, b = j + 1 < n ? h[j + 1] : 0.0;
        return a + (u - static_cast<double>(j)) * (b - a);
    };
    double err = 0.0, ymax = 0.0;
    std::uint64_t s0 = 0, outs = 0;
    std::size_t call = 0;
    for (std::uint64_t blk : kBlocks) {
        if (call++ == 5)
            bank.set_step(steps[1]); // the ratio changes while the stream runs
        const std::uint64_t step = bank.step(), time = bank.time(), n = bank.out_samples(blk);
        std::vector<real_t> in(kChannels * blk * width), out(kChannels * n * width);
        for (std::uint64_t c = 0; c < kChannels; c++)
            std::copy_n(&x[(c * total + s0) * width], blk * width, &in[c * blk * width]);
        if (bank.process_host(in.data(), out.data(), blk) != n)
            return 1;
        for (std::uint64_t c = 0; c < kChannels; c++)
            for (std::uint64_t m = 0; m < n; m++) {
                const std::uint64_t t = time + m * step;
                const std::uint64_t i = s0 + (t >> 32); // the stream's sample index
                const double f = static_cast<double>(t & 0xffffffffull) / 4294967296.0;
                for (std::size_t w = 0; w < width; w++) {
                    double want = 0.0;
                    for (std::uint32_t k = 0; k < kTaps && k <= i; k++)
                        want += proto((k + f) * kPhases) * static_cast<double>(x[(c * total + i - k) * width + w]);
                    err = std::max(err, std::fabs(static_cast<double>(out[(c * n + m) * width + w]) - want));
                    ymax = std::max(ymax, std::fabs(want));
                }
            }
        s0 += blk;
        outs += n;
    }
    const double worst = absolute ? err / (phase_sum * xmax) : err / ymax;
    const sdsp_hip_arb_plan_info info = bank.info();
    std::printf("arb_resampler_bank<%s> %s input: %u phases x %u taps, hist %u, block %u, kernel %s, %llu outputs, err %.3e (bound %.0e)\n",
                sizeof(real_t) == 8 ? "double" : "float", cplx ? "complex" : "real", info.phases, info.taps, info.hist, info.block_out,
                info.kernel, static_cast<unsigned long long>(outs), worst, tol);
    return worst <= tol && outs > 0 ? 0 : 1;
}
} // namespace

int main()
{
    try {
        const int rc = run<float>(false, 1e-6, false) | run<float>(true, 1e-6, false) | run<double>(false, 1e-12, true) |
                       run<double>(true, 1e-12, true);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
