// sdsp::beamformer_bank (include/sdsp/beamformer.h) against a double filter-and-sum computed here, block by block on the host entry with
// blocks shorter than the history: real and complex rows, two groups, a steered dense plan (set_steering) and a sparse one with a beam
// without entries.  Every output is held within (terms + 2) u sum|g| max|x| of the double result (x 2 for complex rows), u the unit
// roundoff of the precision and terms the multiply-adds of the beam: the a-priori bound of a chain of fused or unfused multiply-adds.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/beamformer.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kTaps = 16, kSensors = 4, kBeams = 3, kGroups = 2;
constexpr std::uint64_t kBlocks[] = { 4, 0, 12, 400, 8, 1200, 36 };

template <typename real_t> int run(bool cplx, bool steered)
{
    std::mt19937 gen(11);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    const std::size_t width = cplx ? 2 : 1;
    std::vector<real_t> x(kGroups * kSensors * total * width);
    for (real_t &v : x)
        v = static_cast<real_t>(dist(gen));
    sdsp::beamformer_bank<real_t> bank(kSensors, kBeams, kTaps, kGroups, cplx);
    if (steered) { // fractional delays, a taper as weights
        std::vector<double> tau(kBeams * kSensors), w(kBeams * kSensors);
        for (std::uint32_t b = 0; b < kBeams; b++)
            for (std::uint32_t c = 0; c < kSensors; c++) {
                tau[b * kSensors + c] = 1.65 * c * (b + 0.5);
                w[b * kSensors + c] = 0.25 + 0.1 * c;
            }
        bank.set_steering(tau, w, 8.0);
    } else { // beam 1 has no entry; sensor 2 is used by no beam
        const std::vector<sdsp_hip_beam_entry> entries = { { 0, 0, 0 }, { 0, 3, 41 }, { 2, 1, 7 } };
        std::vector<double> taps(entries.size() * kTaps * width);
        for (double &v : taps)
            v = dist(gen);
        bank.set_entries(entries, taps);
    }
    std::vector<real_t> y(kGroups * kBeams * total * width);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        std::vector<real_t> in(kGroups * kSensors * blk * width), out(kGroups * kBeams * blk * width);
        for (std::uint64_t r = 0; r < kGroups * kSensors; r++)
            std::copy_n(&x[(r * total + s0) * width], blk * width, &in[r * blk * width]);
        bank.process_host(in.data(), out.data(), blk);
        for (std::uint64_t r = 0; r < kGroups * kBeams; r++)
            std::copy_n(&out[r * blk * width], blk * width, &y[(r * total + s0) * width]);
        s0 += blk;
    }
    double xmax = 0.0;
    for (real_t v : x)
        xmax = std::max(xmax, std::fabs(static_cast<double>(v)));
    const double u = sizeof(real_t) == 8 ? std::ldexp(1.0, -53) : std::ldexp(1.0, -24);
    const std::vector<sdsp_hip_beam_entry> &entries = bank.entries();
    double worst = 0.0; // error / bound
    for (std::uint32_t g = 0; g < kGroups; g++)
        for (std::uint32_t b = 0; b < kBeams; b++) {
            double gsum = 0.0, terms = 0.0;
            for (std::size_t e = 0; e < entries.size(); e++)
                if (entries[e].beam == b) {
                    terms += kTaps * (cplx ? 2.0 : 1.0);
                    for (std::size_t t = 0; t < kTaps * width; t++)
                        gsum += std::fabs(static_cast<double>(static_cast<real_t>(bank.coeff()[e * kTaps * width + t])));
                }
            const double bound = (terms + 2.0) * u * gsum * xmax * (cplx ? 2.0 : 1.0);
            for (std::uint64_t n = 0; n < total; n++) {
                std::complex<double> acc = 0.0;
                for (std::size_t e = 0; e < entries.size(); e++) {
                    if (entries[e].beam != b)
                        continue;
                    for (std::uint32_t t = 0; t < kTaps && entries[e].delay + t <= n; t++) {
                        const real_t *p = &x[((g * kSensors + entries[e].sensor) * total + (n - entries[e].delay - t)) * width];
                        const double *q = &bank.coeff()[(e * kTaps + t) * width];
                        const std::complex<double> xv(static_cast<double>(p[0]), cplx ? static_cast<double>(p[1]) : 0.0);
                        const std::complex<double> gv(static_cast<double>(static_cast<real_t>(q[0])),
                                                      cplx ? static_cast<double>(static_cast<real_t>(q[1])) : 0.0);
                        acc += gv * xv;
                    }
                }
                const real_t *o = &y[((g * kBeams + b) * total + n) * width];
                const std::complex<double> got(static_cast<double>(o[0]), cplx ? static_cast<double>(o[1]) : 0.0);
                const double err = std::abs(got - acc);
                worst = std::max(worst, bound == 0.0 ? (err == 0.0 ? 0.0 : 2.0) : err / bound); // no entry: exactly zero
            }
        }
    const sdsp_hip_beam_plan_info info = bank.info();
    std::printf("beamformer_bank<%s> %s rows, %s: %u sensors, %u beams, %u groups, %u taps, %u entries, hist %u, %u chunks, kernel %s, "
                "err / bound %.3f\n",
                sizeof(real_t) == 8 ? "double" : "float", cplx ? "complex" : "real", steered ? "steered" : "sparse", info.sensors, info.beams,
                info.groups, info.taps, info.entries, info.hist, info.chunks, info.kernel, worst);
    return worst <= 1.0 && info.hist == bank.hist() ? 0 : 1;
}
} // namespace

int main()
{
    try {
        int rc = 0;
        for (int steered = 0; steered < 2; steered++)
            for (int cplx = 0; cplx < 2; cplx++)
                rc |= run<float>(cplx != 0, steered != 0) | run<double>(cplx != 0, steered != 0);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
