// sdsp::pfb_bank (include/sdsp/pfb.h) against a double DFT of the folded frames computed here, block by block on the host entry
// (blocks shorter than the history included), real and complex input, both phase references: within 4 L eps (f64) / 2e-6 (f32) of
// the largest bin of the run.  Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/pfb.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint32_t kM = 64, kP = 4, kHop = 32, kL = kM * kP;
constexpr std::uint64_t kStreams = 3;
constexpr std::uint64_t kBlocks[] = { 32, 96, 640, 32 }; // multiples of hop; 32 and 96 are shorter than hist = 224

template <typename real_t> int run(int kind, int phase, double tol)
{
    using bank_t = sdsp::pfb_bank<real_t>;
    const std::uint32_t cv = kind == SDSP_HIP_PFB_COMPLEX ? 2u : 1u;
    std::mt19937 gen(11);
    std::normal_distribution<double> dist(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<real_t> x(kStreams * total * cv);
    for (auto &v : x)
        v = static_cast<real_t>(dist(gen));
    bank_t bank(kM, kP, kHop, kStreams, kind, phase);
    bank.set_prototype(SDSP_HIP_WINDOW_HANN);
    bank.preload_filter(0.25);
    const std::uint32_t bins = bank.bins(), hist = bank.hist();
    // frames of every block: y[c][frame][bin][re, im]
    std::vector<std::vector<double>> y(kStreams);
    std::uint64_t s0 = 0;
    for (std::uint64_t blk : kBlocks) {
        const std::uint64_t frames = bank.frames(blk);
        std::vector<real_t> in(kStreams * blk * cv), out(kStreams * frames * bins * 2);
        for (std::uint64_t c = 0; c < kStreams; c++)
            std::copy_n(&x[(c * total + s0) * cv], blk * cv, &in[c * blk * cv]);
        bank.process_host(in.data(), out.data(), blk);
        for (std::uint64_t c = 0; c < kStreams; c++)
            for (std::uint64_t i = 0; i < frames * bins * 2; i++)
                y[c].push_back(static_cast<double>(out[c * frames * bins * 2 + i]));
        s0 += blk;
    }
    if (bank.position() != total)
        return 1;
    std::vector<double> h;
    for (double t : bank.taps())
        h.push_back(static_cast<double>(static_cast<real_t>(t))); // rounded once to the plan precision
    const double pi = 3.14159265358979323846;
    double num = 0.0, den = 0.0;
    for (std::uint64_t c = 0; c < kStreams; c++) {
        // the stream with the preloaded history in front: (re, im) pairs
        std::vector<double> sr(hist, static_cast<double>(static_cast<real_t>(0.25))), si(hist, 0.0);
        for (std::uint64_t i = 0; i < total; i++) {
            sr.push_back(static_cast<double>(x[(c * total + i) * cv]));
            si.push_back(cv == 2 ? static_cast<double>(x[(c * total + i) * cv + 1]) : 0.0);
        }
        const std::uint64_t frames = total / kHop;
        for (std::uint64_t j = 0; j < frames; j++) {
            // the fold, then the rotation by the absolute index of the frame's first sample (TIME)
            std::vector<double> ur(kM, 0.0), ui(kM, 0.0);
            const std::uint64_t shift = phase == SDSP_HIP_PFB_PHASE_TIME ? (j * kHop + kL * 8 - hist) % kM : 0;
            for (std::uint32_t r = 0; r < kM; r++)
                for (std::uint32_t p = 0; p < kP; p++) {
                    ur[(r + shift) % kM] += sr[j * kHop + p * kM + r] * h[p * kM + r];
                    ui[(r + shift) % kM] += si[j * kHop + p * kM + r] * h[p * kM + r];
                }
            for (std::uint32_t k = 0; k < bins; k++) {
                double re = 0.0, im = 0.0;
                for (std::uint32_t r = 0; r < kM; r++) {
                    const double a = -2.0 * pi * static_cast<double>((static_cast<std::uint64_t>(k) * r) % kM) / kM;
                    re += ur[r] * std::cos(a) - ui[r] * std::sin(a);
                    im += ur[r] * std::sin(a) + ui[r] * std::cos(a);
                }
                const double gr = y[c][(j * bins + k) * 2], gi = y[c][(j * bins + k) * 2 + 1];
                num = std::max(num, std::hypot(gr - re, gi - im));
                den = std::max(den, std::hypot(re, im));
            }
        }
    }
    const sdsp_hip_pfb_plan_info info = bank.info();
    std::printf("pfb_bank<%s> %s %s: hist %u, bins %u, fold %s, kernel %s, rel err vs DFT %.3e\n", sizeof(real_t) == 8 ? "double" : "float",
                kind == SDSP_HIP_PFB_COMPLEX ? "complex" : "real", phase == SDSP_HIP_PFB_PHASE_TIME ? "time" : "frame", info.hist,
                info.bins, info.fold, info.kernel, num / den);
    return num / den <= tol ? 0 : 1;
}
} // namespace

int main()
{
    try {
        int rc = 0;
        for (int kind : { SDSP_HIP_PFB_REAL, SDSP_HIP_PFB_COMPLEX })
            for (int phase : { SDSP_HIP_PFB_PHASE_FRAME, SDSP_HIP_PFB_PHASE_TIME })
                rc |= run<float>(kind, phase, 2e-6) | run<double>(kind, phase, 4.0 * kL * 2.220446049250313e-16);
        std::printf("%s\n", rc ? "FAILED" : "ok");
        return rc;
    } catch (const std::exception &e) {
        std::printf("no usable device: %s\n", e.what());
        return 3;
    }
}
