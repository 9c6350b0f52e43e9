// sdsp::timing_bank (include/sdsp/timing.h) on symbol-timing recovery: every channel is a row of random QPSK symbols held for four
// samples each (a little off the nominal rate, with a random start) plus Gaussian noise, streamed block by block through the host
// entry (empty and one-sample blocks included) with the gains of sdsp_hip_timing_gains.  Every channel's count, its symbols, err and
// period of every block, and the stream times and integrators read back at the end, must equal the contract's recursion computed
// here in the bank's own precision: the steps of sdsp_hip.h with one std::fma per ma in float and a multiply then an add in double,
// on the prototype of sdsp_hip_timing_design rounded once to the precision.  The program is built without FMA contraction (no -march
// flag: the baseline x86-64 has no fused instruction to contract to), so the double loop rounds every product and sum on its own.
// Exit 0 = pass, 1 = mismatch, 3 = no usable device (the library has no CPU fallback).
#include <sdsp/timing.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <random>
#include <vector>

namespace
{
constexpr std::uint64_t kChannels = 70;
constexpr std::uint64_t kBlocks[] = { 4, 0, 12, 1, 400, 83, 300 };
constexpr std::uint32_t kPhases = 8, kTaps = 16;
constexpr double kSps = 4.0, kBn = 0.01, kKd = 1.0, kNoise = 0.05, kMaxDev = 0.25;

template <typename real_t> real_t ma(real_t a, real_t b, real_t c);
template <> float ma<float>(float a, float b, float c) { return std::fma(a, b, c); }
template <> double ma<double>(double a, double b, double c)
{
    const double p = a * b;
    return p + c;
}

template <typename real_t> struct loop {
    real_t integ = 0, psr = 0, psi = 0, ymr = 0, ymi = 0;
    std::uint64_t t = 0;
    std::int32_t w = 0;
    std::uint32_t parity = 0;
    std::vector<real_t> hist; // newest first, interleaved
};

template <typename real_t> bool same(real_t a, real_t b) { return std::memcmp(&a, &b, sizeof(real_t)) == 0; }

template <typename real_t> int run()
{
    std::mt19937 gen(29);
    std::normal_distribution<double> noise(0.0, kNoise);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    std::uint64_t total = 0;
    for (std::uint64_t b : kBlocks)
        total += b;
    std::vector<double> h(kPhases * kTaps);
    sdsp::detail::check(sdsp_hip_timing_design(kPhases, kTaps, kSps, 0.35, h.data()));
    double alpha = 0.0, beta = 0.0;
    sdsp::detail::check(sdsp_hip_timing_gains(kBn, std::sqrt(0.5), kKd, kSps, &alpha, &beta));
    std::vector<real_t> x(kChannels * total * 2);
    for (std::uint64_t c = 0; c < kChannels; c++) {
        const double period = kSps * (1.0 + 4e-4 * (unit(gen) - 0.5)), start = unit(gen) * period;
        std::vector<int> bits;
        for (std::uint64_t n = 0; n < total; n++) {
            const std::size_t k = static_cast<std::size_t>((static_cast<double>(n) + start) / period);
            while (bits.size() <= 2 * k + 1)
                bits.push_back(static_cast<int>(gen() & 1u));
            x[2 * (c * total + n)] = static_cast<real_t>((bits[2 * k] ? 1.0 : -1.0) * std::sqrt(0.5) + noise(gen));
            x[2 * (c * total + n) + 1] = static_cast<real_t>((bits[2 * k + 1] ? 1.0 : -1.0) * std::sqrt(0.5) + noise(gen));
        }
    }
    sdsp::timing_bank<real_t> bank(kChannels, SDSP_HIP_TIMING_GARDNER, kSps, kPhases, h, kMaxDev);
    const std::uint64_t step0 = bank.step0();
    // the contract in this precision
    const real_t a_r = static_cast<real_t>(alpha), b_r = static_cast<real_t>(beta), dev = static_cast<real_t>(kMaxDev);
    const real_t lo = static_cast<real_t>(-2147483648.0), hi = static_cast<real_t>(sizeof(real_t) == 8 ? 2147483647.0 : 2147483520.0);
    std::vector<real_t> table(kPhases * kTaps);
    for (std::uint32_t p = 0; p < kPhases; p++)
        for (std::uint32_t k = 0; k < kTaps; k++)
            table[p * kTaps + k] = static_cast<real_t>(h[k * kPhases + p]);
    std::vector<loop<real_t>> loops(kChannels);
    for (auto &l : loops)
        l.hist.assign(2 * (kTaps - 1), real_t(0));

    bool ok = true;
    std::uint64_t s0 = 0, symbols = 0;
    for (std::uint64_t blk : kBlocks) {
        const std::uint64_t cap = bank.max_out(blk);
        std::vector<real_t> bx(kChannels * blk * 2), by(kChannels * cap * 2, real_t(-7)), be(kChannels * cap, real_t(-7)),
            bp(kChannels * cap, real_t(-7));
        for (std::uint64_t c = 0; c < kChannels; c++)
            for (std::uint64_t n = 0; n < 2 * blk; n++)
                bx[2 * c * blk + n] = x[2 * (c * total + s0) + n];
        const std::vector<std::uint32_t> counts = bank.process_host(bx.data(), by.data(), be.data(), bp.data(), blk, alpha, beta);
        for (std::uint64_t c = 0; c < kChannels; c++) {
            loop<real_t> &l = loops[c];
            const real_t *row = &bx[2 * c * blk];
            auto sample = [&](std::int64_t n, int part) {
                return n >= 0 ? row[2 * n + part] : l.hist[static_cast<std::size_t>(2 * (-1 - n) + part)];
            };
            std::uint64_t m = 0;
            while ((l.t >> 32) < blk) {
                const std::int64_t i = static_cast<std::int64_t>(l.t >> 32);
                const std::uint32_t f = static_cast<std::uint32_t>(l.t), p = f >> 29; // 8 phases
                real_t zr = table[p * kTaps] * sample(i, 0), zi = table[p * kTaps] * sample(i, 1);
                for (std::uint32_t k = 1; k < kTaps; k++) {
                    zr = ma<real_t>(table[p * kTaps + k], sample(i - k, 0), zr);
                    zi = ma<real_t>(table[p * kTaps + k], sample(i - k, 1), zi);
                }
                if (l.parity == 0) {
                    l.ymr = zr;
                    l.ymi = zi;
                    l.parity = 1;
                } else {
                    const real_t dr = l.psr - zr, di = l.psi - zi;
                    const real_t e = ma<real_t>(di, l.ymi, dr * l.ymr);
                    real_t g = ma<real_t>(b_r, e, l.integ);
                    g = g < -dev ? -dev : (g > dev ? dev : g);
                    l.integ = g;
                    real_t q = ma<real_t>(a_r, e, g) * static_cast<real_t>(4294967296.0);
                    q = q < lo ? lo : (q > hi ? hi : q);
                    l.w = static_cast<std::int32_t>(std::nearbyint(q));
                    if (m < counts[c] && m < cap)
                        ok = ok && same(by[2 * (c * cap + m)], zr) && same(by[2 * (c * cap + m) + 1], zi) && same(be[c * cap + m], e) &&
                             same(bp[c * cap + m], g);
                    m++;
                    l.psr = zr;
                    l.psi = zi;
                    l.parity = 0;
                }
                l.t += step0 + static_cast<std::uint64_t>(static_cast<std::int64_t>(l.w));
            }
            l.t -= blk << 32;
            ok = ok && m == counts[c] && m <= cap;
            for (std::uint64_t k = m; k < cap; k++) // behind the count the rows keep what they held
                ok = ok && same(by[2 * (c * cap + k)], real_t(-7)) && same(be[c * cap + k], real_t(-7)) && same(bp[c * cap + k], real_t(-7));
            std::vector<real_t> nh(l.hist.size());
            for (std::int64_t j = 0; j + 1 < static_cast<std::int64_t>(kTaps); j++) {
                nh[static_cast<std::size_t>(2 * j)] = sample(static_cast<std::int64_t>(blk) - 1 - j, 0);
                nh[static_cast<std::size_t>(2 * j + 1)] = sample(static_cast<std::int64_t>(blk) - 1 - j, 1);
            }
            l.hist = nh;
            symbols += m;
        }
        s0 += blk;
    }
    // the state read back, then a fresh start
    const std::vector<real_t> integ = bank.period();
    const std::vector<std::uint64_t> time = bank.time();
    for (std::uint64_t c = 0; c < kChannels; c++)
        ok = ok && same(integ[c], loops[c].integ) && time[c] == loops[c].t;
    bank.reset();
    const bool fresh = bank.period() == std::vector<real_t>(kChannels, real_t(0)) && bank.time() == std::vector<std::uint64_t>(kChannels, 0u);
    const double per_channel = static_cast<double>(symbols) / static_cast<double>(kChannels);
    const bool rate = std::fabs(per_channel - static_cast<double>(total) / kSps) <= 2.0; // one symbol per kSps samples
    const sdsp_hip_timing_plan_info info = bank.info();
    std::printf("timing_bank<%s>: %llu channels, L %u, T %u, block %u, waves %u, lds %u, kernel %s, %.1f symbols per channel from %llu "
                "samples: %s\n",
                sizeof(real_t) == 8 ? "double" : "float", static_cast<unsigned long long>(info.channels), info.phases, info.taps, info.block,
                info.waves, info.lds_bytes, info.kernel, per_channel, static_cast<unsigned long long>(total),
                ok ? "equal to the program's loop" : "DIFFERS from the program's loop");
    return ok && fresh && rate && info.phases == kPhases && info.taps == kTaps && info.step0 == step0 ? 0 : 1;
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
