// sdsp::cfar2d_plan (include/sdsp/cfar2d.h) on 3 maps of 16 x 33 cells: thresholds, decisions and the ordered hit lists through the host
// entry, in float and in double, both edge modes, with and without the peak rule, in both kernel variants, against the contract's sums
// written as direct loops here (the same additions in the same order, so the comparison is on bits).  Exit 0 = pass, 1 = mismatch,
// 3 = no usable device (the library has no CPU fallback).
#include <sdsp/cfar2d.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <random>
#include <vector>

namespace
{
constexpr std::uint64_t kMaps = 3;
constexpr std::uint32_t kD = 16, kR = 33;
constexpr sdsp::cfar2d_window kWin{ 2, 1, 4, 1 };
constexpr double kAlpha = 2.75;

template <typename real_t> struct direct {
    std::vector<real_t> thr;
    std::vector<std::uint8_t> det;
    std::vector<std::vector<typename sdsp::cfar2d_plan<real_t>::hit_t>> hits;
};

template <typename real_t> direct<real_t> by_loops(const std::vector<real_t> &p, bool clip, bool peak)
{
    const int Hd = static_cast<int>(kWin.train_d + kWin.guard_d), Gd = static_cast<int>(kWin.guard_d);
    const int Hr = static_cast<int>(kWin.train_r + kWin.guard_r), Gr = static_cast<int>(kWin.guard_r);
    const int D = static_cast<int>(kD), R = static_cast<int>(kR);
    direct<real_t> out;
    out.thr.resize(p.size());
    out.det.resize(p.size());
    out.hits.resize(kMaps);
    for (std::size_t m = 0; m < kMaps; m++) {
        const real_t *map = p.data() + m * kD * kR;
        auto at = [&](int d, int r) { return (r >= 0 && r < R) ? map[((d % D + D) % D) * R + r] : real_t(0); };
        for (int d = 0; d < D; d++)
            for (int r = 0; r < R; r++) {
                real_t top = 0, band = 0, bottom = 0;
                for (int i = -Hd; i <= Hd; i++) {
                    real_t lag = 0, mid = 0, lead = 0;
                    for (int j = -Hr; j < -Gr; j++)
                        lag = lag + at(d + i, r + j);
                    for (int j = -Gr; j <= Gr; j++)
                        mid = mid + at(d + i, r + j);
                    for (int j = Gr + 1; j <= Hr; j++)
                        lead = lead + at(d + i, r + j);
                    const real_t side = lag + lead, lm = lag + mid, full = lm + lead;
                    if (i < -Gd)
                        top = top + full;
                    else if (i <= Gd)
                        band = band + side;
                    else
                        bottom = bottom + full;
                }
                auto inside = [&](int h) { return std::min(r + h, R - 1) - std::max(r - h, 0) + 1; };
                const int n = (2 * Hd + 1) * inside(Hr) - (2 * Gd + 1) * inside(Gr);
                const real_t c = static_cast<real_t>(kAlpha / static_cast<double>(n)), tb = top + band, T = tb + bottom;
                real_t th = T * c;
                if (!clip && (r < Hr || r >= R - Hr))
                    th = std::numeric_limits<real_t>::infinity();
                const real_t pv = at(d, r);
                bool hit = pv > th;
                if (hit && peak)
                    for (int i = -1; i <= 1; i++)
                        for (int j = -1; j <= 1; j++) {
                            if ((i == 0 && j == 0) || r + j < 0 || r + j >= R)
                                continue;
                            const bool before = i < 0 || (i == 0 && j < 0);
                            hit = hit && (before ? pv > at(d + i, r + j) : pv >= at(d + i, r + j));
                        }
                const std::size_t idx = (m * kD + static_cast<std::size_t>(d)) * kR + static_cast<std::size_t>(r);
                out.thr[idx] = th;
                out.det[idx] = hit ? 1 : 0;
                if (hit) {
                    typename sdsp::cfar2d_plan<real_t>::hit_t h{};
                    h.doppler = static_cast<std::uint32_t>(d);
                    h.range = static_cast<std::uint32_t>(r);
                    h.power = pv;
                    h.thr = th;
                    out.hits[m].push_back(h);
                }
            }
    }
    return out;
}

template <typename real_t> int run()
{
    using hit_t = typename sdsp::cfar2d_plan<real_t>::hit_t;
    static_assert(sizeof(hit_t) == 8 + 2 * sizeof(real_t), "the record has no padding");
    std::mt19937 gen(17);
    std::exponential_distribution<double> noise(1.0);
    std::vector<real_t> p(static_cast<std::size_t>(kMaps * kD * kR));
    for (real_t &v : p)
        v = static_cast<real_t>(noise(gen));
    p[(1 * kD + 15) * kR + 20] = real_t(40); // a target next to the Doppler wrap
    p[(1 * kD + 0) * kR + 20] = real_t(40);  // and its equal on the other side: the peak rule keeps one
    int bad = 0;
    std::size_t listed = 0;
    sdsp_hip_cfar2d_plan_info info{};
    for (int clip = 0; clip < 2; clip++)
        for (int peak = 0; peak < 2; peak++) {
            const direct<real_t> want = by_loops<real_t>(p, clip != 0, peak != 0);
            sdsp::cfar2d_plan<real_t> plan(kD, kR, kMaps, kWin, kAlpha, clip ? sdsp::cfar2d_edge::clip : sdsp::cfar2d_edge::mark, peak != 0);
            for (int variant = 0; variant < 2; variant++) {
                plan.set_variant(variant);
                if (variant == 0)
                    info = plan.info();
                std::size_t most = 0;
                for (const auto &h : want.hits)
                    most = std::max(most, h.size());
                for (std::uint64_t cap : { static_cast<std::uint64_t>(most), static_cast<std::uint64_t>(most ? most - 1 : 0), std::uint64_t(0) }) {
                    std::vector<real_t> thr(p.size(), real_t(-1));
                    std::vector<std::uint8_t> det(p.size(), 9);
                    std::vector<hit_t> hits(static_cast<std::size_t>(kMaps * cap) + 1);
                    std::vector<std::uint32_t> counts(kMaps, 77);
                    plan.process_host(p.data(), thr.data(), det.data(), hits.data(), counts.data(), cap, kMaps);
                    bad += std::memcmp(thr.data(), want.thr.data(), thr.size() * sizeof(real_t)) != 0;
                    bad += det != want.det;
                    for (std::size_t m = 0; m < kMaps; m++) {
                        const std::size_t n = std::min<std::size_t>(want.hits[m].size(), static_cast<std::size_t>(cap));
                        bad += counts[m] != want.hits[m].size();
                        bad += n && std::memcmp(hits.data() + m * cap, want.hits[m].data(), n * sizeof(hit_t)) != 0;
                        listed += n;
                    }
                }
                // the list alone
                std::vector<hit_t> hits(static_cast<std::size_t>(kMaps * most) + 1);
                std::vector<std::uint32_t> counts(kMaps, 77);
                plan.process_host(p.data(), nullptr, nullptr, hits.data(), counts.data(), most, kMaps);
                for (std::size_t m = 0; m < kMaps; m++) {
                    const std::size_t n = want.hits[m].size();
                    bad += counts[m] != n || (n && std::memcmp(hits.data() + m * most, want.hits[m].data(), n * sizeof(hit_t)) != 0);
                }
            }
        }
    const std::uint32_t Hd = kWin.train_d + kWin.guard_d, Hr = kWin.train_r + kWin.guard_r;
    const bool shape_ok = info.D == kD && info.R == kR && info.max_maps == kMaps
                          && info.cells == (2 * Hd + 1) * (2 * Hr + 1) - (2 * kWin.guard_d + 1) * (2 * kWin.guard_r + 1) && listed > 0;
    const bool ok = bad == 0 && shape_ok;
    std::printf("cfar2d_plan<%s>: %llu x %u x %u, kernel %s, tile %u x %u, %u threads, lds %u, %zu records compared: %s\n",
                sizeof(real_t) == 8 ? "double" : "float", static_cast<unsigned long long>(kMaps), kD, kR, info.kernel, info.tile_rows,
                info.tile_cols, info.threads, info.lds_bytes, listed, ok ? "bit for bit" : "MISMATCH");
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
