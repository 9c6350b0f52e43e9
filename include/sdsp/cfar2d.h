// sdsp/cfar2d.h -- 2-D cell-averaging CFAR over range-Doppler maps for the MI355X engine (sdsp_hip_cfar2d_*).
//
// `maps` compact maps of D rows (Doppler, which wraps) by R columns (range, which has edges) of real powers: the POWER output of
// sdsp::fft_cols_plan with n = D, width = R.  A plan writes a threshold map, a byte map of decisions and, per map, the ordered list of
// detections (doppler, range, power, thr); each output is optional.  The bits are the contract's in front of
// sdsp_hip_cfar2d_plan_create.  Mirrors sdsp::cfar_bank's plan handling (sdsp/cfar.h): an RAII plan, process() on device pointers,
// process_host() for host buffers through detail::host_stage, info().  There is no CPU path.
#ifndef SDSP_MI355X_CFAR2D_H
#define SDSP_MI355X_CFAR2D_H

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
enum class cfar2d_edge : int { mark = SDSP_HIP_CFAR2D_EDGE_MARK, clip = SDSP_HIP_CFAR2D_EDGE_CLIP };

struct cfar2d_window {
    std::uint32_t train_d, guard_d, train_r, guard_r;
};

// the constant-false-alarm table c(r) = pfa^(-1 / n(r)) - 1 of R doubles (sdsp_hip_cfar2d_scale)
inline std::vector<double> cfar2d_scale(std::uint32_t D, std::uint32_t R, const cfar2d_window &w, double pfa)
{
    sdsp_hip_cfar2d_desc d{};
    d.train_d = w.train_d;
    d.guard_d = w.guard_d;
    d.train_r = w.train_r;
    d.guard_r = w.guard_r;
    d.edge = SDSP_HIP_CFAR2D_EDGE_CLIP;
    std::vector<double> c(R);
    detail::check(sdsp_hip_cfar2d_scale(D, R, &d, pfa, c.data()));
    return c;
}

template <typename real_t = float> class cfar2d_plan {
public:
    using hit_t = typename std::conditional<sizeof(real_t) == 8, sdsp_hip_cfar2d_hit_f64, sdsp_hip_cfar2d_hit_f32>::type;

    // c(r) = alpha / n(r)
    cfar2d_plan(std::uint32_t D, std::uint32_t R, std::uint64_t max_maps, const cfar2d_window &w, double alpha,
                cfar2d_edge edge = cfar2d_edge::mark, bool peak = false, int device = 0)
        : m_D(D), m_R(R), m_max_maps(max_maps), m_device(device)
    {
        create(w, alpha, nullptr, edge, peak);
    }
    // c(r) from a table of R doubles, such as cfar2d_scale's
    cfar2d_plan(std::uint32_t D, std::uint32_t R, std::uint64_t max_maps, const cfar2d_window &w, const std::vector<double> &scale,
                cfar2d_edge edge = cfar2d_edge::mark, bool peak = false, int device = 0)
        : m_D(D), m_R(R), m_max_maps(max_maps), m_device(device)
    {
        if (scale.size() != R)
            throw hip_error(SDSP_HIP_ERR_INVALID_ARG, "sdsp::cfar2d_plan: the scale table must hold R values");
        create(w, 0.0, scale.data(), edge, peak);
    }
    cfar2d_plan(const cfar2d_plan &) = delete;
    cfar2d_plan &operator=(const cfar2d_plan &) = delete;

    // device pointers to `maps` maps; every output may be null but not all, hits and counts go together (hits: maps x cap records,
    // counts: maps totals); asynchronous on `stream`
    void process(const real_t *device_p, real_t *device_thr, std::uint8_t *device_det, hit_t *device_hits, std::uint32_t *device_counts,
                 std::uint64_t cap, std::uint64_t maps, void *stream = nullptr)
    {
        detail::check(sdsp_hip_cfar2d_process(m_plan.get(), device_p, device_thr, device_det, device_hits, device_counts, cap, maps, stream));
    }
    // host pointers: contiguous maps x D x R elements each, host_hits maps x cap records, host_counts maps totals
    void process_host(const real_t *host_p, real_t *host_thr, std::uint8_t *host_det, hit_t *host_hits, std::uint32_t *host_counts,
                      std::uint64_t cap, std::uint64_t maps)
    {
        if (maps == 0)
            return;
        const std::size_t cells = static_cast<std::size_t>(maps * m_D * m_R);
        hit_t none{}; // a list of cap == 0 has no record to copy back, but the call still needs a pointer
        const bool empty = host_hits && cap == 0;
        const detail::stage_item items[] = { { host_p, nullptr, cells * sizeof(real_t) },
                                             { nullptr, host_thr, cells * sizeof(real_t) },
                                             { nullptr, host_det, cells },
                                             { nullptr, empty ? &none : host_hits, empty ? sizeof(hit_t) : static_cast<std::size_t>(maps * cap) * sizeof(hit_t) },
                                             { nullptr, host_counts, static_cast<std::size_t>(maps) * sizeof(std::uint32_t) } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_cfar2d_process(m_plan.get(), dev[0], dev[1], static_cast<std::uint8_t *>(dev[2]), dev[3],
                                           static_cast<std::uint32_t *>(dev[4]), cap, maps, nullptr);
        });
    }
    std::uint32_t doppler_bins() const noexcept { return m_D; }
    std::uint32_t range_bins() const noexcept { return m_R; }
    std::uint64_t max_maps() const noexcept { return m_max_maps; }
    void set_alpha(double alpha) { detail::check(sdsp_hip_cfar2d_plan_set_alpha(m_plan.get(), alpha)); }
    // 0 = the tiled kernel, 1 = the plain cross-check kernel
    void set_variant(int variant) { detail::check(sdsp_hip_cfar2d_plan_set_variant(m_plan.get(), variant)); }
    std::uint64_t launches(bool thr_or_det, bool hits) const
    {
        std::uint64_t v = 0;
        detail::check(sdsp_hip_cfar2d_plan_launches(m_plan.get(), thr_or_det ? 1 : 0, hits ? 1 : 0, &v));
        return v;
    }
    sdsp_hip_cfar2d_plan_info info() const
    {
        sdsp_hip_cfar2d_plan_info i{};
        detail::check(sdsp_hip_cfar2d_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    void create(const cfar2d_window &w, double alpha, const double *scale, cfar2d_edge edge, bool peak)
    {
        sdsp_hip_cfar2d_desc d{};
        d.train_d = w.train_d;
        d.guard_d = w.guard_d;
        d.train_r = w.train_r;
        d.guard_r = w.guard_r;
        d.edge = static_cast<int>(edge);
        d.peak = peak ? 1 : 0;
        d.alpha = alpha;
        sdsp_hip_cfar2d_plan *plan = nullptr;
        detail::check(sdsp_hip_cfar2d_plan_create(&plan, m_D, m_R, m_max_maps, &d, scale, detail::precision_of<real_t>::value, m_device));
        m_plan.reset(plan);
    }

    std::uint32_t m_D, m_R;
    std::uint64_t m_max_maps;
    int m_device;
    detail::plan_ptr<sdsp_hip_cfar2d_plan, sdsp_hip_cfar2d_plan_destroy> m_plan;
};
} // namespace sdsp

#endif // SDSP_MI355X_CFAR2D_H
