// sdsp/rank_filter.h -- rank-order filter bank (running median, minimum, maximum, any rank) for the MI355X engine (sdsp_hip_rank_*,
// DESIGN.md section 5.26).
//
// `channels` independent real rows: process() writes, for every sample, the element of rank r (counted from 0, ascending, in IEEE 754
// totalOrder) of the last `window` samples of its row, continuing from the bank's history.  Every output is one of the inputs, bit for
// bit.  Mirrors sdsp::lms_bank (sdsp/lms.h): RAII plan and device-resident state, process() on device pointers, process_host() for
// host buffers.  The state is the x history, [channel][window - 1], newest first.  No reference counterpart: pinned to a sorting loop and
// to scipy.signal.medfilt.  There is no CPU path.
#ifndef SDSP_MI355X_RANK_FILTER_H
#define SDSP_MI355X_RANK_FILTER_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <typename real_t = float> class rank_filter_bank {
public:
    // rank: 0 = the running minimum, window - 1 = the running maximum, (window - 1) / 2 with an odd window = the running median
    rank_filter_bank(std::uint64_t channels, std::uint32_t window, std::uint32_t rank, int device = 0)
        : m_channels(channels), m_window(window), m_rank(rank), m_device(device)
    {
        sdsp_hip_rank_plan *plan = nullptr;
        detail::check(sdsp_hip_rank_plan_create(&plan, channels, window, rank, detail::precision_of<real_t>::value, device));
        m_plan.reset(plan);
    }
    // the running median of an odd window
    static std::uint32_t median_rank(std::uint32_t window) noexcept { return (window - 1u) / 2u; }
    rank_filter_bank(const rank_filter_bank &) = delete;
    rank_filter_bank &operator=(const rank_filter_bank &) = delete;

    // zero history
    void reset()
    {
        if (m_state)
            zero_state();
    }

    // device pointers (channel-major rows, strides in elements; y may not overlap x), asynchronous on `stream`; continues every row's
    // stream
    void process(const real_t *device_x, std::uint64_t x_stride, real_t *device_y, std::uint64_t y_stride, std::uint64_t samples,
                 void *stream = nullptr)
    {
        ensure_state();
        detail::check(sdsp_hip_rank_process(m_plan.get(), device_x, x_stride, device_y, y_stride, samples, m_state.get(), stream));
    }
    // host pointers: contiguous channels x samples elements each
    void process_host(const real_t *host_x, real_t *host_y, std::uint64_t samples)
    {
        ensure_state();
        if (samples == 0)
            return;
        const std::size_t bytes = static_cast<std::size_t>(m_channels * samples) * sizeof(real_t);
        detail::host_stage(m_device, { { host_x, nullptr, bytes }, { nullptr, host_y, bytes } }, [&](void *const *dev) {
            return sdsp_hip_rank_process(m_plan.get(), dev[0], samples, dev[1], samples, samples, m_state.get(), nullptr);
        });
    }
    // the x history, [channel][window - 1], newest first, copied from the device state
    std::vector<real_t> history()
    {
        ensure_state();
        std::vector<real_t> h(history_elems());
        if (!h.empty())
            m_state.download(h.data(), h.size() * sizeof(real_t));
        return h;
    }
    // ... copied into it
    void set_history(const std::vector<real_t> &h)
    {
        if (h.size() != history_elems())
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: history must be channels x (window - 1)");
        ensure_state();
        if (!h.empty())
            m_state.upload(h.data(), h.size() * sizeof(real_t));
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    std::uint32_t window() const noexcept { return m_window; }
    std::uint32_t rank() const noexcept { return m_rank; }
    void set_variant(int variant) { detail::check(sdsp_hip_rank_plan_set_variant(m_plan.get(), variant)); }
    void set_run(std::uint64_t run) { detail::check(sdsp_hip_rank_plan_set_run(m_plan.get(), run)); }
    sdsp_hip_rank_plan_info info() const
    {
        sdsp_hip_rank_plan_info i{};
        detail::check(sdsp_hip_rank_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t history_elems() const noexcept { return static_cast<std::size_t>(m_channels) * (m_window - 1u); }
    void zero_state()
    {
        const std::size_t bytes = history_elems() * sizeof(real_t);
        if (bytes == 0)
            return;
        if (!m_state)
            m_state.alloc(bytes, m_device);
        m_state.fill<unsigned char>(bytes, 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint64_t m_channels;
    std::uint32_t m_window, m_rank;
    int m_device;
    detail::plan_ptr<sdsp_hip_rank_plan, sdsp_hip_rank_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_RANK_FILTER_H
