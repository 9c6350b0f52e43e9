// sdsp/cfar.h -- constant-false-alarm-rate detector bank (CA, GO, SO and OS thresholds) for the MI355X engine (sdsp_hip_cfar_*,
// DESIGN.md section 5.27).
//
// `channels` independent rows of power (or of interleaved I/Q, which becomes power re re + im im on the way in): process() writes, for
// every input sample n, a threshold made from the 2 `train` training cells around the cell under test p[n - (train + guard)] and the
// decision cell > threshold as one byte, continuing from the bank's history.  The bank is causal with a delay of train + guard samples.
// Mirrors sdsp::rank_filter_bank (sdsp/rank_filter.h): RAII plan and device-resident state, process() on device pointers,
// process_host() for host buffers.  The state is the x history, [channel][window - 1] elements of the input's kind, newest first.  No
// reference counterpart: pinned to a numpy loop with the contract's order of operations.  There is no CPU path.
#ifndef SDSP_MI355X_CFAR_H
#define SDSP_MI355X_CFAR_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
enum class cfar_mode : int { ca = SDSP_HIP_CFAR_CA, go = SDSP_HIP_CFAR_GO, so = SDSP_HIP_CFAR_SO, os = SDSP_HIP_CFAR_OS };
enum class cfar_input : int { power = SDSP_HIP_CFAR_POWER, iq = SDSP_HIP_CFAR_IQ };

template <typename real_t = float> class cfar_bank {
public:
    // rank: OS only, 0 <= rank < 2 train (default_rank(train) is three quarters of the way up)
    cfar_bank(std::uint64_t channels, std::uint32_t train, std::uint32_t guard, cfar_mode mode, double alpha, std::uint32_t rank = 0,
              cfar_input input = cfar_input::power, int device = 0)
        : m_channels(channels), m_train(train), m_guard(guard), m_iq(input == cfar_input::iq), m_device(device)
    {
        sdsp_hip_cfar_desc d{};
        d.train = train;
        d.guard = guard;
        d.mode = static_cast<int>(mode);
        d.rank = rank;
        d.input = static_cast<int>(input);
        d.alpha = alpha;
        sdsp_hip_cfar_plan *plan = nullptr;
        detail::check(sdsp_hip_cfar_plan_create(&plan, channels, &d, detail::precision_of<real_t>::value, device));
        m_plan.reset(plan);
    }
    static std::uint32_t default_rank(std::uint32_t train) noexcept { return (3u * 2u * train) / 4u; }
    cfar_bank(const cfar_bank &) = delete;
    cfar_bank &operator=(const cfar_bank &) = delete;

    // zero history
    void reset()
    {
        if (m_state)
            zero_state();
    }

    // device pointers (channel-major rows, strides in elements of each row's kind; thr or det may be null, not both; outputs may not
    // overlap x or each other), asynchronous on `stream`; continues every row's stream
    void process(const real_t *device_x, std::uint64_t x_stride, real_t *device_thr, std::uint64_t thr_stride, std::uint8_t *device_det,
                 std::uint64_t det_stride, std::uint64_t samples, void *stream = nullptr)
    {
        ensure_state();
        detail::check(sdsp_hip_cfar_process(m_plan.get(), device_x, x_stride, device_thr, thr_stride, device_det, det_stride, samples,
                                            m_state.get(), stream));
    }
    // host pointers: contiguous channels x samples elements each (x: one real per element for power, an interleaved pair for I/Q);
    // thr or det may be null, not both
    void process_host(const real_t *host_x, real_t *host_thr, std::uint8_t *host_det, std::uint64_t samples)
    {
        ensure_state();
        if (samples == 0)
            return;
        const std::size_t n = static_cast<std::size_t>(m_channels * samples);
        const detail::stage_item items[] = { { host_x, nullptr, n * sizeof(real_t) * reals_per_element() },
                                             { nullptr, host_thr, n * sizeof(real_t) },
                                             { nullptr, host_det, n } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_cfar_process(m_plan.get(), dev[0], samples, dev[1], samples, static_cast<std::uint8_t *>(dev[2]), samples,
                                         samples, m_state.get(), nullptr);
        });
    }
    // the x history, [channel][window - 1] elements (I/Q: interleaved pairs), newest first, copied from the device state
    std::vector<real_t> history()
    {
        ensure_state();
        std::vector<real_t> h(history_reals());
        if (!h.empty())
            m_state.download(h.data(), h.size() * sizeof(real_t));
        return h;
    }
    // ... copied into it
    void set_history(const std::vector<real_t> &h)
    {
        if (h.size() != history_reals())
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: history must be channels x (window - 1) elements");
        ensure_state();
        if (!h.empty())
            m_state.upload(h.data(), h.size() * sizeof(real_t));
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    std::uint32_t train() const noexcept { return m_train; }
    std::uint32_t guard() const noexcept { return m_guard; }
    std::uint32_t delay() const noexcept { return m_train + m_guard; }
    std::uint32_t window() const noexcept { return 2u * (m_train + m_guard) + 1u; }
    void set_alpha(double alpha) { detail::check(sdsp_hip_cfar_plan_set_alpha(m_plan.get(), alpha)); }
    void set_variant(int variant) { detail::check(sdsp_hip_cfar_plan_set_variant(m_plan.get(), variant)); }
    void set_run(std::uint64_t run) { detail::check(sdsp_hip_cfar_plan_set_run(m_plan.get(), run)); }
    sdsp_hip_cfar_plan_info info() const
    {
        sdsp_hip_cfar_plan_info i{};
        detail::check(sdsp_hip_cfar_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    std::size_t reals_per_element() const noexcept { return m_iq ? 2u : 1u; }
    std::size_t history_reals() const noexcept { return static_cast<std::size_t>(m_channels) * (window() - 1u) * reals_per_element(); }
    void zero_state()
    {
        const std::size_t bytes = history_reals() * sizeof(real_t);
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
    std::uint32_t m_train, m_guard;
    bool m_iq;
    int m_device;
    detail::plan_ptr<sdsp_hip_cfar_plan, sdsp_hip_cfar_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_CFAR_H
