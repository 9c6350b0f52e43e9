// sdsp/timing.h -- symbol-timing recovery bank for the MI355X engine (sdsp_hip_timing_*).
//
// `channels` independent second-order timing loops on interleaved I/Q rows: process() interpolates every row with the bank's polyphase
// table at two strobes per symbol, measures the timing error on the symbol strobes with the bank's detector (Gardner or zero-crossing)
// and steers the step through a proportional-plus-integral loop filter whose gains alpha and beta are arguments of the call; it writes
// the symbol strobes y, optionally the detector output err and the tracked period offset, and each channel's number of symbols, which
// depends on the data.  Mirrors sdsp::pll_bank (sdsp/pll.h): RAII plan and device-resident state, process() on device pointers,
// process_host() for host buffers.  period() and time() copy the integrators and the Q32.32 stream times out of the state (its first
// array is the times; the layout is in sdsp_hip.h).  No reference counterpart: pinned to tests/timing_ref.py.  There is no CPU path.
#ifndef SDSP_MI355X_TIMING_H
#define SDSP_MI355X_TIMING_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <typename real_t = float> class timing_bank {
public:
    // mode: SDSP_HIP_TIMING_GARDNER, SDSP_HIP_TIMING_ZC_QPSK or SDSP_HIP_TIMING_ZC_BPSK; sps: nominal samples per symbol in [2, 128];
    // h: phases x taps prototype values (sdsp_hip_timing_design, or any interpolating filter in the sdsp_hip_arb_tables layout);
    // max_dev in (0, 0.5] samples per half symbol bounds the integrator
    timing_bank(std::uint64_t channels, int mode, double sps, std::uint32_t phases, const std::vector<double> &h, double max_dev = 0.5,
                int device = 0)
        : m_channels(channels), m_device(device)
    {
        if (phases == 0 || h.empty() || h.size() % phases)
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: h must hold phases x taps values");
        detail::check(sdsp_hip_timing_step(sps, &m_step0));
        sdsp_hip_timing_plan *plan = nullptr;
        detail::check(sdsp_hip_timing_plan_create(&plan, channels, detail::precision_of<real_t>::value, mode, phases,
                                                  static_cast<std::uint32_t>(h.size() / phases), h.data(), m_step0, max_dev, device));
        m_plan.reset(plan);
    }
    timing_bank(const timing_bank &) = delete;
    timing_bank &operator=(const timing_bank &) = delete;

    // a fresh loop at t = 0 preceded by zeros
    void reset()
    {
        if (m_state)
            zero_state();
    }

    // the capacity a row of y, err or period needs for `samples` inputs
    std::uint64_t max_out(std::uint64_t samples) const
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_timing_max_out(m_plan.get(), samples, &n));
        return n;
    }

    // device pointers (channel-major rows: x and y of I/Q pairs, err and period of reals, strides in elements; err and period may be
    // null; counts: channels words), asynchronous on `stream`; continues every channel's loop
    void process(const real_t *device_x, std::uint64_t x_stride, real_t *device_y, std::uint64_t y_stride, real_t *device_err,
                 std::uint64_t err_stride, real_t *device_period, std::uint64_t period_stride, std::uint32_t *device_counts,
                 std::uint64_t samples, double alpha, double beta, void *stream = nullptr)
    {
        ensure_state();
        detail::check(sdsp_hip_timing_process(m_plan.get(), device_x, x_stride, device_y, y_stride, device_err, err_stride, device_period,
                                              period_stride, device_counts, samples, alpha, beta, m_state.get(), stream));
    }
    // host pointers: x holds channels x samples elements (interleaved re, im), y, err and period channels x max_out(samples); err and
    // period may be null.  Returns the counts: row c holds counts[c] symbols, the rest of it is left as it was
    std::vector<std::uint32_t> process_host(const real_t *host_x, real_t *host_y, real_t *host_err, real_t *host_period,
                                            std::uint64_t samples, double alpha, double beta)
    {
        ensure_state();
        std::vector<std::uint32_t> counts(static_cast<std::size_t>(m_channels), 0u);
        if (samples == 0)
            return counts;
        const std::uint64_t cap = max_out(samples);
        const std::size_t in_bytes = static_cast<std::size_t>(m_channels * samples) * 2 * sizeof(real_t);
        const std::size_t reals = static_cast<std::size_t>(m_channels * cap) * sizeof(real_t);
        detail::check(host_y ? SDSP_HIP_OK : SDSP_HIP_ERR_INVALID_ARG);
        // y, err and period go in as well as out: what lies behind a row's count keeps the caller's values
        const detail::stage_item items[] = { { host_x, nullptr, in_bytes },
                                             { host_y, host_y, 2 * reals },
                                             { host_err, host_err, reals },
                                             { host_period, host_period, reals },
                                             { nullptr, counts.data(), counts.size() * sizeof(std::uint32_t) } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_timing_process(m_plan.get(), dev[0], samples, dev[1], cap, dev[2], cap, dev[3], cap,
                                           static_cast<std::uint32_t *>(dev[4]), samples, alpha, beta, m_state.get(), nullptr);
        });
        return counts;
    }
    // the integrators, copied from the device state: the tracked offsets of the half-symbol period, in samples
    std::vector<real_t> period()
    {
        ensure_state();
        std::vector<real_t> f(static_cast<std::size_t>(m_channels));
        m_state.download(f.data(), f.size() * sizeof(real_t), integ_offset());
        return f;
    }
    // the Q32.32 stream times, copied from the device state
    std::vector<std::uint64_t> time()
    {
        ensure_state();
        std::vector<std::uint64_t> t(static_cast<std::size_t>(m_channels));
        m_state.download(t.data(), t.size() * sizeof(std::uint64_t));
        return t;
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    std::uint64_t step0() const noexcept { return m_step0; }
    void set_variant(int variant) { detail::check(sdsp_hip_timing_plan_set_variant(m_plan.get(), variant)); }
    sdsp_hip_timing_plan_info info() const
    {
        sdsp_hip_timing_plan_info i{};
        detail::check(sdsp_hip_timing_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    static std::size_t up8(std::size_t v) noexcept { return (v + 7) / 8 * 8; }
    // t (channels uint64), ps and ym (channels complex values each), then integ
    std::size_t integ_offset() const noexcept
    {
        const std::size_t ch = static_cast<std::size_t>(m_channels);
        return ch * 8 + 2 * up8(ch * 2 * sizeof(real_t));
    }
    void zero_state()
    {
        std::uint64_t bytes = 0;
        detail::check(sdsp_hip_timing_state_bytes(m_plan.get(), &bytes));
        if (!m_state)
            m_state.alloc(static_cast<std::size_t>(bytes), m_device);
        m_state.fill<unsigned char>(static_cast<std::size_t>(bytes), 0);
    }
    void ensure_state()
    {
        if (!m_state)
            zero_state();
    }

    std::uint64_t m_channels;
    int m_device;
    std::uint64_t m_step0{ 0 };
    detail::plan_ptr<sdsp_hip_timing_plan, sdsp_hip_timing_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_TIMING_H
