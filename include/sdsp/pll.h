// sdsp/pll.h -- carrier-recovery PLL / Costas loop bank for the MI355X engine (sdsp_hip_pll_*).
//
// `channels` independent second-order loops on interleaved I/Q rows: process() de-rotates every row with its own 32-bit numerically
// controlled oscillator, measures the phase error with the bank's detector and steers the oscillator through a proportional-plus-
// integral loop filter whose gains alpha and beta are arguments of the call; it writes the de-rotated rows y, the detector output err
// and the tracked frequency offset freq (cycles per sample), any of which may be left out.  Mirrors sdsp::lms_bank (sdsp/lms.h): RAII
// plan and device-resident state, process() on device pointers, process_host() for host buffers.  The state holds the integrators
// (channels reals), then the phase words (channels uint32); freq(), phase(), set_freq() and set_phase() copy them.  No reference
// counterpart: pinned to tests/pll_ref.py.  There is no CPU path.
#ifndef SDSP_MI355X_PLL_H
#define SDSP_MI355X_PLL_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <typename real_t = float> class pll_bank {
public:
    // mode: SDSP_HIP_PLL_CROSS, SDSP_HIP_PLL_BPSK or SDSP_HIP_PLL_QPSK; fcw0: the centre-frequency words of sdsp_hip_ddc_phase_word, one
    // per channel; max_dev in (0, 0.5] cycles per sample bounds the integrator
    pll_bank(std::uint64_t channels, int mode, const std::vector<std::uint32_t> &fcw0, double max_dev = 0.5, int device = 0)
        : m_channels(channels), m_device(device)
    {
        create(mode, fcw0.data(), fcw0.size(), max_dev);
    }
    // one centre-frequency word shared by every channel
    pll_bank(std::uint64_t channels, int mode, std::uint32_t fcw0, double max_dev = 0.5, int device = 0)
        : m_channels(channels), m_device(device)
    {
        create(mode, &fcw0, 1, max_dev);
    }
    pll_bank(const pll_bank &) = delete;
    pll_bank &operator=(const pll_bank &) = delete;

    // zero integrators, phase 0
    void reset()
    {
        if (m_state)
            zero_state();
    }

    // device pointers (channel-major rows: x and y of I/Q pairs, err and freq of reals, strides in elements; y, err and freq may be null,
    // y may be x), asynchronous on `stream`; continues every channel's loop
    void process(const real_t *device_x, std::uint64_t x_stride, real_t *device_y, std::uint64_t y_stride, real_t *device_err,
                 std::uint64_t err_stride, real_t *device_freq, std::uint64_t freq_stride, std::uint64_t samples, double alpha, double beta,
                 void *stream = nullptr)
    {
        ensure_state();
        detail::check(sdsp_hip_pll_process(m_plan.get(), device_x, x_stride, device_y, y_stride, device_err, err_stride, device_freq,
                                           freq_stride, samples, alpha, beta, m_state.get(), stream));
    }
    // host pointers: contiguous channels x samples elements each (x and y: interleaved re, im); y, err and freq may be null
    void process_host(const real_t *host_x, real_t *host_y, real_t *host_err, real_t *host_freq, std::uint64_t samples, double alpha,
                      double beta)
    {
        ensure_state();
        if (samples == 0)
            return;
        const std::size_t reals = static_cast<std::size_t>(m_channels * samples) * sizeof(real_t);
        const detail::stage_item items[] = { { host_x, nullptr, 2 * reals }, { nullptr, host_y, 2 * reals }, { nullptr, host_err, reals },
                                             { nullptr, host_freq, reals } };
        detail::host_stage(m_device, items, [&](void *const *dev) {
            return sdsp_hip_pll_process(m_plan.get(), dev[0], samples, dev[1], samples, dev[2], samples, dev[3], samples, samples, alpha,
                                        beta, m_state.get(), nullptr);
        });
    }
    // the integrators, copied from the device state: the tracked frequency offsets in cycles per sample
    std::vector<real_t> freq()
    {
        ensure_state();
        std::vector<real_t> f(static_cast<std::size_t>(m_channels));
        m_state.download(f.data(), f.size() * sizeof(real_t));
        return f;
    }
    // the phase words, copied from the device state
    std::vector<std::uint32_t> phase()
    {
        ensure_state();
        std::vector<std::uint32_t> t(static_cast<std::size_t>(m_channels));
        m_state.download(t.data(), t.size() * sizeof(std::uint32_t), words());
        return t;
    }
    // ... copied into it; the other half of the state stays
    void set_freq(const std::vector<real_t> &f)
    {
        if (f.size() != m_channels)
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: freq must hold one value per channel");
        ensure_state();
        m_state.upload(f.data(), f.size() * sizeof(real_t));
    }
    void set_phase(const std::vector<std::uint32_t> &t)
    {
        if (t.size() != m_channels)
            throw hip_error(SDSP_HIP_ERR_INVALID_SIZE, "sdsp_hip: phase must hold one word per channel");
        ensure_state();
        m_state.upload(t.data(), t.size() * sizeof(std::uint32_t), words());
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    void set_variant(int variant) { detail::check(sdsp_hip_pll_plan_set_variant(m_plan.get(), variant)); }
    sdsp_hip_pll_plan_info info() const
    {
        sdsp_hip_pll_plan_info i{};
        detail::check(sdsp_hip_pll_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    void create(int mode, const std::uint32_t *fcw0, std::size_t n_fcw0, double max_dev)
    {
        sdsp_hip_pll_plan *plan = nullptr;
        detail::check(sdsp_hip_pll_plan_create(&plan, m_channels, detail::precision_of<real_t>::value, mode, fcw0, n_fcw0, max_dev,
                                               m_device));
        m_plan.reset(plan);
    }
    // byte offset of the phase words in the state, behind the integrators
    std::size_t words() const noexcept { return static_cast<std::size_t>(m_channels) * sizeof(real_t); }
    void zero_state()
    {
        std::uint64_t bytes = 0;
        detail::check(sdsp_hip_pll_state_bytes(m_plan.get(), &bytes));
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
    detail::plan_ptr<sdsp_hip_pll_plan, sdsp_hip_pll_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_PLL_H
