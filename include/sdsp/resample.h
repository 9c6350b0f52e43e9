// sdsp/resample.h -- polyphase FIR resampler bank for the MI355X engine (sdsp_hip_resample_*).
//
// Up by `up`, filter with n_taps coefficients, down by `down`, out of place, for a bank of channels on the device.  Mirrors
// sdsp::fir_bank (sdsp/fir.h): RAII plan and device-resident per-channel history, process() on device pointers, process_host()
// for host buffers.  A call of S samples per channel (S a multiple of down / gcd(up, down)) writes S * up / down outputs.  Like
// the FIR bank this has no reference counterpart and is pinned to scipy.signal.upfirdn.  There is no CPU path.
#ifndef SDSP_MI355X_RESAMPLE_H
#define SDSP_MI355X_RESAMPLE_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <size_t n_taps, std::uint32_t up, std::uint32_t down, typename real_t = float> class fir_resampler_bank {
    static_assert(n_taps >= 1 && n_taps <= SDSP_HIP_FIR_MAX_TAPS, "a resampler takes 1 .. SDSP_HIP_FIR_MAX_TAPS taps");
    static_assert(up >= 1 && up <= SDSP_HIP_RESAMPLE_MAX_FACTOR, "up must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");
    static_assert(down >= 1 && down <= SDSP_HIP_RESAMPLE_MAX_FACTOR, "down must be in [1, SDSP_HIP_RESAMPLE_MAX_FACTOR]");

public:
    static constexpr size_t hist = (n_taps - 1) / up; // history per channel, newest first

    explicit fir_resampler_bank(std::uint64_t channels, int device = 0) : m_channels(channels), m_device(device) {}
    fir_resampler_bank(const fir_resampler_bank &) = delete;
    fir_resampler_bank &operator=(const fir_resampler_bank &) = delete;

    void set_coeff(const std::array<double, n_taps> &h)
    {
        m_coeff = h;
        m_plan.reset();
    }
    // Hamming low-pass at 1 / (2 max(up, down)) of the intermediate rate, gain up (sdsp_hip_resample_design)
    void set_antialias_coeff()
    {
        detail::check(sdsp_hip_resample_design(static_cast<std::uint32_t>(n_taps), up, down, m_coeff.data()));
        m_plan.reset();
    }
    void preload_filter(double value) { fill_state(static_cast<real_t>(value)); }
    void reset()
    {
        if (m_state)
            fill_state(real_t(0));
    }

    // outputs of a call of `samples` inputs per channel; throws unless samples is a multiple of down / gcd(up, down)
    static std::uint64_t out_samples(std::uint64_t samples)
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_resample_out_samples(up, down, samples, &n));
        return n;
    }

    // device pointers, channel-major, asynchronous on `stream`; continues every channel's stream
    void process(const real_t *device_in, std::uint64_t in_stride, real_t *device_out, std::uint64_t out_stride, std::uint64_t samples,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_resample_process(m_plan.get(), device_in, in_stride, device_out, out_stride, m_channels, samples,
                                                m_state.get(), stream));
    }
    // host pointers: in = channels x samples, out = channels x out_samples(samples), both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t outs = out_samples(samples);
        const size_t in_bytes = static_cast<size_t>(m_channels * samples) * sizeof(real_t);
        const size_t out_bytes = static_cast<size_t>(m_channels * outs) * sizeof(real_t);
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_resample_process(m_plan.get(), dev[0], samples, dev[1], outs, m_channels, samples, m_state.get(), nullptr);
        });
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    const std::array<double, n_taps> &coeff() const { return m_coeff; }
    sdsp_hip_resample_plan_info info()
    {
        ensure_plan();
        sdsp_hip_resample_plan_info i{};
        detail::check(sdsp_hip_resample_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    static constexpr size_t state_len = hist > 0 ? hist : 1;
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_resample_plan *plan = nullptr;
        detail::check(sdsp_hip_resample_plan_create(&plan, static_cast<std::uint32_t>(n_taps), m_coeff.data(), up, down,
                                                    detail::precision_of<real_t>::value, m_device));
        m_plan.reset(plan);
    }
    void fill_state(real_t v)
    {
        if (!m_state)
            m_state.alloc(state_len * m_channels * sizeof(real_t), m_device);
        m_state.fill(state_len * m_channels, v);
    }
    void ensure_state()
    {
        if (!m_state)
            fill_state(real_t(0));
    }

    std::uint64_t m_channels;
    int m_device;
    std::array<double, n_taps> m_coeff{};
    detail::plan_ptr<sdsp_hip_resample_plan, sdsp_hip_resample_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_RESAMPLE_H
