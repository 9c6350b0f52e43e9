// sdsp/welch.h -- streaming Welch power spectral density bank for the MI355X engine (sdsp_hip_welch_*).
//
// scipy.signal.welch for a bank of channels on the device, accumulated across calls: segments of n_fft samples every hop samples,
// detrended, windowed and transformed with the library's real-input FFT, their powers summed in double on the device.  Mirrors
// sdsp::stft_bank (sdsp/stft.h): RAII plan and device-resident per-channel history and sums, process() on device pointers,
// process_host() for host buffers; psd() / psd_host() turn the sums into the estimate.  Pinned to scipy.signal.welch and numpy;
// there is no CPU path.
#ifndef SDSP_MI355X_WELCH_H
#define SDSP_MI355X_WELCH_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <std::uint32_t n_fft, std::uint32_t hop, typename real_t = float> class welch_bank {
    static_assert(n_fft >= 32 && (n_fft & (n_fft - 1)) == 0, "n_fft must be a power of two >= 32");
    static_assert(n_fft <= (sizeof(real_t) == 8 ? 32768u : 65536u), "n_fft must be in the real-input range (f32 .. 65536, f64 .. 32768)");
    static_assert(hop >= 1 && hop <= n_fft, "hop must be in [1, n_fft]");

public:
    static constexpr std::uint32_t bins = n_fft / 2 + 1;
    static constexpr std::uint32_t hist = n_fft - 1; // history per channel, newest first

    explicit welch_bank(std::uint64_t channels, int detrend = SDSP_HIP_DETREND_CONSTANT, int scaling = SDSP_HIP_SCALING_DENSITY,
                        double fs = 1.0, int device = 0)
        : m_channels(channels), m_detrend(detrend), m_scaling(scaling), m_fs(fs), m_device(device)
    {
        set_window(SDSP_HIP_WINDOW_HANN);
    }
    welch_bank(const welch_bank &) = delete;
    welch_bank &operator=(const welch_bank &) = delete;

    void set_window(const std::array<double, n_fft> &w)
    {
        m_window = w;
        m_plan.reset();
    }
    // periodic SDSP_HIP_WINDOW_RECT / HANN / HAMMING / BLACKMAN (sdsp_hip_stft_window)
    void set_window(int kind)
    {
        detail::check(sdsp_hip_stft_window(kind, n_fft, m_window.data()));
        m_plan.reset();
    }
    // a new stream: position, segment count, history and sums back to zero
    void reset()
    {
        m_position = 0;
        m_frames = 0;
        if (m_acc)
            zero_buffers();
    }

    // segments a call of `samples` per channel counts at the bank's position
    std::uint64_t segments(std::uint64_t samples) const
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_welch_frames(n_fft, hop, m_position, samples, &n));
        return n;
    }
    std::uint64_t position() const noexcept { return m_position; }
    std::uint64_t frames() const noexcept { return m_frames; }

    // device pointer, channel-major; asynchronous on `stream`; continues every channel's stream
    void process(const real_t *device_in, std::uint64_t in_stride, std::uint64_t samples, void *stream = nullptr)
    {
        ensure();
        const std::uint64_t f = segments(samples);
        detail::check(sdsp_hip_welch_process(m_plan.get(), device_in, in_stride, m_channels, samples, m_position, m_state.get(), acc(),
                                             bins, stream));
        m_position += samples;
        m_frames += f;
    }
    // host pointer: in = channels x samples, contiguous (synchronous)
    void process_host(const real_t *host_in, std::uint64_t samples)
    {
        ensure();
        if (samples == 0)
            return;
        const std::uint64_t f = segments(samples);
        const size_t in_bytes = static_cast<size_t>(m_channels * samples) * sizeof(real_t);
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes } }, [&](void *const *dev) {
            const int rc = sdsp_hip_welch_process(m_plan.get(), dev[0], samples, m_channels, samples, m_position, m_state.get(), acc(),
                                                  bins, nullptr);
            return rc ? rc : sdsp_hip_device_synchronize(m_device);
        });
        m_position += samples;
        m_frames += f;
    }
    // the estimate from the segments so far: channels rows of bins values, out_stride apart (device pointer, asynchronous)
    void psd(real_t *device_out, std::uint64_t out_stride, void *stream = nullptr)
    {
        ensure();
        detail::check(sdsp_hip_welch_finalize(m_plan.get(), acc(), bins, m_frames, device_out, out_stride, m_channels, stream));
    }
    // host pointer: out = channels x bins, contiguous (synchronous)
    void psd_host(real_t *host_out)
    {
        ensure();
        const size_t out_bytes = static_cast<size_t>(m_channels * bins) * sizeof(real_t);
        detail::host_stage(m_device, { { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_welch_finalize(m_plan.get(), acc(), bins, m_frames, dev[0], bins, m_channels, nullptr);
        });
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    const std::array<double, n_fft> &window() const { return m_window; }
    sdsp_hip_welch_plan_info info()
    {
        ensure();
        sdsp_hip_welch_plan_info i{};
        detail::check(sdsp_hip_welch_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    double *acc() const noexcept { return static_cast<double *>(m_acc.get()); }
    void zero_buffers()
    {
        m_state.fill(static_cast<size_t>(hist * m_channels), real_t(0));
        m_acc.fill(static_cast<size_t>(bins * m_channels), 0.0);
    }
    void ensure()
    {
        if (!m_plan) {
            sdsp_hip_welch_plan *plan = nullptr;
            detail::check(sdsp_hip_welch_plan_create(&plan, n_fft, hop, m_window.data(), m_detrend, m_scaling, m_fs,
                                                     detail::precision_of<real_t>::value, 0, m_device));
            m_plan.reset(plan);
        }
        if (!m_acc) {
            if (!m_state)
                m_state.alloc(static_cast<size_t>(hist * m_channels) * sizeof(real_t), m_device);
            m_acc.alloc(static_cast<size_t>(bins * m_channels) * sizeof(double), m_device);
            zero_buffers();
        }
    }

    std::uint64_t m_channels;
    int m_detrend, m_scaling;
    double m_fs;
    int m_device;
    std::array<double, n_fft> m_window{};
    detail::plan_ptr<sdsp_hip_welch_plan, sdsp_hip_welch_plan_destroy> m_plan;
    detail::device_buffer m_state, m_acc;
    std::uint64_t m_position{ 0 }, m_frames{ 0 };
};
} // namespace sdsp

#endif // SDSP_MI355X_WELCH_H
