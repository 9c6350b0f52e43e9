// sdsp/stft.h -- streaming STFT bank for the MI355X engine (sdsp_hip_stft_*).
//
// Frames of n_fft samples every hop samples, windowed and transformed with the library's real-input FFT, for a bank of channels
// on the device.  Mirrors sdsp::fir_resampler_bank (sdsp/resample.h): RAII plan and device-resident per-channel history,
// process() on device pointers, process_host() for host buffers.  A call of S samples per channel (S a multiple of hop) writes
// S / hop frames of n_fft / 2 + 1 bins: complex (interleaved re, im), power or magnitude.  Pinned to torch.stft(center = False)
// and numpy; there is no CPU path.
#ifndef SDSP_MI355X_STFT_H
#define SDSP_MI355X_STFT_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <std::uint32_t n_fft, std::uint32_t hop, typename real_t = float> class stft_bank {
    static_assert(n_fft >= 32 && (n_fft & (n_fft - 1)) == 0, "n_fft must be a power of two >= 32");
    static_assert(n_fft <= (sizeof(real_t) == 8 ? 32768u : 65536u), "n_fft must be in the real-input range (f32 .. 65536, f64 .. 32768)");
    static_assert(hop >= 1 && hop <= n_fft, "hop must be in [1, n_fft]");

public:
    static constexpr std::uint32_t bins = n_fft / 2 + 1;
    static constexpr std::uint32_t hist = n_fft - hop; // history per channel, newest first

    explicit stft_bank(std::uint64_t channels, int output = SDSP_HIP_STFT_COMPLEX, int device = 0)
        : m_channels(channels), m_output(output), m_device(device)
    {
        set_window(SDSP_HIP_WINDOW_HANN);
    }
    stft_bank(const stft_bank &) = delete;
    stft_bank &operator=(const stft_bank &) = delete;

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
    void preload_filter(double value) { fill_state(static_cast<real_t>(value)); }
    void reset()
    {
        if (m_state)
            fill_state(real_t(0));
    }

    // frames of a call of `samples` per channel; throws unless samples is a multiple of hop
    static std::uint64_t frames(std::uint64_t samples)
    {
        std::uint64_t n = 0;
        detail::check(sdsp_hip_stft_frames(hop, samples, &n));
        return n;
    }
    // real_t values per output bin: 2 for complex output, 1 for power and magnitude
    std::uint32_t bin_values() const noexcept { return m_output == SDSP_HIP_STFT_COMPLEX ? 2u : 1u; }

    // device pointers, channel-major; out_stride counts bins; asynchronous on `stream`; continues every channel's stream
    void process(const real_t *device_in, std::uint64_t in_stride, void *device_out, std::uint64_t out_stride, std::uint64_t samples,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_stft_process(m_plan.get(), device_in, in_stride, device_out, out_stride, m_channels, samples,
                                            m_state.get(), stream));
    }
    // host pointers: in = channels x samples, out = channels x frames(samples) x bins x bin_values(), both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t samples)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t row = frames(samples) * bins;
        const size_t in_bytes = static_cast<size_t>(m_channels * samples) * sizeof(real_t);
        const size_t out_bytes = static_cast<size_t>(m_channels * row * bin_values()) * sizeof(real_t);
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_stft_process(m_plan.get(), dev[0], samples, dev[1], row, m_channels, samples, m_state.get(), nullptr);
        });
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    const std::array<double, n_fft> &window() const { return m_window; }
    sdsp_hip_stft_plan_info info()
    {
        ensure_plan();
        sdsp_hip_stft_plan_info i{};
        detail::check(sdsp_hip_stft_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    static constexpr size_t state_len = hist > 0 ? hist : 1;
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_stft_plan *plan = nullptr;
        detail::check(sdsp_hip_stft_plan_create(&plan, n_fft, hop, m_window.data(), m_output, detail::precision_of<real_t>::value, 0,
                                                m_device));
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
    int m_output;
    int m_device;
    std::array<double, n_fft> m_window{};
    detail::plan_ptr<sdsp_hip_stft_plan, sdsp_hip_stft_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_STFT_H
