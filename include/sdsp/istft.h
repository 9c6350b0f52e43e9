// sdsp/istft.h -- streaming inverse STFT bank for the MI355X engine (sdsp_hip_istft_*).
//
// Overlap-add synthesis from frames of n_fft / 2 + 1 complex bins (sdsp::stft_bank's COMPLEX layout), every hop samples, with the
// library's reverse real-input FFT, for a bank of channels on the device.  Mirrors sdsp::stft_bank (sdsp/stft.h): RAII plan and
// device-resident per-channel pending sums, process() on device pointers, process_host() for host buffers.  A call of F frames per
// channel writes F hop samples; with the default window-square normalisation, istft_bank(stft_bank(x)) is x delayed by n_fft - hop
// samples.  Pinned to torch.istft(center = False) and numpy; there is no CPU path.
#ifndef SDSP_MI355X_ISTFT_H
#define SDSP_MI355X_ISTFT_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <std::uint32_t n_fft, std::uint32_t hop, typename real_t = float> class istft_bank {
    static_assert(n_fft >= 32 && (n_fft & (n_fft - 1)) == 0, "n_fft must be a power of two >= 32");
    static_assert(n_fft <= (sizeof(real_t) == 8 ? 32768u : 65536u), "n_fft must be in the real-input range (f32 .. 65536, f64 .. 32768)");
    static_assert(hop >= 1 && hop <= n_fft, "hop must be in [1, n_fft]");

public:
    static constexpr std::uint32_t bins = n_fft / 2 + 1;
    static constexpr std::uint32_t hist = n_fft - hop; // pending sums per channel, time order

    explicit istft_bank(std::uint64_t channels, int norm = SDSP_HIP_ISTFT_NORMALIZED, int device = 0)
        : m_channels(channels), m_norm(norm), m_device(device)
    {
        set_window(SDSP_HIP_WINDOW_HANN);
    }
    istft_bank(const istft_bank &) = delete;
    istft_bank &operator=(const istft_bank &) = delete;

    // the analysis window w (the synthesis window is w / its squared overlap-add, or w itself for SDSP_HIP_ISTFT_RAW)
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
    void reset()
    {
        if (m_state)
            fill_state(real_t(0));
    }

    // device pointers, channel-major; in_stride counts complex bins, out_stride reals; asynchronous on `stream`
    void process(const void *device_in, std::uint64_t in_stride, real_t *device_out, std::uint64_t out_stride, std::uint64_t frames,
                 void *stream = nullptr)
    {
        ensure_plan();
        ensure_state();
        detail::check(sdsp_hip_istft_process(m_plan.get(), device_in, in_stride, device_out, out_stride, m_channels, frames, m_state.get(),
                                             stream));
    }
    // host pointers: in = channels x frames x bins x (re, im), out = channels x frames hop, both contiguous
    void process_host(const real_t *host_in, real_t *host_out, std::uint64_t frames)
    {
        ensure_plan();
        ensure_state();
        const std::uint64_t in_row = frames * bins, out_row = frames * hop;
        const size_t in_bytes = static_cast<size_t>(m_channels * in_row * 2) * sizeof(real_t);
        const size_t out_bytes = static_cast<size_t>(m_channels * out_row) * sizeof(real_t);
        if (in_bytes == 0 || out_bytes == 0)
            return;
        detail::host_stage(m_device, { { host_in, nullptr, in_bytes }, { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_istft_process(m_plan.get(), dev[0], in_row, dev[1], out_row, m_channels, frames, m_state.get(), nullptr);
        });
    }
    std::uint64_t channels() const noexcept { return m_channels; }
    const std::array<double, n_fft> &window() const { return m_window; }
    std::array<double, n_fft> synthesis_window() const
    {
        std::array<double, n_fft> g{};
        detail::check(sdsp_hip_istft_synthesis_window(n_fft, hop, m_window.data(), m_norm, g.data()));
        return g;
    }
    sdsp_hip_istft_plan_info info()
    {
        ensure_plan();
        sdsp_hip_istft_plan_info i{};
        detail::check(sdsp_hip_istft_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    static constexpr size_t state_len = hist > 0 ? hist : 1;
    void ensure_plan()
    {
        if (m_plan)
            return;
        sdsp_hip_istft_plan *plan = nullptr;
        detail::check(sdsp_hip_istft_plan_create(&plan, n_fft, hop, m_window.data(), m_norm, detail::precision_of<real_t>::value, 0,
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
    int m_norm;
    int m_device;
    std::array<double, n_fft> m_window{};
    detail::plan_ptr<sdsp_hip_istft_plan, sdsp_hip_istft_plan_destroy> m_plan;
    detail::device_buffer m_state;
};
} // namespace sdsp

#endif // SDSP_MI355X_ISTFT_H
