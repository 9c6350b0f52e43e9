// sdsp/csd.h -- streaming cross-spectral density and coherence bank for the MI355X engine (sdsp_hip_csd_*).
//
// scipy.signal.csd and scipy.signal.coherence for a list of channel pairs of a bank of channels on the device, accumulated across
// calls: the Welch bank's segments, detrending, window and real-input FFT; conj(X_a) X_b of every pair and |X_c|^2 of every channel
// are summed in double on the device.  Mirrors sdsp::welch_bank (sdsp/welch.h): RAII plan and device-resident per-channel history
// and sums, process() on device pointers, process_host() for host buffers; csd() / coherence() and their _host forms turn the sums
// into the estimates.  Pinned to scipy.signal and numpy; there is no CPU path.
#ifndef SDSP_MI355X_CSD_H
#define SDSP_MI355X_CSD_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <std::uint32_t n_fft, std::uint32_t hop, typename real_t = float> class csd_bank {
    static_assert(n_fft >= 32 && (n_fft & (n_fft - 1)) == 0, "n_fft must be a power of two >= 32");
    static_assert(n_fft <= (sizeof(real_t) == 8 ? 32768u : 65536u), "n_fft must be in the real-input range (f32 .. 65536, f64 .. 32768)");
    static_assert(hop >= 1 && hop <= n_fft, "hop must be in [1, n_fft]");

public:
    static constexpr std::uint32_t bins = n_fft / 2 + 1;
    static constexpr std::uint32_t hist = n_fft - 1; // history per channel, newest first

    // pairs: (a, b) channel indices; pair i is row i of csd() and coherence()
    csd_bank(std::uint64_t channels, const std::vector<std::pair<std::uint32_t, std::uint32_t>> &pairs,
             int detrend = SDSP_HIP_DETREND_CONSTANT, int scaling = SDSP_HIP_SCALING_DENSITY, double fs = 1.0, int device = 0)
        : m_channels(channels), m_detrend(detrend), m_scaling(scaling), m_fs(fs), m_device(device)
    {
        for (const auto &p : pairs) {
            m_pairs.push_back(p.first);
            m_pairs.push_back(p.second);
        }
        set_window(SDSP_HIP_WINDOW_HANN);
    }
    csd_bank(const csd_bank &) = delete;
    csd_bank &operator=(const csd_bank &) = delete;

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
        if (m_acc_xy)
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
    std::uint64_t channels() const noexcept { return m_channels; }
    std::uint64_t npairs() const noexcept { return m_pairs.size() / 2; }

    // device pointer, channel-major; asynchronous on `stream`; continues every channel's stream
    void process(const real_t *device_in, std::uint64_t in_stride, std::uint64_t samples, void *stream = nullptr)
    {
        ensure();
        const std::uint64_t f = segments(samples);
        detail::check(sdsp_hip_csd_process(m_plan.get(), device_in, in_stride, samples, m_position, m_state.get(), acc_xy(), 2 * bins,
                                           acc_auto(), bins, stream));
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
            const int rc = sdsp_hip_csd_process(m_plan.get(), dev[0], samples, samples, m_position, m_state.get(), acc_xy(), 2 * bins,
                                                acc_auto(), bins, nullptr);
            return rc ? rc : sdsp_hip_device_synchronize(m_device);
        });
        m_position += samples;
        m_frames += f;
    }
    // the cross-spectral density from the segments so far: npairs rows of bins interleaved (re, im) values, out_stride reals apart
    // (device pointer, asynchronous)
    void csd(real_t *device_out, std::uint64_t out_stride, void *stream = nullptr)
    {
        finalize(SDSP_HIP_CSD_CROSS, device_out, out_stride, stream);
    }
    // the magnitude-squared coherence: npairs rows of bins values, out_stride apart (device pointer, asynchronous)
    void coherence(real_t *device_out, std::uint64_t out_stride, void *stream = nullptr)
    {
        finalize(SDSP_HIP_CSD_COHERENCE, device_out, out_stride, stream);
    }
    // host pointers: out = npairs x 2 bins (csd) or npairs x bins (coherence), contiguous (synchronous)
    void csd_host(real_t *host_out) { finalize_host(SDSP_HIP_CSD_CROSS, host_out, 2 * bins); }
    void coherence_host(real_t *host_out) { finalize_host(SDSP_HIP_CSD_COHERENCE, host_out, bins); }
    const std::array<double, n_fft> &window() const { return m_window; }
    sdsp_hip_csd_plan_info info()
    {
        ensure();
        sdsp_hip_csd_plan_info i{};
        detail::check(sdsp_hip_csd_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    void finalize(int mode, real_t *device_out, std::uint64_t out_stride, void *stream)
    {
        ensure();
        detail::check(sdsp_hip_csd_finalize(m_plan.get(), mode, acc_xy(), 2 * bins, acc_auto(), bins, m_frames, device_out, out_stride,
                                            stream));
    }
    void finalize_host(int mode, real_t *host_out, std::uint64_t row)
    {
        ensure();
        const size_t out_bytes = static_cast<size_t>(npairs() * row) * sizeof(real_t);
        detail::host_stage(m_device, { { nullptr, host_out, out_bytes } }, [&](void *const *dev) {
            return sdsp_hip_csd_finalize(m_plan.get(), mode, acc_xy(), 2 * bins, acc_auto(), bins, m_frames, dev[0], row, nullptr);
        });
    }
    double *acc_xy() const noexcept { return static_cast<double *>(m_acc_xy.get()); }
    double *acc_auto() const noexcept { return static_cast<double *>(m_acc_auto.get()); }
    void zero_buffers()
    {
        m_state.fill(static_cast<size_t>(hist * m_channels), real_t(0));
        m_acc_xy.fill(static_cast<size_t>(2 * bins * npairs()), 0.0);
        m_acc_auto.fill(static_cast<size_t>(bins * m_channels), 0.0);
    }
    void ensure()
    {
        if (!m_plan) {
            sdsp_hip_csd_plan *plan = nullptr;
            detail::check(sdsp_hip_csd_plan_create(&plan, n_fft, hop, m_window.data(), m_detrend, m_scaling, m_fs,
                                                   detail::precision_of<real_t>::value, m_channels, npairs(), m_pairs.data(), 0,
                                                   m_device));
            m_plan.reset(plan);
        }
        if (!m_acc_auto) {
            if (!m_state)
                m_state.alloc(static_cast<size_t>(hist * m_channels) * sizeof(real_t), m_device);
            if (!m_acc_xy)
                m_acc_xy.alloc(static_cast<size_t>(2 * bins * npairs()) * sizeof(double), m_device);
            m_acc_auto.alloc(static_cast<size_t>(bins * m_channels) * sizeof(double), m_device);
            zero_buffers();
        }
    }

    std::uint64_t m_channels;
    int m_detrend, m_scaling;
    double m_fs;
    int m_device;
    std::vector<std::uint32_t> m_pairs; // a_0, b_0, a_1, b_1 ..
    std::array<double, n_fft> m_window{};
    detail::plan_ptr<sdsp_hip_csd_plan, sdsp_hip_csd_plan_destroy> m_plan;
    detail::device_buffer m_state, m_acc_xy, m_acc_auto;
    std::uint64_t m_position{ 0 }, m_frames{ 0 };
};
} // namespace sdsp

#endif // SDSP_MI355X_CSD_H
