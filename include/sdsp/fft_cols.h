// sdsp/fft_cols.h -- batched FFT along the strided axis for the MI355X engine (sdsp_hip_fft_cols_*).
//
// Every column of `batch` compact row-major cubes of n rows x width complex columns is one transform of n points: the Doppler step
// of a pulse-Doppler chain ([cube][pulse][range bin]) and the second axis of a 2-D transform, in one read and one write of the cube.
// Mirrors sdsp::stft_bank's plan handling (sdsp/stft.h): an RAII plan made on first use, exec() on device pointers, exec_host() for
// host buffers, info().  Forward plans take a window over the rows, a shift (zero frequency in the middle) and power output; reverse
// plans (conjugate twiddles, 1/n) undo a forward plan of the same shift.  There is no CPU path.
#ifndef SDSP_MI355X_FFT_COLS_H
#define SDSP_MI355X_FFT_COLS_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "detail/hip_runtime.h"

namespace sdsp
{
template <typename real_t = float> class fft_cols_plan {
public:
    fft_cols_plan(std::uint32_t n, std::uint64_t width, int direction = SDSP_HIP_FORWARD, int output = SDSP_HIP_FFT_COLS_COMPLEX,
                  bool shift = false, int device = 0)
        : m_n(n), m_width(width), m_direction(direction), m_output(output), m_shift(shift), m_device(device)
    {
    }
    fft_cols_plan(const fft_cols_plan &) = delete;
    fft_cols_plan &operator=(const fft_cols_plan &) = delete;

    // n values over the rows (forward plans); an empty vector removes the window
    void set_window(const std::vector<double> &w)
    {
        m_window = w;
        m_plan.reset();
    }
    // 0 = the tuned kernel, 1 = the plain cross-check kernel
    void set_variant(int variant)
    {
        ensure_plan();
        detail::check(sdsp_hip_fft_cols_plan_set_variant(m_plan.get(), variant));
    }
    // real_t values per output element: 2 for complex output, 1 for power
    std::uint32_t out_values() const noexcept { return m_output == SDSP_HIP_FFT_COLS_COMPLEX ? 2u : 1u; }
    std::uint32_t n() const noexcept { return m_n; }
    std::uint64_t width() const noexcept { return m_width; }

    // device pointers to `batch` cubes; device_out == device_in transforms in place (complex output); asynchronous on `stream`
    void exec(const void *device_in, void *device_out, std::uint64_t batch, void *stream = nullptr)
    {
        ensure_plan();
        detail::check(sdsp_hip_fft_cols_exec(m_plan.get(), device_in, device_out, batch, stream));
    }
    // host pointers: in = batch x n x width complex (interleaved), out = batch x n x width x out_values() reals, both contiguous
    void exec_host(const real_t *host_in, real_t *host_out, std::uint64_t batch)
    {
        ensure_plan();
        detail::check(sdsp_hip_fft_cols_exec_host(m_plan.get(), host_in, host_out, batch));
    }
    std::uint64_t launches(std::uint64_t batch)
    {
        ensure_plan();
        std::uint64_t v = 0;
        detail::check(sdsp_hip_fft_cols_plan_launches(m_plan.get(), batch, &v));
        return v;
    }
    sdsp_hip_fft_cols_plan_info info()
    {
        ensure_plan();
        sdsp_hip_fft_cols_plan_info i{};
        detail::check(sdsp_hip_fft_cols_plan_get_info(m_plan.get(), &i));
        return i;
    }

private:
    void ensure_plan()
    {
        if (!m_window.empty() && m_window.size() != m_n)
            throw hip_error(SDSP_HIP_ERR_INVALID_ARG, "sdsp::fft_cols_plan: the window must hold n values");
        if (m_plan)
            return;
        sdsp_hip_fft_cols_plan *plan = nullptr;
        detail::check(sdsp_hip_fft_cols_plan_create(&plan, m_n, m_width, m_direction, detail::precision_of<real_t>::value, m_output,
                                                    m_shift ? 1 : 0, m_window.empty() ? nullptr : m_window.data(), m_device));
        m_plan.reset(plan);
    }

    std::uint32_t m_n;
    std::uint64_t m_width;
    int m_direction;
    int m_output;
    bool m_shift;
    int m_device;
    std::vector<double> m_window;
    detail::plan_ptr<sdsp_hip_fft_cols_plan, sdsp_hip_fft_cols_plan_destroy> m_plan;
};
} // namespace sdsp

#endif // SDSP_MI355X_FFT_COLS_H
