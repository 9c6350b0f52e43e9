// sdsp/detail/hip_runtime.h -- glue between the sdsp:: headers and the C ABI (sdsp_hip.h).
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../sdsp_hip.h"

namespace sdsp
{
// Thrown when the MI355X path cannot run (no device, HIP error, unsupported shape).  The
// reference has no run-time errors on this path; there is deliberately no CPU fallback here.
class hip_error : public std::runtime_error {
public:
    hip_error(int code, const std::string &what) : std::runtime_error(what), m_code(code) {}
    int code() const noexcept { return m_code; }

private:
    int m_code;
};

namespace detail
{
inline void check(int rc)
{
    if (rc != SDSP_HIP_OK)
        throw hip_error(rc, std::string("sdsp_hip: ") + sdsp_hip_last_error_string());
}

template <typename real_t> struct precision_of;
template <> struct precision_of<float> { static constexpr int value = SDSP_HIP_F32; };
template <> struct precision_of<double> { static constexpr int value = SDSP_HIP_F64; };

// Owner of one device allocation on one device: empty until alloc(), freed by reset() and by the destructor.
class device_buffer {
public:
    device_buffer() = default;
    ~device_buffer() { reset(); }
    device_buffer(const device_buffer &) = delete;
    device_buffer &operator=(const device_buffer &) = delete;

    void alloc(std::size_t bytes, int device)
    {
        reset();
        m_device = device;
        check(sdsp_hip_malloc(&m_ptr, bytes, device));
    }
    void reset() noexcept
    {
        if (m_ptr)
            sdsp_hip_free(m_ptr, m_device);
        m_ptr = nullptr;
    }
    void upload(const void *host, std::size_t bytes, std::size_t byte_offset = 0)
    {
        check(sdsp_hip_memcpy_h2d(static_cast<unsigned char *>(m_ptr) + byte_offset, host, bytes, m_device));
    }
    void download(void *host, std::size_t bytes, std::size_t byte_offset = 0) const
    {
        check(sdsp_hip_memcpy_d2h(host, static_cast<const unsigned char *>(m_ptr) + byte_offset, bytes, m_device));
    }
    // the first `count` elements set to `value`, through a host image
    template <typename elem_t> void fill(std::size_t count, elem_t value)
    {
        const std::vector<elem_t> host(count, value);
        upload(host.data(), count * sizeof(elem_t));
    }
    void *get() const noexcept { return m_ptr; }
    explicit operator bool() const noexcept { return m_ptr != nullptr; }

private:
    void *m_ptr{ nullptr };
    int m_device{ 0 };
};

// Owner of a plan of the C ABI: a unique_ptr that ends in the family's sdsp_hip_*_plan_destroy.
template <typename plan_t, int (*destroy_fn)(plan_t *)> struct plan_deleter {
    void operator()(plan_t *plan) const noexcept { destroy_fn(plan); }
};
template <typename plan_t, int (*destroy_fn)(plan_t *)> using plan_ptr = std::unique_ptr<plan_t, plan_deleter<plan_t, destroy_fn>>;

// One buffer of a host-pointer call: copied in from copy_in_from and back to copy_back_to where these are set; an item with neither
// is absent and reaches the callable as a null device pointer.
struct stage_item {
    const void *copy_in_from;
    void *copy_back_to;
    std::size_t bytes;
};

// The host-pointer form of a call (the C++ twin of host_stage in capi.hip): allocates every present item on `device`, copies the
// inputs in, calls run(device pointers, one per item), which returns the C ABI's code, and on success copies the outputs back.
// Throws at the first failure; the device buffers are freed on every path, also when run itself throws.
template <std::size_t n_items, typename run_t> void host_stage(int device, const stage_item (&items)[n_items], run_t &&run)
{
    device_buffer buf[n_items];
    void *dev[n_items];
    for (std::size_t i = 0; i < n_items; ++i)
        if (items[i].copy_in_from || items[i].copy_back_to)
            buf[i].alloc(items[i].bytes, device);
    for (std::size_t i = 0; i < n_items; ++i) {
        if (items[i].copy_in_from)
            buf[i].upload(items[i].copy_in_from, items[i].bytes);
        dev[i] = buf[i].get();
    }
    check(run(static_cast<void *const *>(dev)));
    for (std::size_t i = 0; i < n_items; ++i)
        if (items[i].copy_back_to)
            buf[i].download(items[i].copy_back_to, items[i].bytes);
}

// RAII owner of an FFT plan
class fft_plan_handle {
public:
    fft_plan_handle(std::uint32_t n, int radix, int direction, int precision, std::uint64_t max_batch, int device)
    {
        sdsp_hip_fft_plan *plan = nullptr;
        check(sdsp_hip_fft_plan_create(&plan, n, radix, direction, precision, max_batch, device));
        m_plan.reset(plan);
    }
    fft_plan_handle(const fft_plan_handle &) = delete;
    fft_plan_handle &operator=(const fft_plan_handle &) = delete;
    sdsp_hip_fft_plan *get() const noexcept { return m_plan.get(); }
    std::mutex &mutex() noexcept { return m_mutex; } // the plan's host staging buffer is not re-entrant

private:
    plan_ptr<sdsp_hip_fft_plan, sdsp_hip_fft_plan_destroy> m_plan;
    std::mutex m_mutex;
};
} // namespace detail
} // namespace sdsp
