// stream_dev.h -- what the streaming layers (stft, istft, welch, pfb, pfb_synth, fir_fft, fir_resample, stream_carry .hip) share: the
// workgroup size, the 16-byte vector and complex-pair types, workgroup placement, the cheap divide, and the host side of a launch
// (grid from a thread count, the launch status).  One definition each.
#pragma once

#include "sdsp_hip_internal.h"

#include <hip/hip_runtime.h>

namespace sdsp_hip
{
constexpr int kThreads = 256;

// N reals as one vector
template <typename R, int N> struct vec_n {
    typedef R type __attribute__((ext_vector_type(N)));
};

// 16 bytes of reals: four f32 or two f64
template <typename R> struct vec16 {
    static constexpr int lanes = 16 / sizeof(R);
    typedef typename vec_n<R, lanes>::type type;
};

// one interleaved complex value
template <typename R> struct cplx_pair {
    typedef typename vec_n<R, 2>::type type;
};

// workgroup b -> the position it works on: the blocks that share an XCD (b mod 8: the dispatcher deals workgroups round-robin over
// the eight) get one contiguous range, so that units which overlap one another are read by workgroups behind the same L2.  A
// bijection on [0, nb) for every nb.
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb)
{
    const uint32_t q = nb / 8, r = nb % 8, x = b % 8;
    return x * q + min(x, r) + b / 8;
}

// a / b with the 32-bit divide when both fit (the common case)
__device__ __forceinline__ uint64_t udiv(uint64_t a, uint64_t b)
{
    return (a | b) < (1ull << 32) ? static_cast<uint64_t>(static_cast<uint32_t>(a) / static_cast<uint32_t>(b)) : a / b;
}

// ceil(log2(v))
inline uint32_t log2u(uint64_t v)
{
    uint32_t l = 0;
    while ((1ull << l) < v)
        l++;
    return l;
}

// a grid of `blocks` workgroups, or UNSUPPORTED "<what> too large for one launch" (what: "stft slice", "pfb state" ..)
inline int grid_of_blocks(uint64_t blocks, const char *what, dim3 *grid)
{
    if (blocks > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, std::string(what) + " too large for one launch");
    *grid = dim3(static_cast<uint32_t>(blocks));
    return SDSP_HIP_OK;
}
// ... for `threads` threads in workgroups of kThreads
inline int grid_for(uint64_t threads, const char *what, dim3 *grid) { return grid_of_blocks((threads + kThreads - 1) / kThreads, what, grid); }

// after a family's launches: HIP "<family> launch: ..." when one of them was refused
inline int launch_status(const char *family)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(SDSP_HIP_ERR_HIP, std::string(family) + " launch: " + hipGetErrorString(e));
    return SDSP_HIP_OK;
}
} // namespace sdsp_hip
