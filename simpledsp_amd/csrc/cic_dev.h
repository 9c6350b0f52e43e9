// cic_dev.h -- what the two CIC kernels files (cic.hip, cic_interp.hip) share on the device: the signed twin of a register type, the
// sign extension of a sample to the register width, and the cross-lane move of the stage scan.  One definition each.
#pragma once

#include "stream_dev.h"

namespace sdsp_hip
{
template <typename ACC> struct signed_of {
    typedef int32_t type;
};
template <> struct signed_of<uint64_t> {
    typedef int64_t type;
};

// a sample, sign-extended to the register width
template <typename ACC, typename IN> __device__ __forceinline__ ACC widen(IN x)
{
    return static_cast<ACC>(static_cast<typename signed_of<ACC>::type>(x));
}

// the value of the lane d below (its own for the lanes that have none)
__device__ __forceinline__ uint32_t lane_up(uint32_t t, uint32_t d) { return __shfl_up(t, d, 64); }
__device__ __forceinline__ uint64_t lane_up(uint64_t t, uint32_t d)
{
    return static_cast<uint64_t>(__shfl_up(static_cast<unsigned long long>(t), d, 64));
}
} // namespace sdsp_hip
