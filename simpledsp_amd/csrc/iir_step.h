// iir_step.h -- the cascaded-biquad recurrence shared by the IIR bank (iir.hip) and the forward-backward plans
// (iir_filtfilt.hip): one sample through the cascade, per-channel state in and out, the precision pairs and the 16-byte
// global accesses.  Both files are compiled with -ffp-contract=off -fno-slp-vectorize, so every kernel that includes this
// computes the same bits for the same inputs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sdsp_hip.h"

namespace sdsp_hip
{
namespace
{
// S: the type the samples are stored in; R: the type the recurrence (state, coefficients, arithmetic) runs in.
// (float, float), (double, double), or -- the mixed mode, SDSP_HIP_F32_F64STATE -- (float, double): 8 bytes of HBM traffic per
// sample with the double-precision recurrence's accuracy (f32 state loses 1e-4 at f0/fs = 0.005).
// A kernel's pair of types: S samples in memory, R recurrence.
template <typename S_, typename R_> struct prec {
    using S = S_;
    using R = R_;
    static constexpr bool fused = sizeof(S_) == 4; // f32 and mixed: parity by tolerance; f64: bit-exact operation order
};
using prec_f32 = prec<float, float>;
using prec_f64 = prec<double, double>;
using prec_mix = prec<float, double>;

template <typename R> struct vec16;
template <> struct vec16<float> {
    using type = float4;
    using native = float __attribute__((ext_vector_type(4)));
    static constexpr int n = 4;
};
template <> struct vec16<double> {
    using type = double2;
    using native = double __attribute__((ext_vector_type(2)));
    static constexpr int n = 2;
};

// 16-byte global accesses; NT = streaming (non-temporal) policy: every sample is touched exactly
// once each way, and keeping it out of the L2 / Infinity-Cache replacement state is worth ~10 % on
// in-place streams (tools/membench.hip)
template <typename R, bool NT> __device__ __forceinline__ typename vec16<R>::type gload16(const R *p)
{
    using V = typename vec16<R>::type;
    using N = typename vec16<R>::native;
    if constexpr (NT) {
        const N v = __builtin_nontemporal_load(reinterpret_cast<const N *>(p));
        V out;
        __builtin_memcpy(&out, &v, 16);
        return out;
    } else {
        return *reinterpret_cast<const V *>(p);
    }
}
template <typename R, bool NT> __device__ __forceinline__ void gstore16(R *p, typename vec16<R>::type a)
{
    using V = typename vec16<R>::type;
    using N = typename vec16<R>::native;
    if constexpr (NT) {
        N v;
        __builtin_memcpy(&v, &a, 16);
        __builtin_nontemporal_store(v, reinterpret_cast<N *>(p));
    } else {
        *reinterpret_cast<V *>(p) = a;
    }
}

// One sample through the cascade.  y1[j] / y2[j] are level j's values one / two samples ago
// (level 0 = gain-scaled input, level M = output): the reference's m_mem ring (casc_2o_iir.h:15)
// with the ring index resolved at compile time.
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// FUSED: parity by tolerance (f32 and mixed mode) -- each "x*b - y*a" pair is a multiply and an FMA; !FUSED (f64): the
// reference's exact operation order, bit for bit.
template <typename R, int KIND, int M, bool FUSED, typename ARGS>
__device__ __forceinline__ R cascade_step(R x, const ARGS &p, R (&y1)[M + 1], R (&y2)[M + 1], R (&y3)[M + 1])
{
    R cur[M + 1];
    cur[0] = x * p.gain; // :52 / :242
#pragma unroll
    for (int j = 0; j < M; j++) {
        R acc = cur[j];
        if constexpr (FUSED) {
            // parity by tolerance (1e-6): same terms, grouped as the reference groups them, but
            // each "x*b - y*a" pair costs a multiply and an FMA instead of two multiplies and a subtract
            if constexpr (KIND == SDSP_HIP_IIR_GENERIC) {
                acc += fma_t(y1[j], p.b1[j], -(y1[j + 1] * p.a1[j]));
                acc += fma_t(y2[j], p.b2[j], -(y2[j + 1] * p.a2[j]));
            } else if constexpr (KIND == SDSP_HIP_IIR_LP) {
                acc += fma_t(-y1[j + 1], p.a1[j], y1[j] + y1[j]);
                acc += fma_t(-y2[j + 1], p.a2[j], y2[j]);
            } else if constexpr (KIND == SDSP_HIP_IIR_HP) {
                acc += fma_t(-y1[j + 1], p.a1[j], -y1[j] - y1[j]);
                acc += fma_t(-y2[j + 1], p.a2[j], y2[j]);
            } else {
                acc += -y1[j + 1] * p.a1[j];
                acc += fma_t(-y2[j + 1], p.a2[j], -y2[j]);
            }
        } else if constexpr (KIND == SDSP_HIP_IIR_GENERIC) { // :67-68
            acc += y1[j] * p.b1[j] - y1[j + 1] * p.a1[j];
            acc += y2[j] * p.b2[j] - y2[j + 1] * p.a2[j];
        } else if constexpr (KIND == SDSP_HIP_IIR_LP) { // :292-293
            acc += y1[j] + y1[j] - y1[j + 1] * p.a1[j];
            acc += y2[j] - y2[j + 1] * p.a2[j];
        } else if constexpr (KIND == SDSP_HIP_IIR_HP) { // :350-351
            acc += -y1[j] - y1[j] - y1[j + 1] * p.a1[j];
            acc += y2[j] - y2[j + 1] * p.a2[j];
        } else { // band pass :408-409
            acc += -y1[j + 1] * p.a1[j];
            acc += -y2[j] - y2[j + 1] * p.a2[j];
        }
        cur[j + 1] = acc;
    }
#pragma unroll
    for (int j = 0; j <= M; j++) {
        y3[j] = y2[j];
        y2[j] = y1[j];
        y1[j] = cur[j];
    }
    return cur[M]; // :71 / :254
}

template <typename R, int M, typename ARGS>
__device__ __forceinline__ void load_state(const ARGS &p, uint64_t c, R (&y1)[M + 1],
                                           R (&y2)[M + 1], R (&y3)[M + 1])
{
#pragma unroll
    for (int j = 0; j <= M; j++) {
        y1[j] = y2[j] = y3[j] = R(0);
    }
    if (p.state) {
#pragma unroll
        for (int j = 0; j <= M; j++) {
            y1[j] = p.state[(uint64_t)(3 * j + 0) * p.channels + c];
            y2[j] = p.state[(uint64_t)(3 * j + 1) * p.channels + c];
            y3[j] = p.state[(uint64_t)(3 * j + 2) * p.channels + c];
        }
    }
}

template <typename R, int M, typename ARGS>
__device__ __forceinline__ void store_state(const ARGS &p, uint64_t c, const R (&y1)[M + 1],
                                            const R (&y2)[M + 1], const R (&y3)[M + 1])
{
    if (p.state) {
#pragma unroll
        for (int j = 0; j <= M; j++) {
            p.state[(uint64_t)(3 * j + 0) * p.channels + c] = y1[j];
            p.state[(uint64_t)(3 * j + 1) * p.channels + c] = y2[j];
            p.state[(uint64_t)(3 * j + 2) * p.channels + c] = y3[j];
        }
    }
}
} // namespace
} // namespace sdsp_hip
