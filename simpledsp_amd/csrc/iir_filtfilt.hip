// iir_filtfilt.hip -- zero-phase forward-backward filtering of cascaded-biquad banks on gfx950.
//
// For each channel the row x of L samples is extended by P samples at each end (odd / even / constant, in the sample type S),
// run forward through the cascade from the steady state of its first extended sample, run backward from the steady state of the
// last forward output, and its middle L samples are written back in place: scipy.signal.sosfiltfilt in the library's own
// arithmetic.  The recurrence is iir_step.h's cascade_step, the one the IIR bank runs, so a plan equals the composition pad ->
// sdsp_hip_iir_process -> flip -> sdsp_hip_iir_process -> flip -> slice bit for bit.  Compiled with iir.hip's flags.
//
// Two kernels, bit-identical:
//   sdsp_filtfilt_fused_kernel   one wave owns 64 channels and moves them in iir.hip's [64 channels x 512 B] super-tiles
//                                (row-group-major 16-byte accesses, LDS transpose, each lane filtering its own row).  Order:
//                                prologue (right-edge extension inputs -> workspace), forward over the left extension (no
//                                stores), forward over the tiles 0 .. T-1 in place, forward over the workspace, then backward
//                                over the workspace and the tiles T-1 .. 0 in place.  The left extension is never run backward:
//                                its outputs are discarded.
//   sdsp_filtfilt_direct_kernel  one lane per channel, plain scalar accesses, the same steps: any alignment, any length.
// The workspace holds the P right-edge samples of each channel, [64-channel group][i][lane], so that a wave's workspace
// accesses are 64 consecutive elements.
#include <hip/hip_runtime.h>

#include <string>

#include "iir_step.h"
#include "sdsp_hip_internal.h"

namespace sdsp_hip
{
namespace
{
template <typename S, typename R, int M> struct ff_dev_args {
    S *data;
    S *ws; // ceil(channels / 64) * 64 * padlen samples
    uint64_t channels, samples, stride;
    uint32_t padlen;
    int padtype;
    R gain;
    R a1[M], a2[M], b1[M], b2[M];
    R ss[M + 1]; // steady state of level j per unit input, rounded to R
};

// every age of level j = R(s_j) * v, rounded in R
template <typename R, int M, typename ARGS>
__device__ __forceinline__ void steady_state(const ARGS &p, R v, R (&y1)[M + 1], R (&y2)[M + 1], R (&y3)[M + 1])
{
#pragma unroll
    for (int j = 0; j <= M; j++)
        y1[j] = y2[j] = y3[j] = p.ss[j] * v;
}

// extension samples, computed in S: left e[i] (i < P) from x[0] and x[P - i]; right e[P + L + i] from x[L - 1] and x[L - 2 - i]
template <typename S> __device__ __forceinline__ S extend(int padtype, S edge, S mirror)
{
    if (padtype == SDSP_HIP_PAD_ODD) {
        const S two_edge = S(2) * edge;
        return two_edge - mirror;
    }
    return padtype == SDSP_HIP_PAD_EVEN ? mirror : edge;
}

// ---- direct kernel: lane = channel
template <typename P, int KIND, int M>
__global__ __launch_bounds__(256) void sdsp_filtfilt_direct_kernel(ff_dev_args<typename P::S, typename P::R, M> p)
{
    using S = typename P::S;
    using R = typename P::R;
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.channels)
        return;
    S *row = p.data + c * p.stride;
    S *ws = p.ws + (c / 64) * 64 * (uint64_t)p.padlen + c % 64; // element i at ws[64 i]
    const uint64_t L = p.samples;
    const uint32_t pad = p.padlen;
    const S x0 = row[0], xl = row[L - 1];
    for (uint32_t i = 0; i < pad; i++)
        ws[64 * (uint64_t)i] = extend<S>(p.padtype, xl, row[L - 2 - i]);

    R y1[M + 1], y2[M + 1], y3[M + 1];
    steady_state<R, M>(p, (R)(pad ? extend<S>(p.padtype, x0, row[pad]) : x0), y1, y2, y3);
    for (uint32_t i = 0; i < pad; i++)
        (void)cascade_step<R, KIND, M, P::fused>((R)extend<S>(p.padtype, x0, row[pad - i]), p, y1, y2, y3);
    for (uint64_t s = 0; s < L; s++)
        row[s] = (S)cascade_step<R, KIND, M, P::fused>((R)row[s], p, y1, y2, y3);
    for (uint32_t i = 0; i < pad; i++)
        ws[64 * (uint64_t)i] = (S)cascade_step<R, KIND, M, P::fused>((R)ws[64 * (uint64_t)i], p, y1, y2, y3);

    // backward from the last forward output: y1[M] is its unrounded value
    steady_state<R, M>(p, (R)(S)y1[M], y1, y2, y3);
    for (uint32_t i = pad; i-- > 0;)
        (void)cascade_step<R, KIND, M, P::fused>((R)ws[64 * (uint64_t)i], p, y1, y2, y3);
    for (uint64_t s = L; s-- > 0;)
        row[s] = (S)cascade_step<R, KIND, M, P::fused>((R)row[s], p, y1, y2, y3);
}

// ---- fused kernel: one wave, 64 channels, iir.hip's super-tile transport.  SUBS = 4 sub-tiles of 128 bytes per channel per
// super-tile (512 contiguous bytes per channel per burst).
template <typename P, int KIND, int M, bool BACK, bool NT_LOAD, bool NT_STORE, int SUBS>
__device__ __forceinline__ void tile_pass(const ff_dev_args<typename P::S, typename P::R, M> &p, unsigned char *tile, uint64_t ch0,
                                          typename P::R (&y1)[M + 1], typename P::R (&y2)[M + 1], typename P::R (&y3)[M + 1])
{
    using S = typename P::S;
    using R = typename P::R;
    using V = typename vec16<S>::type;
    constexpr int EPV = vec16<S>::n;
    constexpr int ROWB = 128;
    constexpr int T = ROWB / (int)sizeof(S); // samples per sub-tile
    constexpr int NV = ROWB / 16;            // vectors per sub-row = lanes per row
    constexpr int RPI = 64 / NV;             // rows per wave-wide access
    constexpr int PITCH = ROWB + 16;
    const int lane = threadIdx.x;
    const int piece = lane % NV, sub = lane / NV;
    const uint64_t L = p.samples;
    const uint64_t n_super = (L + SUBS * T - 1) / (SUBS * T);
    const bool interior = ch0 + 64 <= p.channels;
    S *const lane_base = p.data + (ch0 + sub) * p.stride + (uint64_t)piece * EPV;
    const uint64_t group_step = (uint64_t)RPI * p.stride;

    for (uint64_t k = 0; k < n_super; k++) {
        const uint64_t st = BACK ? n_super - 1 - k : k;
        V stage[SUBS * NV]; // register SUBS*i + j: rows 8i..8i+7, sub-tile j
        const bool full = interior && (st + 1) * SUBS * T <= L;
        S *const tile_base = lane_base + st * SUBS * T;
        if (full) {
#pragma unroll
            for (int i = 0; i < NV; i++)
#pragma unroll
                for (int j = 0; j < SUBS; j++)
                    stage[SUBS * i + j] = gload16<S, NT_LOAD>(tile_base + i * group_step + j * T);
        } else {
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const uint64_t ch = ch0 + (uint64_t)(i * RPI + sub);
#pragma unroll
                for (int j = 0; j < SUBS; j++) {
                    const uint64_t s0 = (st * SUBS + j) * T + (uint64_t)piece * EPV;
                    stage[SUBS * i + j] = V{};
                    if (ch < p.channels && s0 < L) {
                        const S *src = p.data + ch * p.stride + s0;
                        if (s0 + EPV <= L) {
                            stage[SUBS * i + j] = gload16<S, NT_LOAD>(src);
                        } else { // the vector that straddles L: element by element, nothing at or past L is read
                            S *d = reinterpret_cast<S *>(&stage[SUBS * i + j]);
#pragma unroll
                            for (int e = 0; e < EPV; e++)
                                if (s0 + e < L)
                                    d[e] = src[e];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < SUBS; jj++) {
            const int j = BACK ? SUBS - 1 - jj : jj;
            const uint64_t first = (st * SUBS + j) * T;
            if (first >= L)
                continue; // only the last super-tile has empty sub-tiles: uniform across the wave
            const uint64_t left = L - first;
            const int valid = left < (uint64_t)T ? (int)left : T;
#pragma unroll
            for (int i = 0; i < NV; i++)
                *reinterpret_cast<V *>(tile + (i * RPI + sub) * PITCH + piece * 16) = stage[SUBS * i + j];
            __syncthreads();
            V *myrow = reinterpret_cast<V *>(tile + lane * PITCH);
            if (valid == T) {
#pragma unroll
                for (int vv = 0; vv < NV; vv++) {
                    const int v = BACK ? NV - 1 - vv : vv;
                    V x = myrow[v];
                    S *xe = reinterpret_cast<S *>(&x);
#pragma unroll
                    for (int ee = 0; ee < EPV; ee++) {
                        const int e = BACK ? EPV - 1 - ee : ee;
                        xe[e] = (S)cascade_step<R, KIND, M, P::fused>((R)xe[e], p, y1, y2, y3);
                    }
                    myrow[v] = x;
                }
            } else {
                const int nv = (valid + EPV - 1) / EPV;
                for (int vv = 0; vv < nv; vv++) {
                    const int v = BACK ? nv - 1 - vv : vv;
                    V x = myrow[v];
                    S *xe = reinterpret_cast<S *>(&x);
#pragma unroll
                    for (int ee = 0; ee < EPV; ee++) {
                        const int e = BACK ? EPV - 1 - ee : ee;
                        if (v * EPV + e < valid)
                            xe[e] = (S)cascade_step<R, KIND, M, P::fused>((R)xe[e], p, y1, y2, y3);
                    }
                    myrow[v] = x;
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NV; i++)
                stage[SUBS * i + j] = *reinterpret_cast<const V *>(tile + (i * RPI + sub) * PITCH + piece * 16);
            __syncthreads();
        }
        if (full) {
#pragma unroll
            for (int i = 0; i < NV; i++)
#pragma unroll
                for (int j = 0; j < SUBS; j++)
                    gstore16<S, NT_STORE>(tile_base + i * group_step + j * T, stage[SUBS * i + j]);
        } else {
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const uint64_t ch = ch0 + (uint64_t)(i * RPI + sub);
#pragma unroll
                for (int j = 0; j < SUBS; j++) {
                    const uint64_t s0 = (st * SUBS + j) * T + (uint64_t)piece * EPV;
                    if (ch < p.channels && s0 < L) {
                        S *dst = p.data + ch * p.stride + s0;
                        if (s0 + EPV <= L) {
                            gstore16<S, NT_STORE>(dst, stage[SUBS * i + j]);
                        } else { // nothing at or past L is written
                            const S *d = reinterpret_cast<const S *>(&stage[SUBS * i + j]);
#pragma unroll
                            for (int e = 0; e < EPV; e++)
                                if (s0 + e < L)
                                    dst[e] = d[e];
                        }
                    }
                }
            }
        }
    }
}

// two waves per SIMD where the recurrence fits beside the 128-VGPR super-tile without spilling (f32, and every precision at
// two sections); one otherwise -- a 2-wave bound costs the double recurrences of 4 .. 8 sections 12 .. 650 VGPRs of spill
template <typename R, int M> constexpr int ff_waves_per_simd() { return (sizeof(R) == 4 || M == 2) ? 2 : 1; }

template <typename P, int KIND, int M>
__global__ __launch_bounds__(64, (ff_waves_per_simd<typename P::R, M>())) void sdsp_filtfilt_fused_kernel(ff_dev_args<typename P::S, typename P::R, M> p)
{
    using S = typename P::S;
    using R = typename P::R;
    extern __shared__ __attribute__((aligned(16))) unsigned char sdsp_filtfilt_smem[];
    const int lane = threadIdx.x;
    const uint64_t ch0 = (uint64_t)blockIdx.x * 64;
    const uint64_t my_ch = ch0 + lane;
    const bool have_ch = my_ch < p.channels;
    const uint64_t L = p.samples;
    const uint32_t pad = p.padlen;
    // lanes without a channel run the recurrence on zeros and store nothing to the rows (they take part in the transpose)
    const S *row = p.data + (have_ch ? my_ch : 0) * p.stride;
    S *ws = p.ws + (uint64_t)blockIdx.x * 64 * pad + lane; // element i at ws[64 i]

    // prologue: the right-edge extension inputs, before the forward pass overwrites the row's end
    const S x0 = have_ch ? row[0] : S(0), xl = have_ch ? row[L - 1] : S(0);
    for (uint32_t i = 0; i < pad; i++)
        ws[64 * (uint64_t)i] = extend<S>(p.padtype, xl, have_ch ? row[L - 2 - i] : S(0));

    // forward over the left extension: state only
    R y1[M + 1], y2[M + 1], y3[M + 1];
    steady_state<R, M>(p, (R)(pad ? extend<S>(p.padtype, x0, have_ch ? row[pad] : S(0)) : x0), y1, y2, y3);
    for (uint32_t i = 0; i < pad; i++)
        (void)cascade_step<R, KIND, M, P::fused>((R)extend<S>(p.padtype, x0, have_ch ? row[pad - i] : S(0)), p, y1, y2, y3);

    // forward over the row, then over the right extension in the workspace
    tile_pass<P, KIND, M, false, true, false, 4>(p, sdsp_filtfilt_smem, ch0, y1, y2, y3);
    for (uint32_t i = 0; i < pad; i++)
        ws[64 * (uint64_t)i] = (S)cascade_step<R, KIND, M, P::fused>((R)ws[64 * (uint64_t)i], p, y1, y2, y3);

    // backward from the last forward output (y1[M] is its unrounded value): the workspace, then the row, last tile first
    steady_state<R, M>(p, (R)(S)y1[M], y1, y2, y3);
    for (uint32_t i = pad; i-- > 0;)
        (void)cascade_step<R, KIND, M, P::fused>((R)ws[64 * (uint64_t)i], p, y1, y2, y3);
    tile_pass<P, KIND, M, true, false, true, 4>(p, sdsp_filtfilt_smem, ch0, y1, y2, y3);
}

template <typename P, int M> ff_dev_args<typename P::S, typename P::R, M> make_ff_args(const filtfilt_args &a)
{
    using R = typename P::R;
    ff_dev_args<typename P::S, R, M> p;
    p.data = reinterpret_cast<typename P::S *>(a.data);
    p.ws = reinterpret_cast<typename P::S *>(a.ws);
    p.channels = a.channels;
    p.samples = a.samples;
    p.stride = a.stride;
    p.padlen = a.padlen;
    p.padtype = a.padtype;
    p.gain = (R)a.gain;
    for (int j = 0; j < M; j++) {
        p.a1[j] = (R)a.a1[j];
        p.a2[j] = (R)a.a2[j];
        p.b1[j] = (R)a.b1[j];
        p.b2[j] = (R)a.b2[j];
    }
    for (int j = 0; j <= M; j++)
        p.ss[j] = (R)a.ss[j];
    return p;
}

// ---- selection: ONE function, used by the launcher and by the plan info.  Variant 0: the fused kernel for up to 8 sections
// on 16-byte aligned rows (data pointer and stride), the direct kernel otherwise (10 .. 16 sections: correct, not tuned, as in
// the IIR bank); variant 1: the direct kernel always.
enum ff_kernel_id { FF_K_FUSED, FF_K_DIRECT, FF_K_BAD };

ff_kernel_id ff_select(int precision, const filtfilt_args &a, int variant)
{
    const size_t ss = precision == SDSP_HIP_F64 ? 8 : 4;
    const bool aligned = (uintptr_t)a.data % 16 == 0 && (a.channels <= 1 || (a.stride * ss) % 16 == 0);
    switch (variant) {
    case 0: return (a.sections <= 8 && aligned) ? FF_K_FUSED : FF_K_DIRECT;
    case 1: return FF_K_DIRECT;
    default: return FF_K_BAD;
    }
}

template <typename P, int KIND, int M> int launch_ff_km(const filtfilt_args &a, ff_kernel_id id, hipStream_t stream)
{
    const auto p = make_ff_args<P, M>(a);
    const uint64_t blocks = id == FF_K_DIRECT ? (a.channels + 255) / 256 : (a.channels + 63) / 64;
    if (blocks > 0x7fffffffull)
        return fail(SDSP_HIP_ERR_UNSUPPORTED, "too many channels for one launch");
    if (id == FF_K_FUSED) {
        if constexpr (M <= 8)
            hipLaunchKernelGGL((sdsp_filtfilt_fused_kernel<P, KIND, M>), dim3((uint32_t)blocks), dim3(64), 64 * (128 + 16), stream, p);
        else
            return fail(SDSP_HIP_ERR_UNSUPPORTED, "the fused filtfilt kernel is built for up to 8 sections");
    } else {
        hipLaunchKernelGGL((sdsp_filtfilt_direct_kernel<P, KIND, M>), dim3((uint32_t)blocks), dim3(256), 0, stream, p);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(SDSP_HIP_ERR_HIP, std::string("filtfilt launch: ") + hipGetErrorString(e));
    return SDSP_HIP_OK;
}

template <typename P, int KIND> int launch_ff_k(const filtfilt_args &a, ff_kernel_id id, hipStream_t stream)
{
    switch (a.sections) {
    case 2: return launch_ff_km<P, KIND, 2>(a, id, stream);
    case 4: return launch_ff_km<P, KIND, 4>(a, id, stream);
    case 6: return launch_ff_km<P, KIND, 6>(a, id, stream);
    case 8: return launch_ff_km<P, KIND, 8>(a, id, stream);
    case 10: return launch_ff_km<P, KIND, 10>(a, id, stream);
    case 12: return launch_ff_km<P, KIND, 12>(a, id, stream);
    case 14: return launch_ff_km<P, KIND, 14>(a, id, stream);
    case 16: return launch_ff_km<P, KIND, 16>(a, id, stream);
    default: return fail(SDSP_HIP_ERR_UNSUPPORTED, "sections must be even and at most 16");
    }
}

template <typename P> int launch_ff_r(const filtfilt_args &a, ff_kernel_id id, hipStream_t stream)
{
    switch (a.kind) {
    case SDSP_HIP_IIR_GENERIC: return launch_ff_k<P, SDSP_HIP_IIR_GENERIC>(a, id, stream);
    case SDSP_HIP_IIR_LP: return launch_ff_k<P, SDSP_HIP_IIR_LP>(a, id, stream);
    case SDSP_HIP_IIR_HP: return launch_ff_k<P, SDSP_HIP_IIR_HP>(a, id, stream);
    case SDSP_HIP_IIR_BP: return launch_ff_k<P, SDSP_HIP_IIR_BP>(a, id, stream);
    default: return fail(SDSP_HIP_ERR_INVALID_ARG, "unknown IIR kind");
    }
}
} // namespace

int launch_filtfilt(int precision, const filtfilt_args &a, int variant, void *stream)
{
    if (a.channels == 0)
        return SDSP_HIP_OK;
    if (a.samples <= a.padlen)
        return fail(SDSP_HIP_ERR_INVALID_SIZE, "samples must be larger than padlen");
    if (a.padlen && !a.ws)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "a padded call needs the plan's workspace");
    const ff_kernel_id id = ff_select(precision, a, variant);
    if (id == FF_K_BAD)
        return fail(SDSP_HIP_ERR_INVALID_ARG, "unknown filtfilt kernel variant");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (precision == SDSP_HIP_F32_F64STATE)
        return launch_ff_r<prec_mix>(a, id, s);
    return precision == SDSP_HIP_F64 ? launch_ff_r<prec_f64>(a, id, s) : launch_ff_r<prec_f32>(a, id, s);
}

const char *filtfilt_kernel_for(int precision, const filtfilt_args &a, int variant)
{
    switch (ff_select(precision, a, variant)) {
    case FF_K_FUSED: return "sdsp_filtfilt_fused_kernel";
    case FF_K_DIRECT: return "sdsp_filtfilt_direct_kernel";
    default: return "none";
    }
}
} // namespace sdsp_hip
