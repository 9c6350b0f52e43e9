// stream_carry.hip -- the carried-state kernels of the streaming banks: what a call leaves for the next one.
// They only move elements of 4, 8 or 16 bytes (a real or an interleaved complex sample of either precision), so every bank with
// that kind of state launches these and no copy of its own.
//
//   carry_history  the banks that read a history in front of the block (STFT, Welch, both channelizer kinds), after the call's last
//                  frame launch: state[c hist + j] = x[hist + S - 1 - j], newest first, x = old history followed by the block.  For
//                  S >= hist every value comes from `in` (sdsp_carry_history_flat).  For S < hist the row is the block reversed
//                  followed by the old state[0 .. hist - S): an in-place shift toward higher indices, done by one workgroup per row
//                  walking chunks from the high end down with a barrier between each chunk's reads and its writes
//                  (sdsp_carry_history_shift).
//   carry_seed     the banks that carry pending sums behind the block (inverse STFT, both synthesis kinds), before the call's first
//                  slice: the old pending sums P[0 .. min(hist, S)) go to out; for S < hist the rest, P[S .. hist), moves down to the
//                  start of the state row in place (one workgroup per row, chunks walked from the low end up with a barrier between
//                  each chunk's reads and its writes: the mirror of the history shift).  Afterwards every pending sum sits where
//                  its position lives (sdsp_carry_seed).
#include "stream_dev.h"

namespace sdsp_hip
{
namespace
{
// S >= hist: the new history is the block's last hist elements, newest first
template <typename E>
__global__ __launch_bounds__(kThreads) void sdsp_carry_history_flat(const E *__restrict__ in, E *__restrict__ state, uint64_t in_stride,
                                                                    uint64_t samples, uint64_t channels, uint32_t hist)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= channels * hist)
        return;
    const uint64_t c = i / hist, jj = i - c * hist;
    state[i] = in[c * in_stride + (samples - 1 - jj)];
}

// S < hist: one workgroup per row; chunk [lo, lo + kThreads) reads old state[j - S] (j >= S) or the block, waits for every lane's
// read, then writes.  Chunks go from the high end down, so every old value a chunk reads lies below the chunks written before it.
template <typename E>
__global__ __launch_bounds__(kThreads) void sdsp_carry_history_shift(const E *__restrict__ in, E *state, uint64_t in_stride,
                                                                     uint32_t samples, uint32_t hist)
{
    const uint64_t c = blockIdx.x;
    E *row = state + c * hist;
    const uint32_t chunks = (hist + kThreads - 1) / kThreads;
    for (uint32_t q = chunks; q-- > 0;) {
        const uint32_t jj = q * kThreads + threadIdx.x;
        E val = E(0);
        if (jj < hist)
            val = jj < samples ? in[c * in_stride + (samples - 1 - jj)] : row[jj - samples];
        __syncthreads();
        if (jj < hist)
            row[jj] = val;
        __syncthreads();
    }
}

template <typename E>
__global__ __launch_bounds__(kThreads) void sdsp_carry_seed(E *__restrict__ out, E *state, uint64_t out_stride, uint64_t samples,
                                                            uint32_t hist)
{
    const uint64_t c = blockIdx.x;
    E *row = state + c * hist;
    const uint32_t m = samples < hist ? static_cast<uint32_t>(samples) : hist;
    for (uint32_t i = threadIdx.x; i < m; i += kThreads)
        out[c * out_stride + i] = row[i];
    if (samples >= hist)
        return;
    __syncthreads(); // every read of row[0 .. m) above happens before the shift writes there
    const uint32_t s = static_cast<uint32_t>(samples), keep = hist - s;
    const uint32_t chunks = (keep + kThreads - 1) / kThreads;
    for (uint32_t q = 0; q < chunks; q++) { // low to high: a chunk reads only above every index written before it
        const uint32_t i = q * kThreads + threadIdx.x;
        E val = E(0);
        if (i < keep)
            val = row[i + s];
        __syncthreads();
        if (i < keep)
            row[i] = val;
        __syncthreads();
    }
}

template <typename E>
int history(const void *in_v, uint64_t in_stride, void *state_v, uint64_t channels, uint64_t samples, uint32_t hist, hipStream_t stream,
            const std::string &what)
{
    const E *in = static_cast<const E *>(in_v);
    E *state = static_cast<E *>(state_v);
    dim3 grid;
    if (samples >= hist) {
        if (int rc = grid_for(channels * hist, what.c_str(), &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_carry_history_flat<E>, grid, dim3(kThreads), 0, stream, in, state, in_stride, samples, channels, hist);
    } else {
        if (int rc = grid_of_blocks(channels, what.c_str(), &grid))
            return rc;
        hipLaunchKernelGGL(sdsp_carry_history_shift<E>, grid, dim3(kThreads), 0, stream, in, state, in_stride,
                           static_cast<uint32_t>(samples), hist);
    }
    return SDSP_HIP_OK;
}

template <typename E>
int seed(void *out, uint64_t out_stride, void *state, uint64_t channels, uint64_t samples, uint32_t hist, hipStream_t stream,
         const std::string &what)
{
    dim3 grid;
    if (int rc = grid_of_blocks(channels, what.c_str(), &grid))
        return rc;
    hipLaunchKernelGGL(sdsp_carry_seed<E>, grid, dim3(kThreads), 0, stream, static_cast<E *>(out), static_cast<E *>(state), out_stride,
                       samples, hist);
    return SDSP_HIP_OK;
}

// f(a value of the element type of `elem_bytes` bytes in `precision`): the real or its interleaved pair
template <typename F> int with_element(int precision, uint32_t elem_bytes, F f)
{
    const bool f64 = precision == SDSP_HIP_F64;
    if (elem_bytes == 2u) // one 16-bit integer sample (the CIC banks' real I16 rows); their wider elements move as the f32 ones do
        return f(uint16_t());
    if (elem_bytes == (f64 ? 8u : 4u))
        return f64 ? f(double()) : f(float());
    if (elem_bytes == (f64 ? 16u : 8u))
        return f64 ? f(cplx_pair<double>::type()) : f(cplx_pair<float>::type());
    return fail(SDSP_HIP_ERR_INVALID_ARG, "carried state: element size is not one real or one complex value of the precision");
}
} // namespace

int carry_history(int precision, uint32_t elem_bytes, const void *in, uint64_t in_stride, void *state, uint64_t channels,
                  uint64_t samples, uint32_t hist, void *stream, const char *family)
{
    if (hist == 0 || !state || channels == 0)
        return SDSP_HIP_OK;
    const std::string what = std::string(family) + " state";
    if (int rc = with_element(precision, elem_bytes, [&](auto e) {
            return history<decltype(e)>(in, in_stride, state, channels, samples, hist, static_cast<hipStream_t>(stream), what);
        }))
        return rc;
    return launch_status(family);
}

int carry_seed(int precision, uint32_t elem_bytes, void *out, uint64_t out_stride, void *state, uint64_t channels, uint64_t samples,
               uint32_t hist, void *stream, const char *family)
{
    if (hist == 0 || !state || channels == 0)
        return SDSP_HIP_OK;
    const std::string what = std::string(family) + " state";
    if (int rc = with_element(precision, elem_bytes, [&](auto e) {
            return seed<decltype(e)>(out, out_stride, state, channels, samples, hist, static_cast<hipStream_t>(stream), what);
        }))
        return rc;
    return launch_status(family);
}
} // namespace sdsp_hip
