// thip_gemv_reduce.h -- the transpose-reduce butterfly of the dual GEMV kernels (thip_gemv.hip, thip_gemv_multi.hip): K per-lane
// values on 64 lanes -> the K wave-wide sums in K + 3 shuffles instead of 6 K.
#pragma once

#include "thip_common.h"

namespace {

template <int K, int O>
__device__ __forceinline__ void halve(float *v, int lane)
{
    const bool hi = (lane & O) != 0;
#pragma unroll
    for (int i = 0; i < K / 2; ++i) {
        const float send = hi ? v[i] : v[i + K / 2];
        const float keep = hi ? v[i + K / 2] : v[i];
        v[i] = keep + __shfl_xor(send, O, 64);
    }
}

// K per-lane values on 64 lanes -> the K wave-wide sums; the lanes with (lane & (64/K - 1)) == 0 and
// (lane >> (6 - log2 K)) == c hold sum c (in fact every lane of that group does)
template <int K>
__device__ __forceinline__ float multi_reduce(float *v, int lane)
{
    if constexpr (K == 8) {
        halve<8, 32>(v, lane); halve<4, 16>(v, lane); halve<2, 8>(v, lane);
        float r = v[0];
        r += __shfl_xor(r, 4, 64); r += __shfl_xor(r, 2, 64); r += __shfl_xor(r, 1, 64);
        return r;
    } else if constexpr (K == 4) {
        halve<4, 32>(v, lane); halve<2, 16>(v, lane);
        float r = v[0];
        r += __shfl_xor(r, 8, 64); r += __shfl_xor(r, 4, 64); r += __shfl_xor(r, 2, 64); r += __shfl_xor(r, 1, 64);
        return r;
    } else if constexpr (K == 2) {
        halve<2, 32>(v, lane);
        float r = v[0];
        r += __shfl_xor(r, 16, 64); r += __shfl_xor(r, 8, 64); r += __shfl_xor(r, 4, 64);
        r += __shfl_xor(r, 2, 64); r += __shfl_xor(r, 1, 64);
        return r;
    } else {
        return thip::wave_sum(v[0]);
    }
}

template <int K> struct Log2;
template <> struct Log2<1> { static constexpr int v = 0; };
template <> struct Log2<2> { static constexpr int v = 1; };
template <> struct Log2<4> { static constexpr int v = 2; };
template <> struct Log2<8> { static constexpr int v = 3; };

}  // namespace
