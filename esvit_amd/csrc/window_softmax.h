// The softmax of the window-attention kernels (window_attn.hip, window_attn_big.hip): over the keys of ONE query column of a transposed
// score strip.  p[i][jl] is the S^T tile of key tile i and query tile jl as the MFMA leaves it: lane (c, g) holds keys 16 i + 4 g + r of
// query column c, so a column's keys are this lane's NTL x 4 values and those of the lanes 16 and 32 away (two xor steps, no butterfly).
// The scores become probabilities in place.  Keys beyond N carry a bias of -1e30: their exponential is exactly zero.
#pragma once
#include "common.h"

struct ColSoftmax {
    float m, sum, inv;  // maximum, sum of exp(s - m), 1 / sum: the log-sum-exp is m + ln sum
    float ex;           // ENT: sum_k e_k x_k with x = s - m, e = exp(x): the entropy is H = ln sum - ex / sum (a key whose e is zero adds nothing)
};

template <bool ENT, int NTL, int NQ>
__device__ __forceinline__ ColSoftmax column_softmax(f32x4 (&p)[NTL][NQ], int jl) {
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, p[i][jl][r]);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f, ex = 0.f;
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float x = p[i][jl][r] - m;
            const float e = __expf(x);
            p[i][jl][r] = e;
            sum += e;
            if constexpr (ENT) ex += e * x;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if constexpr (ENT) {
        ex += __shfl_xor(ex, 16, 64);
        ex += __shfl_xor(ex, 32, 64);
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int i = 0; i < NTL; ++i) p[i][jl] *= inv;
    return ColSoftmax{m, sum, inv, ex};
}
