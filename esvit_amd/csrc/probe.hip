// Class-index cross-entropy of the linear-probe sweep (eval_linear.py:262, F.cross_entropy on the classifier's logits), for G
// classifiers that share one feature batch: the logits [B, G*C] are Rs = B*G rows of K = C fp32, row r = (sample r / G, member
// r % G).  Entered through esvit_dino_ce_fwd_bwd with terms = 0 (dino_loss.hip dispatches here).  Per row:
//   row_loss[2r]     = lse(z) - z_t
//   row_loss[2r + 1] = rank of the target in the stable descending order = #{j : z_j > z_t} + #{j < t : z_j == z_t}
//                      (a count: exact as a float for C < 2^24; a top-k hit is rank < k)
//   ds[r, j]         = row_w[r] (softmax(z)_j - [j == t])                (ds may be s: in place; ds may be NULL: nothing written)
// A row with a NaN / inf logit (or a target outside [0, C)) gives loss NaN, rank C and a NaN gradient row -- the row's member then
// fails the update's per-member guard -- and touches nothing else: rows never share a reduction.
//
// Two strategies, chosen by the row length:
//   K <= PROBE_REG_ROW_MAX  one WAVE per row, the row read once into registers (16-byte loads), max / sum / count reduced across the
//                           wave with DPP row steps and two cross-row exchanges, no LDS, no barrier;
//   longer rows             one 256-thread WORKGROUP per row, three sweeps over the row (max + rank, sum, gradient): the second and
//                           third come from cache (a 32768-class row is 128 KiB).
// Every reduction has a fixed order and there are no atomics: identical launches give identical bits.
#include <math.h>

#include "common.h"
#include "../../include/esvit_hip.h"

namespace {

constexpr int PROBE_REG_ROW_MAX = 4096;  // longest row kept in registers: 64 lanes x 16 vectors x 4 floats
constexpr int PROBE_NT = 256;

// max over the 16 lanes of a DPP row (as row16_sum of common.h)
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true)));
    return v;
}
__device__ __forceinline__ float wave_max_dpp(float v) {
    v = row16_max(v);
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = row16_sum(v);
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.0e38f; }  // false for NaN and +-inf

// rank contribution of column j holding v, against the target (column t, value zt)
__device__ __forceinline__ int ahead(float v, int j, float zt, int t) { return (v > zt || (v == zt && j < t)) ? 1 : 0; }

// ---- rows of up to 256 * NV floats: one wave per row, the row in NV 16-byte registers per lane ----
template <int NV>
__global__ __launch_bounds__(PROBE_NT) void probe_ce_wave_kernel(const float* s, const int* __restrict__ target,
                                                                 const float* __restrict__ row_w, long Rs, int K,
                                                                 float* __restrict__ row_loss, float* ds) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * (PROBE_NT / 64) + (threadIdx.x >> 6);
    if (r >= Rs) return;  // (whole waves leave: no barrier follows)
    const float* z = s + r * K;
    const int t = target[r];
    const bool t_ok = t >= 0 && t < K;
    const float zt = t_ok ? z[t] : 0.f;  // read before any store of this row (ds may be s)
    f32x4 v[NV];
    float m = -INFINITY;
    int bad = t_ok ? 0 : 1, cnt = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = (i * 64 + lane) * 4;
        if (j < K) {  // K % 4 == 0: a vector is inside the row or outside it
            v[i] = *reinterpret_cast<const f32x4*>(z + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bad |= !finite_f(v[i][e]);
                m = fmaxf(m, v[i][e]);
                cnt += ahead(v[i][e], j + e, zt, t);
            }
        } else {
            v[i] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
    }
    const bool row_bad = __any(bad);
    m = wave_max_dpp(m);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[i][e] = expf(v[i][e] - m);  // (the padding: exp(-inf) = 0)
            sum += v[i][e];
        }
    sum = wave_sum_dpp(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) {
        row_loss[2 * r] = row_bad ? NAN : (logf(sum) + m) - zt;
        row_loss[2 * r + 1] = (float)(row_bad ? K : cnt);
    }
    if (ds == nullptr) return;
    const float w = row_w[r], inv = 1.f / sum;
    float* d = ds + r * K;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = (i * 64 + lane) * 4;
        if (j < K) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = row_bad ? NAN : w * (v[i][e] * inv - (j + e == t ? 1.f : 0.f));
            *reinterpret_cast<f32x4*>(d + j) = o;
        }
    }
}

// ---- longer rows: one workgroup per row, three sweeps ----
__global__ __launch_bounds__(PROBE_NT) void probe_ce_block_kernel(const float* s, const int* __restrict__ target,
                                                                  const float* __restrict__ row_w, int K, float* __restrict__ row_loss,
                                                                  float* ds) {
    __shared__ float scratch[PROBE_NT / 64];
    __shared__ int iscratch[PROBE_NT / 64];
    const long r = blockIdx.x;
    const float* z = s + r * K;
    const int t = target[r];
    const bool t_ok = t >= 0 && t < K;
    const float zt = t_ok ? z[t] : 0.f;
    float m = -INFINITY;
    int bad = t_ok ? 0 : 1, cnt = 0;
    for (int j = threadIdx.x * 4; j < K; j += PROBE_NT * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bad |= !finite_f(v[e]);
            m = fmaxf(m, v[e]);
            cnt += ahead(v[e], j + e, zt, t);
        }
    }
    const bool row_bad = __syncthreads_or(bad) != 0;
    m = block_max<PROBE_NT>(m, scratch);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) iscratch[threadIdx.x >> 6] = cnt;
    float sum = 0.f;
    for (int j = threadIdx.x * 4; j < K; j += PROBE_NT * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + j);
        sum += (expf(v[0] - m) + expf(v[1] - m)) + (expf(v[2] - m) + expf(v[3] - m));
    }
    sum = block_sum<PROBE_NT>(sum, scratch);  // (its barriers also order every read of the row above before the stores below)
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < PROBE_NT / 64; ++i) c += iscratch[i];
        row_loss[2 * r] = row_bad ? NAN : (logf(sum) + m) - zt;
        row_loss[2 * r + 1] = (float)(row_bad ? K : c);
    }
    if (ds == nullptr) return;
    const float w = row_w[r], inv = 1.f / sum;
    float* d = ds + r * K;
    for (int j = threadIdx.x * 4; j < K; j += PROBE_NT * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + j);  // (in place: this thread's own vector, read before it is written)
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = row_bad ? NAN : w * (expf(v[e] - m) * inv - (j + e == t ? 1.f : 0.f));
        *reinterpret_cast<f32x4*>(d + j) = o;
    }
}

}  // namespace

int64_t esvit_i_probe_ce_reg_row() { return PROBE_REG_ROW_MAX; }  // esvit_query

// the terms = 0 mode of esvit_dino_ce_fwd_bwd (arguments already checked there)
int esvit_i_probe_ce(const float* s, const int32_t* target, const float* row_w, int64_t Rs, int K, float* row_loss, float* ds,
                     hipStream_t stream) {
    if (K <= PROBE_REG_ROW_MAX) {
        const dim3 grid((unsigned)((Rs + PROBE_NT / 64 - 1) / (PROBE_NT / 64))), block(PROBE_NT);
#define PROBE_LAUNCH(NV) hipLaunchKernelGGL(probe_ce_wave_kernel<NV>, grid, block, 0, stream, s, target, row_w, (long)Rs, K, row_loss, ds)
        if (K <= 256) PROBE_LAUNCH(1);
        else if (K <= 512) PROBE_LAUNCH(2);
        else if (K <= 1024) PROBE_LAUNCH(4);
        else if (K <= 2048) PROBE_LAUNCH(8);
        else PROBE_LAUNCH(16);
#undef PROBE_LAUNCH
    } else {
        hipLaunchKernelGGL(probe_ce_block_kernel, dim3((unsigned)Rs), dim3(PROBE_NT), 0, stream, s, target, row_w, K, row_loss, ds);
    }
    ESVIT_CHECK_LAUNCH("dino_ce_fwd_bwd(class index)");
    return ESVIT_OK;
}
