// Distribution statistics of softmax rows (the training-health monitor, esvit_amd/monitor.py).  Entered through
// esvit_dino_ce_fwd_bwd with terms = -1 (dino_loss.hip dispatches here).  For rows x [R, K] with an optional centre c [K], an inverse
// temperature and the rows' KNOWN statistics row_max[r] = max_k z, row_lse[r] = ln sum_k exp(z - max) of z = (x - c) * inv_temp (the
// outputs of esvit_teacher_row_stats / esvit_rowstat_combine), with p = softmax(z), d = z - max, L = row_lse:
//   out[2r]     = H(p_r) = L - sum_k p_k d_k          (nats; every term of the sum has one sign: no cancellation against a large max)
//   out[2r + 1] = the lowest index of the maximal z   (as a float: exact for K < 2^24)
//   psum[k]     = sum_r p_rk                          (fp32)
// One read of x: a workgroup owns a SLAB of DIST_SLAB rows and sweeps a block of DIST_COLS columns, a thread taking the same 16-byte
// vector of every row of the slab.  The per-row partials (sum p d, best x - c, its index) stay in registers across the sweep and are
// reduced over the workgroup once, at the end, into one record per (row, column block); the per-column sums of the slab need no
// reduction at all (a thread owns its columns) and go to the fp32 workspace ws [nslabs, K].  A second, small kernel (one workgroup per
// slab) folds a row's records in column-block order into H and the index, and esvit_partial_reduce folds the slabs' column sums in
// a fixed order -- the two-stage pattern of esvit_colsum.  The workspace traffic is 2 * K * 4 bytes per slab against
// DIST_SLAB * K * 2 bytes of bf16 rows: 12.5 %.  No atomics: identical launches give identical bits.
// (Rows longer than DIST_COLS are swept by several workgroups, one per block of DIST_COLS columns.  Shorter blocks were measured and
// lose: at [12544, 65536] bf16 blocks of 8192 columns take 0.72 ms against 0.60 ms for whole rows -- the reduction at the end of a
// workgroup and the fill of its load pipeline are paid per block.  profiles/monitor_bench.json.)
// Per logit: one subtraction (the centre comes off BEFORE the scaling, see dino_ce_kernel), d by one FMA, p by one v_exp_f32 fed by
// one FMA of d (so the exponent's rounding is at the size of d and L, not of max), one FMA into sum p d, one add into the column sum;
// the argmax costs a maximum per logit and one comparison per vector.
// A row whose statistics or logits are NaN / inf gives H = NaN and index -1, and every column sum becomes NaN (the second kernel
// overwrites the slab's workspace row); the row outputs of every other row are what they would have been.
#include <math.h>

#include "common.h"
#include "../../include/esvit_hip.h"

namespace {

constexpr int DIST_NT = 256;
constexpr int DIST_SLAB = 32;
constexpr int DIST_GROUP = 8;  // rows whose loads are in flight together (twice that while a group is worked on)
constexpr int DIST_COLS = 65536;  // columns of one workgroup: the whole row up to the 65536 of the reference's heads (32 sweeps of bf16)

template <typename T>
__global__ __launch_bounds__(DIST_NT) void dist_stats_kernel(const T* __restrict__ x, const float* __restrict__ center,
                                                             const float* __restrict__ row_max, const float* __restrict__ row_lse,
                                                             float inv_temp, long R, int K, f32x4* __restrict__ rec, float* __restrict__ ws) {
    constexpr int V = Vec16<T>::N;
    constexpr int NW = DIST_NT / 64;
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ float sm_pd[NW][DIST_SLAB];
    __shared__ float sm_best[NW][DIST_SLAB];
    __shared__ int sm_idx[NW][DIST_SLAB];
    const int k_end = min(K, ((int)blockIdx.y + 1) * DIST_COLS);
    const long r0 = (long)blockIdx.x * DIST_SLAB;
    const int nrows = (int)min((long)DIST_SLAB, R - r0);
    const T* xs = x + r0 * K;
    float* wrow = ws + (long)blockIdx.x * K;

    float pd[DIST_SLAB], best[DIST_SLAB];
    int bidx[DIST_SLAB];
#pragma unroll
    for (int i = 0; i < DIST_SLAB; ++i) {
        pd[i] = 0.f;
        best[i] = -INFINITY;
        bidx[i] = 0x7fffffff;
    }
    for (int k = (int)blockIdx.y * DIST_COLS + threadIdx.x * V; k < k_end; k += DIST_NT * V) {
        float cv[V], cs[V];
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const f32x4 c4 = center ? *reinterpret_cast<const f32x4*>(center + k + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cv[4 * q + e] = c4[e];
                cs[4 * q + e] = 0.f;
            }
        }
        // one row's vector: d by one FMA, p by one v_exp_f32 fed by one FMA of d, the running argmax by a maximum per logit
        auto row = [&](int i, const Vec16<T>& v) __attribute__((always_inline)) {
            const float mx = row_max[r0 + i];
            const float nl = -row_lse[r0 + i] * LOG2E;
            float y[V];
            float m = -INFINITY;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                y[e] = v.get(e) - cv[e];
                m = fmaxf(m, y[e]);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float d = fmaf(y[e], inv_temp, -mx);
                const float p = __builtin_amdgcn_exp2f(fmaf(d, LOG2E, nl));
                pd[i] = fmaf(p, d, pd[i]);
                cs[e] += p;
            }
            if (m > best[i]) {  // (rare after the first sweeps; the columns of a thread come in rising order: > keeps the lowest)
                best[i] = m;
                int j = V - 1;
#pragma unroll
                for (int e = V - 2; e >= 0; --e) j = y[e] == m ? e : j;
                bidx[i] = k + j;
            }
        };
        if (nrows == DIST_SLAB) {
            // a whole slab: the loads of the next DIST_GROUP rows are issued before the current group is worked on (the argmax branch
            // ends a basic block per row: left to the compiler, one 16-byte load per wave would be in flight)
            Vec16<T> v[2][DIST_GROUP];
#pragma unroll
            for (int j = 0; j < DIST_GROUP; ++j) v[0][j] = ld16<T>(xs + (long)j * K + k);
#pragma unroll
            for (int g = 0; g < DIST_SLAB / DIST_GROUP; ++g) {
                if (g + 1 < DIST_SLAB / DIST_GROUP) {
#pragma unroll
                    for (int j = 0; j < DIST_GROUP; ++j) v[(g + 1) & 1][j] = ld16<T>(xs + (long)((g + 1) * DIST_GROUP + j) * K + k);
                }
#pragma unroll
                for (int j = 0; j < DIST_GROUP; ++j) row(g * DIST_GROUP + j, v[g & 1][j]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < DIST_SLAB; ++i)
                if (i < nrows) row(i, ld16<T>(xs + (long)i * K + k));  // (uniform: the last, partly filled slab)
        }
#pragma unroll
        for (int q = 0; q < V / 4; ++q) *reinterpret_cast<f32x4*>(wrow + k + 4 * q) = f32x4{cs[4 * q], cs[4 * q + 1], cs[4 * q + 2], cs[4 * q + 3]};
    }

    // one reduction per row: lanes by shuffles, then the waves through LDS in a fixed order
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < DIST_SLAB; ++i) {
        float s = pd[i], b = best[i];
        int j = bidx[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            const float b2 = __shfl_xor(b, o, 64);
            const int j2 = __shfl_xor(j, o, 64);
            const bool take = b2 > b || (b2 == b && j2 < j);
            b = take ? b2 : b;
            j = take ? j2 : j;
        }
        if (l == 0) {
            sm_pd[w][i] = s;
            sm_best[w][i] = b;
            sm_idx[w][i] = j;
        }
    }
    __syncthreads();
    if (threadIdx.x < nrows) {
        const int i = threadIdx.x;
        float s = sm_pd[0][i], b = sm_best[0][i];
        int j = sm_idx[0][i];
#pragma unroll
        for (int u = 1; u < NW; ++u) {
            s += sm_pd[u][i];
            const float b2 = sm_best[u][i];
            const int j2 = sm_idx[u][i];
            const bool take = b2 > b || (b2 == b && j2 < j);
            b = take ? b2 : b;
            j = take ? j2 : j;
        }
        rec[(r0 + i) * gridDim.y + blockIdx.y] = f32x4{s, b, (float)j, 0.f};  // (the index as a value: exact below 2^24, 2^31 = no column seen -- not as bits:
                                                                                // hipcc 7.2 folds a bit cast of element 2 of a loaded vector to element 0, cf. common.h: swap16)
    }
}

// rows of a slab from their records (sum p d, best x - c, its index), one per column block, folded in column-block order
__global__ __launch_bounds__(DIST_NT) void dist_rows_kernel(const f32x4* __restrict__ rec, int nblk, const float* __restrict__ row_max,
                                                            const float* __restrict__ row_lse, long R, int K, float* __restrict__ out,
                                                            float* __restrict__ ws) {
    __shared__ int sm_bad[DIST_SLAB];
    const long r0 = (long)blockIdx.x * DIST_SLAB;
    const int nrows = (int)min((long)DIST_SLAB, R - r0);
    if (threadIdx.x < DIST_SLAB) {
        const int i = threadIdx.x;
        int bad = 0;
        if (i < nrows) {
            const f32x4* p = rec + (r0 + i) * nblk;
            float s = 0.f, b = -INFINITY, j = 2147483648.f;
            for (int u = 0; u < nblk; ++u) {
                const f32x4 v = p[u];
                s += v[0];
                const bool take = v[1] > b || (v[1] == b && v[2] < j);
                b = take ? v[1] : b;
                j = take ? v[2] : j;
            }
            const float ent = row_lse[r0 + i] - s;
            // (an inf / NaN logit or statistic leaves sum p d inf or NaN: -inf * 0, inf * inf, NaN)
            bad = !(fabsf(ent) <= 3.0e38f) || !(fabsf(row_max[r0 + i]) <= 3.0e38f) || !(j < (float)K);
            out[2 * (r0 + i)] = bad ? NAN : ent;
            out[2 * (r0 + i) + 1] = bad ? -1.f : j;
        }
        sm_bad[i] = bad;
    }
    __syncthreads();
    int any_bad = 0;
#pragma unroll
    for (int i = 0; i < DIST_SLAB; ++i) any_bad |= sm_bad[i];
    if (any_bad) {  // (uniform) the slab's column sums: NaN, whatever the bad row left in them
        float* wrow = ws + (long)blockIdx.x * K;
        for (int k = threadIdx.x * 4; k < K; k += DIST_NT * 4) *reinterpret_cast<f32x4*>(wrow + k) = f32x4{NAN, NAN, NAN, NAN};
    }
}

}  // namespace

static inline long dist_slabs(long R) { return (R + DIST_SLAB - 1) / DIST_SLAB; }
static inline long dist_col_blocks(long K) { return (K + DIST_COLS - 1) / DIST_COLS; }

// esvit_query(ESVIT_Q_DIST_STATS, R, K): R = 0: the slab height; else the floats of the buffer the mode takes through `ds`:
// K column sums, one partial of K floats per slab, one record of 4 floats per (row, column block)
int64_t esvit_i_dist_stats_ws(int64_t R, int64_t K) {
    if (R == 0) return DIST_SLAB;
    if (R < 0 || K <= 0) return ESVIT_ERR_ARG;
    return (1 + dist_slabs(R)) * K + 4 * R * dist_col_blocks(K);
}

// the terms = -1 mode of esvit_dino_ce_fwd_bwd; buf: fp32, the extent esvit_i_dist_stats_ws answers
int esvit_i_dist_stats(int dtype, const void* x, const float* center, const float* row_max, const float* row_lse, float inv_temp, int64_t R,
                       int K, float* out, float* buf, hipStream_t stream) {
    const int nslabs = (int)dist_slabs(R), nblk = (int)dist_col_blocks(K);
    float* ws = buf + K;
    f32x4* rec = reinterpret_cast<f32x4*>(ws + (long)nslabs * K);
    const dim3 grid((unsigned)nslabs, (unsigned)nblk);
    if (dtype == ESVIT_BF16)
        hipLaunchKernelGGL(dist_stats_kernel<bf16>, grid, dim3(DIST_NT), 0, stream, (const bf16*)x, center, row_max, row_lse, inv_temp, (long)R, K,
                           rec, ws);
    else
        hipLaunchKernelGGL(dist_stats_kernel<float>, grid, dim3(DIST_NT), 0, stream, (const float*)x, center, row_max, row_lse, inv_temp, (long)R,
                           K, rec, ws);
    ESVIT_CHECK_LAUNCH("dino_ce_fwd_bwd(terms = -1)");
    hipLaunchKernelGGL(dist_rows_kernel, dim3((unsigned)nslabs), dim3(DIST_NT), 0, stream, rec, nblk, row_max, row_lse, (long)R, K, out, ws);
    ESVIT_CHECK_LAUNCH("dino_ce_fwd_bwd(terms = -1, rows)");
    return esvit_partial_reduce(ws, nslabs, K, K, buf, 0, stream);
}
