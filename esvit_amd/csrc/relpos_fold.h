// The relative-position table's gradient WITHOUT atomics, from frag-layout slabs [parts][nH][nt * nt * 256] (one definition for the
// finish of the fused C = 96 branch backward, attn_branch_bwd.hip, and for esvit_relpos_bias_bwd | ESVIT_RELPOS_ORDERED, window_attn.hip).
// Two launches: the slabs [0, parts) are summed in slab order, element by element, INTO slab 0 (each element is read and written by
// one thread only; slabs 1.. are not written); then table row t, head h gathers its (query, key) pairs from that sum in ascending
// (query, key) order -- one accumulator, one writer per table element, no dependence on the grid's schedule: identical launches give
// identical bits.
// nt = 16-key tiles per window side (4 for <= 64 tokens, 14 for 14 x 14): element of (q, key) within a head is
// (((key / 16) * nt + q / 16) * 64 + ((key % 16) / 4) * 16 + q % 16) * 4 + key % 4.
#pragma once
#include "common.h"

namespace {

// grid: ceil(total / 256) x 256 threads; total = nH * nt * nt * 256 = the slab stride
__global__ __launch_bounds__(256) void relpos_ordered_fold_kernel(float* __restrict__ dbias, int parts, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float* p = dbias + i;
    float s = 0.f;
    int b = 0;
    for (; b + 8 <= parts; b += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(long)(b + k) * total];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; b < parts; ++b) s += p[(long)b * total];
    p[0] = s;
}

constexpr int RELPOS_LIST = 1024;  // pairs of one table row held in LDS at a time (a Swin row has at most N <= 224)

// grid: table_rows x 256 threads.  The flat index [N * N] is cut into 256 contiguous segments, one per thread: a count pass, an
// exclusive prefix over the threads, then the offsets of the row's pairs are listed in LDS in flat (= ascending (query, key)) order,
// RELPOS_LIST at a time, and thread h walks the list with one accumulator.  index may hold anything: entries outside [0, table_rows)
// match no row, a row may own any number of pairs.
__global__ __launch_bounds__(256) void relpos_ordered_table_kernel(const float* __restrict__ folded, const long* __restrict__ index, int N, int nt,
                                                                   int nH, float* __restrict__ dtable, int accumulate) {
    __shared__ int list[RELPOS_LIST];
    __shared__ int wave_base[4];
    __shared__ int total_sh;
    const int t = blockIdx.x, tid = threadIdx.x;
    const int nn = N * N;
    const int seg = (nn + 255) / 256;
    const int lo = min(tid * seg, nn), hi = min(lo + seg, nn);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += index[i] == t;
    // exclusive prefix of cnt over the 256 threads: inclusive scan inside the wave, then the waves' totals
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if ((tid & 63) >= o) inc += v;
    }
    if ((tid & 63) == 63) wave_base[tid >> 6] = inc;
    __syncthreads();
    if (tid == 0) {
        int a = 0;
        for (int w = 0; w < 4; ++w) {
            const int v = wave_base[w];
            wave_base[w] = a;
            a += v;
        }
        total_sh = a;
    }
    __syncthreads();
    const int first = wave_base[tid >> 6] + inc - cnt;  // list position of this thread's first pair
    const int total = total_sh;
    const int fe = nt * nt * 256;
    for (int h0 = 0; h0 < nH; h0 += 256) {
        const int h = h0 + tid;
        float s = 0.f;
        for (int r0 = 0; r0 < total; r0 += RELPOS_LIST) {
            __syncthreads();  // (the list of the previous round has been read)
            if (cnt > 0 && first < r0 + RELPOS_LIST && first + cnt > r0) {
                int pos = first;
                for (int i = lo; i < hi; ++i)
                    if (index[i] == t) {
                        if (pos >= r0 && pos < r0 + RELPOS_LIST) {
                            const int q = i / N, key = i - q * N;
                            list[pos - r0] = (((key >> 4) * nt + (q >> 4)) * 64 + ((key & 15) >> 2) * 16 + (q & 15)) * 4 + (key & 3);
                        }
                        ++pos;
                    }
            }
            __syncthreads();
            if (h < nH) {
                const float* f = folded + (long)h * fe;
                const int n = min(RELPOS_LIST, total - r0);
                int k = 0;
                for (; k + 8 <= n; k += 8) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = f[list[k + j]];
#pragma unroll
                    for (int j = 0; j < 8; ++j) s += v[j];
                }
                for (; k < n; ++k) s += f[list[k]];
            }
        }
        if (h < nH) {
            float* d = dtable + (long)t * nH + h;
            *d = accumulate ? *d + s : s;
        }
    }
}

// fold + gather on `stream`; slab 0 of dbias_ws holds the sum afterwards
inline void relpos_ordered_launch(float* dbias_ws, int parts, int nt, const int64_t* index, int N, int nH, int table_rows, float* dtable,
                                  int accumulate, hipStream_t stream) {
    const long total = (long)nH * nt * nt * 256;
    hipLaunchKernelGGL(relpos_ordered_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, dbias_ws, parts, total);
    hipLaunchKernelGGL(relpos_ordered_table_kernel, dim3(table_rows), dim3(256), 0, stream, (const float*)dbias_ws, (const long*)index, N, nt, nH,
                       dtable, accumulate);
}

}  // namespace
