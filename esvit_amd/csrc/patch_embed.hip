// Fused Swin patch embedding (bf16 mode): Conv2d(3, E, 4, 4) + LayerNorm(E) of swin_transformer.py:531-547 straight from the fp32 NCHW
// images, one kernel each way.  The im2col matrix, the projection output y and dL/dy never exist in memory.
//
//   patch_embed_fwd_kernel    image -> x = LN(cols W^T + b) fp32 (+ mean, rstd per row when asked), any number of crop tensors per launch
//   patch_embed_bwd_kernel    persistent workgroups: recompute y per tile, LayerNorm backward in registers, dya rounded to bf16 where
//                             layernorm_bwd_to_act rounds it, dW += dya^T cols on the MFMA (tokens are its K), dbp, dgamma, dbeta in
//                             registers; one fp32 partial record [dW E x 48 | dbp | dgamma | dbeta] per workgroup
//   patch_embed_reduce_kernel the partial records summed in a fixed order (no atomics anywhere: identical launches, identical bits)
//
// A token's 48 columns keep the (c, ph, pw) order of im2col_kernel and are rounded to bf16 as there; K is padded to 64 with zeros (two
// k-steps of v_mfma_f32_16x16x32_bf16).  Lane (c, g) of a wave holds, for token c of a 16-token subtile, k = 32 ks + 8 g .. + 7: for
// ks = 0 that is channel g >> 1, patch rows 2 (g & 1) and + 1 (two 16-byte loads), for ks = 1 channel 2, rows 2 g and + 1 (g < 2).  The
// weight lives in LDS in fragment order, read once per workgroup.
//
// The forward forms y TRANSPOSED (A = weight, B = tokens): a lane ends with 4 consecutive channels of its token per 16-channel tile --
// 16-byte stores of x -- and the row statistics cross the four lane rows.  The backward forms y as it is (A = tokens, B = weight): a lane
// ends with ONE channel of 4 tokens per tile, so dgamma / dbeta / dbp cost E / 16 registers each, the row statistics are DPP row sums,
// and the rounded dya of two subtiles IS the A fragment of the weight gradient (frag_p_regs' token order); the columns come back from a
// per-wave LDS image with the same token permutation (frag_v_perm).
#include "common.h"
#include "mfma.h"
#include "../../include/esvit_hip.h"

namespace {

constexpr int PE_MAXC = ESVIT_PATCH_EMBED_MAX_CROPS;
constexpr int PE_K = 48;       // 3 x 4 x 4
constexpr int PE_FWD_T = 64;   // tokens per workgroup tile, forward (4 waves x 16)
constexpr int PE_BWD_T = 128;  // backward (4 waves x 2 subtiles of 16: one k-step of the weight gradient per wave)

struct PECrops {
    const float* img[PE_MAXC];
    int row0[PE_MAXC + 1];  // first output row of crop i; row0[n] = one past the last row of the launch
    int H[PE_MAXC], W[PE_MAXC];
    int n;
};

struct PETok {
    const float* base;  // pixel (image b, channel 0, row 4 ty, column 4 tx)
    long plane;         // H * W
    int W;
};

// crop of row r (uniform)
__device__ __forceinline__ int pe_first_crop(const PECrops& a, int r) {
    int cf = 0;
    for (int i = 1; i < a.n; ++i) cf += (r >= a.row0[i]);
    return cf;
}

// where row r's patch starts; cf: the crop of the wave's first row, rend: one past its last (both uniform -- a wave's rows leave crop cf
// only where a crop boundary falls inside them, so the loop below has no iteration on almost every tile)
__device__ __forceinline__ PETok pe_locate(const PECrops& a, int cf, int rend, int r) {
    const float* img = a.img[cf];
    int H = a.H[cf], W = a.W[cf], r0 = a.row0[cf];
    for (int i = cf + 1; i < a.n && a.row0[i] < rend; ++i)
        if (r >= a.row0[i]) img = a.img[i], H = a.H[i], W = a.W[i], r0 = a.row0[i];
    const unsigned rl = (unsigned)(r - r0), Gw = (unsigned)W >> 2, L = ((unsigned)H >> 2) * Gw;
    const unsigned b = rl / L, rem = rl - b * L;
    const unsigned ty = rem / Gw, tx = rem - ty * Gw;
    PETok t;
    t.plane = (long)H * W;
    t.W = W;
    t.base = img + (long)b * 3 * t.plane + (long)(4 * ty) * W + 4 * tx;
    return t;
}

// the token's 48 pixels as this lane reads them: v[0], v[1] the two patch rows of k-step 0, v[2], v[3] those of k-step 1 (g < 2); an absent
// token is all zeros and forms no address
__device__ __forceinline__ void pe_pixel_load(const PETok& t, bool valid, int g, f32x4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const float* p0 = t.base + (g >> 1) * t.plane + 2 * (g & 1) * t.W;
        v[0] = *reinterpret_cast<const f32x4*>(p0);
        v[1] = *reinterpret_cast<const f32x4*>(p0 + t.W);
        if (g < 2) {
            const float* p1 = t.base + 2 * t.plane + 2 * g * t.W;
            v[2] = *reinterpret_cast<const f32x4*>(p1);
            v[3] = *reinterpret_cast<const f32x4*>(p1 + t.W);
        }
    }
}

// ... as the operand fragments of the two k-steps, rounded to bf16 as im2col_kernel rounds them
__device__ __forceinline__ void pe_pixel_frags(const f32x4 (&v)[4], Frag<bf16> (&f)[2]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[0].v[e] = (bf16)v[0][e];
        f[0].v[4 + e] = (bf16)v[1][e];
        f[1].v[e] = (bf16)v[2][e];
        f[1].v[4 + e] = (bf16)v[3][e];
    }
}

// LDS: the weight in fragment order wf[(j * 2 + ks) * 64 + lane] = W[16 j + c][32 ks + 8 g .. + 7] (zeros from k = 48 on), then nvec
// fp32 vectors of E (bias, gamma, beta)
template <int E>
__device__ __forceinline__ void pe_fill(bf16x8* wf, float* vecs, const bf16* __restrict__ W, const float* __restrict__ v0, const float* __restrict__ v1,
                                        const float* __restrict__ v2) {
    constexpr int NJ = E / 16;
    for (int i = threadIdx.x; i < NJ * 2 * 64; i += 256) {
        const int lane = i & 63, ks = (i >> 6) & 1, j = i >> 7;
        const int c = lane & 15, g = lane >> 4, k0 = 32 * ks + 8 * g;
        bf16x8 w;
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = (bf16)0.f;
        if (k0 < PE_K) w = *reinterpret_cast<const bf16x8*>(W + (16 * j + c) * PE_K + k0);
        wf[i] = w;
    }
    for (int i = threadIdx.x; i < E; i += 256) {
        vecs[i] = v0[i];
        vecs[E + i] = v1[i];
        if (v2) vecs[2 * E + i] = v2[i];
    }
}

// Row sum over the E channels in the order ln_fwd_kernel<float, G, ITERS> adds them (norm.hip: E = 96 -> <8, 3>, 128 -> <32, 1>,
// 192 -> <16, 3>), so that mean, rstd and x keep the bits of the unfused route.  There lane gl of a G-lane group owns the 16-byte vectors
// gl + G it and adds their hsum4 in order, then a butterfly runs over gl (xor G/2 ... 1).  Here lane (c, g) owns the vectors 4 j + g:
// gl = 4 (j mod G/4) + g, it = j div (G/4) -- the upper butterfly steps are in-lane, the last two cross the lane rows (g ^ 2, g ^ 1).
template <int E>
__device__ __forceinline__ float pe_row_sum(const float (&h)[E / 16]) {
    constexpr int NJ = E / 16, GJ = E == 96 ? 2 : (E == 128 ? 8 : 4), ITERS = NJ / GJ;
    float p[GJ];
#pragma unroll
    for (int m = 0; m < GJ; ++m) {
        p[m] = 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) p[m] += h[m + GJ * it];
    }
#pragma unroll
    for (int o = GJ / 2; o > 0; o >>= 1) {
        float q[GJ];
#pragma unroll
        for (int m = 0; m < GJ; ++m) q[m] = p[m] + p[m ^ o];
#pragma unroll
        for (int m = 0; m < GJ; ++m) p[m] = q[m];
    }
    float s = p[0];
    s += __shfl_xor(s, 32, 64);
    s += __shfl_xor(s, 16, 64);
    return s;
}

template <int E>
constexpr int pe_fwd_lds() { return (E / 16) * 2 * 64 * 16 + 3 * E * 4; }

template <int E>
__global__ __launch_bounds__(256) void patch_embed_fwd_kernel(const PECrops a, const bf16* __restrict__ W, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                              float* __restrict__ x, float* __restrict__ mean, float* __restrict__ rstd) {
    constexpr int NJ = E / 16;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16x8* wf = reinterpret_cast<bf16x8*>(smem_raw);
    float* sb = reinterpret_cast<float*>(smem_raw + NJ * 2 * 64 * 16);
    float *sg = sb + E, *st = sg + E;
    pe_fill<E>(wf, sb, W, bias, gamma, beta);
    __syncthreads();
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rowlo = a.row0[0], rowhi = a.row0[a.n];
    const int ntiles = (rowhi - rowlo + PE_FWD_T - 1) / PE_FWD_T;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int rfirst = rowlo + t * PE_FWD_T + wave * 16;
        if (rfirst >= rowhi) continue;  // (a whole wave; there is no barrier in this loop)
        const int rend = rfirst + 16 < rowhi ? rfirst + 16 : rowhi;
        const int r = rfirst + c;
        const bool valid = r < rowhi;
        const PETok tok = pe_locate(a, pe_first_crop(a, rfirst), rend, valid ? r : rfirst);
        f32x4 px[4];
        pe_pixel_load(tok, valid, g, px);
        Frag<bf16> tf[2];
        pe_pixel_frags(px, tf);
        // y^T: acc[j][e] = y[token c][channel 16 j + 4 g + e]
        f32x4 v[NJ];
        float hs[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            Frag<bf16> w0, w1;
            w0.v = wf[(j * 2 + 0) * 64 + lane];
            w1.v = wf[(j * 2 + 1) * 64 + lane];
            mma(w0, tf[0], acc);
            mma(w1, tf[1], acc);
            v[j] = acc + *reinterpret_cast<const f32x4*>(sb + 16 * j + 4 * g);
            hs[j] = (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
        const float mu = pe_row_sum<E>(hs) / E;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f32x4 d = v[j] - mu;
            const f32x4 dd = d * d;
            hs[j] = (dd[0] + dd[1]) + (dd[2] + dd[3]);
        }
        const float rs = rsqrtf(pe_row_sum<E>(hs) / E + eps);
        if (valid) {
            float* xr = x + (long)r * E + 4 * g;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 gm = *reinterpret_cast<const f32x4*>(sg + 16 * j + 4 * g);
                const f32x4 bt = *reinterpret_cast<const f32x4*>(st + 16 * j + 4 * g);
                *reinterpret_cast<f32x4*>(xr + 16 * j) = (v[j] - mu) * rs * gm + bt;
            }
            if (mean && g == 0) {
                mean[r] = mu;
                rstd[r] = rs;
            }
        }
    }
}

template <int E>
constexpr int pe_rec() { return E * (PE_K + 3); }  // [dW E x 48 | dbp E | dgamma E | dbeta E]
template <int E>
constexpr int pe_bwd_lds() { return (E / 16) * 2 * 64 * 16 + 2 * E * 4 + 4 * 32 * PE_K * 2 + pe_rec<E>() * 4; }

// Order between a wave's own LDS writes and its later cross-lane reads of them (the column image is per wave, and a wave's LDS
// instructions execute in order): a compiler barrier plus a wait for the LDS counter.  NOT __syncthreads() and no fence: either makes
// hipcc emit s_waitcnt vmcnt(0), which would drain the loads of the subtile ahead at every tile (as chunk_barrier, common.h); and
// without a workgroup barrier the four waves of a workgroup walk their tiles independently.
__device__ __forceinline__ void pe_wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// what one 16-token subtile of the backward reads from memory, loaded one subtile ahead of its use: the pixels (as pe_pixel_load), and for
// this lane's result rows (tokens rfirst + 4 g + e, channel 16 j + c) gx and the saved statistics.  Absent rows read as zeros (rstd = 0
// makes their xhat, and with gx = 0 their dya, zero) and form no address.
template <int NJ>
struct PESub {
    f32x4 px[4];
    f32x4 d[NJ];
    float mu[4], rs[4];
};

template <int E>
__device__ __forceinline__ void pe_bwd_load(const PECrops& a, int rfirst, int rowhi, int c, int g, const float* __restrict__ gx,
                                            const float* __restrict__ mean, const float* __restrict__ rstd, PESub<E / 16>& s) {
    constexpr int NJ = E / 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) s.px[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) s.d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) s.mu[e] = s.rs[e] = 0.f;
    if (rfirst >= rowhi) return;  // uniform: no such subtile
    const int rend = rfirst + 16 < rowhi ? rfirst + 16 : rowhi;
    const int r = rfirst + c;
    const bool valid = r < rowhi;
    const PETok tok = pe_locate(a, pe_first_crop(a, rfirst), rend, valid ? r : rfirst);
    pe_pixel_load(tok, valid, g, s.px);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int tr = rfirst + 4 * g + e;
        if (tr < rowhi) {
            s.mu[e] = mean[tr];
            s.rs[e] = rstd[tr];
            const float* gr = gx + (long)tr * E + c;
#pragma unroll
            for (int j = 0; j < NJ; ++j) s.d[j][e] = gr[16 * j];
        }
    }
}

// One wave per SIMD (the dW accumulators alone are 0.75 E registers): the next subtile's loads are requested before the current one is
// worked on.  Measured at the B = 128 Swin-T rows (profiles/patch_embed_kernel_bench.txt): 277 us one subtile ahead, 282 us a whole tile
// ahead, 294 us with workgroup barriers -- 2.9 TB/s, the kernel is bound by its VALU issue at this occupancy, not by loads in flight.
// E = 192 has 144 accumulators and loads in place.
template <int E>
__global__ __launch_bounds__(256) void patch_embed_bwd_kernel(const PECrops a, const bf16* __restrict__ W, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma, const float* __restrict__ gx,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              float* __restrict__ part) {
    constexpr int NJ = E / 16, REC = pe_rec<E>();
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16x8* wf = reinterpret_cast<bf16x8*>(smem_raw);
    float* sb = reinterpret_cast<float*>(smem_raw + NJ * 2 * 64 * 16);
    float* sg = sb + E;
    bf16* cs_all = reinterpret_cast<bf16*>(sg + E);  // [4 waves][32 tokens][48]: the bf16 columns of the wave's two subtiles
    float* red = reinterpret_cast<float*>(cs_all + 4 * 32 * PE_K);
    pe_fill<E>(wf, sb, W, bias, gamma, nullptr);
    __syncthreads();
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bf16* cs = cs_all + wave * 32 * PE_K;
    const int rowlo = a.row0[0], rowhi = a.row0[a.n];
    const int ntiles = (rowhi - rowlo + PE_BWD_T - 1) / PE_BWD_T;

    f32x4 dw[NJ][3];                     // dw[je][jk][e] = dW[16 je + 4 g + e][16 jk + c]
    float dgam[NJ], dbet[NJ], dbp[NJ];  // channel 16 j + c, this lane's tokens
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dw[j][k] = f32x4{0.f, 0.f, 0.f, 0.f};
        dgam[j] = dbet[j] = dbp[j] = 0.f;
    }

    constexpr bool AHEAD = E <= 128;
    PESub<NJ> nxt;
    if constexpr (AHEAD) pe_bwd_load<E>(a, rowlo + blockIdx.x * PE_BWD_T + wave * 32, rowhi, c, g, gx, mean, rstd, nxt);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int rwave = rowlo + t * PE_BWD_T + wave * 32;
        bf16x4 ob[2][NJ];  // rounded dya of the two subtiles: tokens 16 h + 4 g + e, channel 16 j + c
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            PESub<NJ> cur;
            __builtin_amdgcn_sched_barrier(0);  // (one subtile ahead, not two: the loads below stay below the subtile before)
            if constexpr (AHEAD) {  // the subtile after this one is on its way while this one is worked on
                cur = nxt;
                const int rnext = h == 0 ? rwave + 16 : (t + (int)gridDim.x < ntiles ? rwave + (int)gridDim.x * PE_BWD_T : rowhi);
                pe_bwd_load<E>(a, rnext, rowhi, c, g, gx, mean, rstd, nxt);
            } else {
                pe_bwd_load<E>(a, rwave + 16 * h, rowhi, c, g, gx, mean, rstd, cur);
            }
            Frag<bf16> tf[2];
            pe_pixel_frags(cur.px, tf);
            *reinterpret_cast<bf16x8*>(cs + (16 * h + c) * PE_K + 8 * g) = tf[0].v;
            if (g < 2) *reinterpret_cast<bf16x8*>(cs + (16 * h + c) * PE_K + 32 + 8 * g) = tf[1].v;
            f32x4 xh[NJ];
            f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};  // acc[e] = y[token 4 g + e][channel 16 j + c] (without the bias)
                Frag<bf16> w0, w1;
                w0.v = wf[(j * 2 + 0) * 64 + lane];
                w1.v = wf[(j * 2 + 1) * 64 + lane];
                mma(tf[0], w0, acc);
                mma(tf[1], w1, acc);
                const float bj = sb[16 * j + c], gj = sg[16 * j + c];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xh[j][e] = ((acc[e] + bj) - cur.mu[e]) * cur.rs[e];
                    dgam[j] += cur.d[j][e] * xh[j][e];
                    dbet[j] += cur.d[j][e];
                }
                const f32x4 gd = cur.d[j] * gj;
                s1 += gd;
                s2 += gd * xh[j];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s1[e] = row16_sum(s1[e]) / E;
                s2[e] = row16_sum(s2[e]) / E;
            }
            const f32x4 rs4 = {cur.rs[0], cur.rs[1], cur.rs[2], cur.rs[3]};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 o = (cur.d[j] * sg[16 * j + c] - s1 - xh[j] * s2) * rs4;
                ob[h][j] = bf16x4{(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
                dbp[j] += ((float)ob[h][j][0] + (float)ob[h][j][1]) + ((float)ob[h][j][2] + (float)ob[h][j][3]);
            }
        }
        pe_wave_sync();  // the columns of both subtiles are in this wave's LDS image
#pragma unroll
        for (int jk = 0; jk < 3; ++jk) {
            const Frag<bf16> colf = frag_v_perm<bf16>(cs, PE_K, 16 * jk, 0, c, g);
#pragma unroll
            for (int je = 0; je < NJ; ++je) {
                Frag<bf16> df;
                df.v = __builtin_shufflevector(ob[0][je], ob[1][je], 0, 1, 2, 3, 4, 5, 6, 7);
                mma(df, colf, dw[je][jk]);
            }
        }
        pe_wave_sync();  // ... and read, before the next tile overwrites them
    }

    // fold the lane rows (dgamma, dbeta, dbp: partial over the tokens 4 g + e), then the four waves in order through LDS
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        dgam[j] += __shfl_xor(dgam[j], 16, 64);
        dgam[j] += __shfl_xor(dgam[j], 32, 64);
        dbet[j] += __shfl_xor(dbet[j], 16, 64);
        dbet[j] += __shfl_xor(dbet[j], 32, 64);
        dbp[j] += __shfl_xor(dbp[j], 16, 64);
        dbp[j] += __shfl_xor(dbp[j], 32, 64);
    }
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int je = 0; je < NJ; ++je)
#pragma unroll
                for (int jk = 0; jk < 3; ++jk)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = (16 * je + 4 * g + e) * PE_K + 16 * jk + c;
                        red[i] = (w ? red[i] : 0.f) + dw[je][jk][e];
                    }
            if (g == 0) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int i = E * PE_K + 16 * j + c;
                    red[i] = (w ? red[i] : 0.f) + dbp[j];
                    red[i + E] = (w ? red[i + E] : 0.f) + dgam[j];
                    red[i + 2 * E] = (w ? red[i + 2 * E] : 0.f) + dbet[j];
                }
            }
        }
        __syncthreads();
    }
    float* mine = part + (long)blockIdx.x * REC;
    for (int i = threadIdx.x; i < REC; i += 256) mine[i] = red[i];
}

// out[i] = sum_p part[p][i]: eight strided sums p = s, s + 8, ... per column, then the eight in order
__global__ __launch_bounds__(256) void patch_embed_reduce_kernel(const float* __restrict__ part, int nparts, int E, float* __restrict__ dW,
                                                                 float* __restrict__ dbp, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float sm[8][33];
    const int rec = E * (PE_K + 3);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + tx;
    float s = 0.f;
    if (i < rec)
        for (int p = ty; p < nparts; p += 8) s += part[(long)p * rec + i];
    sm[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && i < rec) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += sm[k][tx];
        const int nw = E * PE_K;
        if (i < nw) dW[i] = t;
        else if (i < nw + E) dbp[i - nw] = t;
        else if (i < nw + 2 * E) dgamma[i - nw - E] = t;
        else dbeta[i - nw - 2 * E] = t;
    }
}

int pe_cus() {
    static int cus[64] = {0};
    int dev = 0;
    int n = 256;  // (no device: the size of an MI355X)
    if (hipGetDevice(&dev) == hipSuccess) {
        int& slot = cus[dev & 63];
        if (slot == 0 && hipDeviceGetAttribute(&slot, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) slot = 0;
        if (slot > 0) n = slot;
    } else {
        (void)hipGetLastError();
    }
    return n;
}

inline bool pe_width(int E) { return E == 96 || E == 128 || E == 192; }

int pe_bwd_grid(long M) {
    const long ntiles = (M + PE_BWD_T - 1) / PE_BWD_T, cap = pe_cus();  // one resident workgroup per CU
    return (int)(ntiles < cap ? ntiles : cap);
}

template <int E>
int pe_launch_fwd(const PECrops& a, int grid, const esvit_patch_embed* d, hipStream_t stream) {
    static unsigned long long raised = 0;
    esvit_raise_lds(patch_embed_fwd_kernel<E>, pe_fwd_lds<E>(), raised);
    hipLaunchKernelGGL(patch_embed_fwd_kernel<E>, dim3(grid), dim3(256), pe_fwd_lds<E>(), stream, a, reinterpret_cast<const bf16*>(d->W), d->bias,
                       d->gamma, d->beta, d->eps, d->x, d->mean, d->rstd);
    ESVIT_CHECK_LAUNCH("patch_embed_fwd");
    return ESVIT_OK;
}

template <int E>
int pe_launch_bwd(const PECrops& a, int grid, const esvit_patch_embed* d, hipStream_t stream) {
    static unsigned long long raised = 0;
    esvit_raise_lds(patch_embed_bwd_kernel<E>, pe_bwd_lds<E>(), raised);
    hipLaunchKernelGGL(patch_embed_bwd_kernel<E>, dim3(grid), dim3(256), pe_bwd_lds<E>(), stream, a, reinterpret_cast<const bf16*>(d->W), d->bias,
                       d->gamma, d->gx, d->mean, d->rstd, d->partials + (long)d->first_partial * pe_rec<E>());
    ESVIT_CHECK_LAUNCH("patch_embed_bwd");
    return ESVIT_OK;
}

}  // namespace

// esvit_query(ESVIT_Q_PATCH_EMBED_WS, dtype, E, M): bytes of the partial records one backward launch over M token rows writes
int64_t esvit_i_patch_embed_ws(int dtype, int E, int64_t M) {
    if (dtype != ESVIT_BF16 || !pe_width(E) || M <= 0 || M > ESVIT_PATCH_EMBED_MAX_ROWS) return 0;
    return (int64_t)pe_bwd_grid((long)M) * E * (PE_K + 3) * 4;
}

// the fused mode of esvit_patch_im2col (nB = -(crop records)): every check answers before any device call
int esvit_i_patch_embed(int dtype, const void* desc, int ncrops, int S, int P, int Kpad, hipStream_t stream) {
    const esvit_patch_embed* d = reinterpret_cast<const esvit_patch_embed*>(desc);
    ESVIT_CHECK_ARG(d != nullptr, "esvit_patch_im2col: fused mode without a descriptor");
    ESVIT_CHECK_ARG(dtype == ESVIT_BF16, "esvit_patch_im2col: the fused patch embedding exists in bf16 mode only (dtype=%d)", dtype);
    ESVIT_CHECK_ARG(S == 0 && P == 4 && Kpad == PE_K, "esvit_patch_im2col: the fused patch embedding takes S=0, P=4, Kpad=48 (S=%d P=%d Kpad=%d)", S, P,
                    Kpad);
    ESVIT_CHECK_ARG(pe_width(d->E), "esvit_patch_im2col: fused patch embedding: E=%d is not one of 96, 128, 192", d->E);
    const int E = d->E;
    if (d->mode == ESVIT_PATCH_EMBED_REDUCE) {
        ESVIT_CHECK_ARG(d->partials && d->dW && d->dbp && d->dgamma && d->dbeta, "esvit_patch_im2col: fused patch embedding (reduce): null pointer");
        ESVIT_CHECK_ARG(d->first_partial > 0, "esvit_patch_im2col: fused patch embedding (reduce): %d partial records", d->first_partial);
        hipLaunchKernelGGL(patch_embed_reduce_kernel, dim3(ceil_div(E * (PE_K + 3), 32)), dim3(256), 0, stream, d->partials, d->first_partial, E, d->dW,
                           d->dbp, d->dgamma, d->dbeta);
        ESVIT_CHECK_LAUNCH("patch_embed_reduce");
        return ESVIT_OK;
    }
    ESVIT_CHECK_ARG(d->mode == ESVIT_PATCH_EMBED_FWD || d->mode == ESVIT_PATCH_EMBED_BWD, "esvit_patch_im2col: fused patch embedding: bad mode %d", d->mode);
    ESVIT_CHECK_ARG(ncrops >= 1 && ncrops <= PE_MAXC, "esvit_patch_im2col: fused patch embedding takes 1..%d crop records per launch, not %d", PE_MAXC,
                    ncrops);
    ESVIT_CHECK_ARG(d->W && d->bias && d->gamma && ((uintptr_t)d->W % 16) == 0, "esvit_patch_im2col: fused patch embedding: null / misaligned weight, bias or gamma");
    PECrops a;
    long row = d->crops[0].row0;
    ESVIT_CHECK_ARG(row >= 0, "esvit_patch_im2col: fused patch embedding: crop 0 starts at row %ld", row);
    for (int i = 0; i < PE_MAXC; ++i) {
        const esvit_patch_crop& cr = d->crops[i < ncrops ? i : 0];  // (unused slots repeat crop 0: never selected, never a wild pointer)
        if (i < ncrops) {
            ESVIT_CHECK_ARG(cr.img && ((uintptr_t)cr.img % 16) == 0, "esvit_patch_im2col: fused patch embedding: crop %d: null / misaligned image", i);
            ESVIT_CHECK_ARG(cr.nB > 0 && cr.H > 0 && cr.W > 0 && cr.H % 4 == 0 && cr.W % 4 == 0 && cr.H < 65536 && cr.W < 65536,
                            "esvit_patch_im2col: fused patch embedding: crop %d: bad image (nB=%d H=%d W=%d)", i, cr.nB, cr.H, cr.W);
            ESVIT_CHECK_ARG(cr.row0 == row, "esvit_patch_im2col: fused patch embedding: crop %d starts at row %ld, the crops before it end at %ld", i,
                            (long)cr.row0, row);
            const long n = (long)cr.nB * (cr.H / 4) * (cr.W / 4);
            ESVIT_CHECK_ARG(n <= ESVIT_PATCH_EMBED_MAX_ROWS && row + n <= ESVIT_PATCH_EMBED_MAX_ROWS,
                            "esvit_patch_im2col: fused patch embedding: more than %d token rows", ESVIT_PATCH_EMBED_MAX_ROWS);
            a.row0[i] = (int)row;
            row += n;
        } else {
            a.row0[i] = 0x7fffffff;
        }
        a.img[i] = cr.img, a.H[i] = cr.H, a.W[i] = cr.W;
    }
    a.row0[ncrops] = (int)row;
    a.n = ncrops;
    const long M = row - a.row0[0];
    if (d->mode == ESVIT_PATCH_EMBED_FWD) {
        ESVIT_CHECK_ARG(d->beta && d->x && ((uintptr_t)d->x % 16) == 0, "esvit_patch_im2col: fused patch embedding (forward): null / misaligned beta or x");
        ESVIT_CHECK_ARG((d->mean == nullptr) == (d->rstd == nullptr), "esvit_patch_im2col: fused patch embedding (forward): mean and rstd come together");
        const long ntiles = (M + PE_FWD_T - 1) / PE_FWD_T, cap = 8L * pe_cus();
        const int grid = (int)(ntiles < cap ? ntiles : cap);
        if (E == 96) return pe_launch_fwd<96>(a, grid, d, stream);
        if (E == 128) return pe_launch_fwd<128>(a, grid, d, stream);
        return pe_launch_fwd<192>(a, grid, d, stream);
    }
    ESVIT_CHECK_ARG(d->gx && d->mean && d->rstd && d->partials && d->first_partial >= 0,
                    "esvit_patch_im2col: fused patch embedding (backward): null gx, mean, rstd or partials");
    const int grid = pe_bwd_grid(M);
    if (E == 96) return pe_launch_bwd<96>(a, grid, d, stream);
    if (E == 128) return pe_launch_bwd<128>(a, grid, d, stream);
    return pe_launch_bwd<192>(a, grid, d, stream);
}
