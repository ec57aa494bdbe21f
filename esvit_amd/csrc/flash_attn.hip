// Flash attention for whole ViT crops of any length (vision_transformer.py:76-83), bf16, gfx950: the global mode of
// esvit_window_attn_fwd / esvit_window_attn_bwd (ws = ESVIT_ATTN_GLOBAL, include/esvit_hip.h).  It takes the crops that do not fit the
// one-window kernels of window_attn.hip (<= 64 tokens) and window_attn_big.hip (<= 224): 785 tokens of a 224^2 crop at patch 8,
// 401 / 577 / 785 tokens of 320^2 / 384^2 / 448^2 at patch 16.  Token-ordered I/O (qkv [B N, 3C], columns [3][nH][hd]; out [B N, C];
// lse fp32 [B, nH, N]): no head split / merge pass, the scores stay on the chip, nothing grows with N^2, nothing is padded in memory.
//
//   forward   flash_fwd: one workgroup per (image, head, 64-query block), four waves, one 16-query tile each.  The Q block is staged
//             once; K and V stream through a two-deep LDS ring in 64-key blocks (the next block's global loads are issued before the
//             current block's MFMAs and stored after them: one barrier per block).  A wave forms S^T = K Q^T for its tile (4 MFMA tiles
//             in registers: P lands in B-operand order), keeps a running max and sum per query in fp32, rescales O when the max moves,
//             and adds P V with the transpose read of V (mfma.h: frag_v_perm), as chunk_attn.hip does for its 448 slots at once.  out = O / l,
//             lse = m + log l.  Slots >= N of the last query / key block are zero rows in LDS; their scores are set to -1e30 before
//             the max (the first key block always holds key 0, so the running max is finite from the first step); their output and lse
//             rows are never stored.
//   backward  delta = rowsum(dO o O) once (flash_delta, fp32 [B, nH, N] in the caller's scratch; summed as the MFMA sums dP); then
//             flash_bwd_dq   per (image, head, query block), over the key blocks:  P = exp(scale s - lse), dS = P o (dP - delta),
//                            dQ += scale dS K
//             flash_bwd_dkv  per (image, head, key block), over the query blocks (Q, dO, lse, delta through the ring):
//                            dV += P^T dO, dK += scale dS^T Q
//             Every row of dqkv is written by exactly one workgroup: no atomics, two launches give identical bits.
//   stats     ws = ESVIT_ATTN_GLOBAL | ESVIT_ATTN_STATS: the entropy of every softmax row (stats_entropy, the forward without V) and
//             the fp32 probability rows of a few listed queries (stats_rows), for the attention analysis of esvit_amd/analysis.py.
//
// Q, K, V and dO enter the MFMAs as the bf16 values they are and the scale multiplies the fp32 scores (chunk_attn.hip's header records
// what scaling Q in LDS cost).  P and dS are rounded to bf16 for their MFMAs; everything else is fp32.  Head dims 32 and 64.
//
// LDS (bf16 rows padded by 8 elements): forward Q + 2 x (K, V) = 5 [64][hd + 8] images, 25.6 KB (hd 32) / 46.1 KB (hd 64); backward
// six images (+ 1 KB of lse / delta for dK dV): 30.7-31.7 / 55.3-56.3 KB -- two workgroups per CU and more at either head dim.
// The statistics kernels hold Q + 2 x K (15.4 / 27.6 KB) and 2 x K + 512 B of per-wave maxima and sums (10.8 / 18.9 KB), statically.
// VGPRs (tools/kernel_regs.sh flash_attn), no scratch, no spills:  hd 32: fwd 76, dq 78, dkv 108, entropy 60, rows 76;
// hd 64: fwd 120, dq 110, dkv 156, entropy 72, rows 88.
#include "common.h"
#include "mfma.h"
#include "../../include/esvit_hip.h"

namespace {

constexpr int BLKT = 64;            // tokens per query block and per key block (a multiple of the 32-deep MFMA k-step)
constexpr int NT16 = BLKT / 16;     // 16-token tiles per block
constexpr int WAVES = BLKT / 16;    // one 16-token tile of the workgroup's own block per wave
constexpr int NTHR = WAVES * 64;

template <int HD>
struct FCfg {
    static constexpr int LDQ = HD + 8;
    static constexpr int VPR = HD / 8;  // 16-byte pieces of a row
    static constexpr int KS = HD / 32, DT = HD / 16;
    static constexpr int IMG = BLKT * LDQ;  // elements of one [64][LDQ] image
};

// stage rows row0 .. row0 + 63 of one image's token-ordered bf16 matrix (g: row 0 of the image at the head's columns) into a
// [64][LDQ] image, zero rows for tokens >= N.  Two phases: every global load of the thread is issued by load(), store() puts
// them into LDS -- the main loops run the MFMAs of the current block between the two (chunk_attn.hip: RowStage, by token table).
template <int HD>
struct RowStage {
    using Cfg = FCfg<HD>;
    static constexpr int ITERS = BLKT * Cfg::VPR / NTHR;
    static_assert(BLKT * Cfg::VPR % NTHR == 0, "whole rounds");
    bf16x8 x[ITERS];
    __device__ __forceinline__ void load(const bf16* __restrict__ g, long row_stride, int row0, int N, int tid) {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int v = tid + it * NTHR;
            const int t = row0 + v / Cfg::VPR, dv = v % Cfg::VPR;
            bf16x8 y = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
            if (t < N) y = *reinterpret_cast<const bf16x8*>(g + (long)t * row_stride + dv * 8);
            x[it] = y;
        }
    }
    __device__ __forceinline__ void store(bf16* lds, int tid) const {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int v = tid + it * NTHR;
            *reinterpret_cast<bf16x8*>(lds + (v / Cfg::VPR) * Cfg::LDQ + (v % Cfg::VPR) * 8) = x[it];
        }
    }
};

struct Unit {
    int z, b, h, blk;
};
__device__ __forceinline__ Unit unit_of(int u, int nblk, int nH) {
    Unit x;
    x.z = u / nblk;
    x.blk = u % nblk;
    x.b = x.z / nH;
    x.h = x.z % nH;
    return x;
}

// -------------------------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(NTHR) void flash_fwd_kernel(const bf16* __restrict__ qkv, int N, int nH, int nblk, float scale,
                                                         bf16* __restrict__ out, float* __restrict__ lse_out) {
    using Cfg = FCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, DT = Cfg::DT, IMG = Cfg::IMG;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16* Qs = reinterpret_cast<bf16*>(smem_raw);
    bf16* Kr = Qs + IMG;      // [2][64][LDQ]
    bf16* Vr = Kr + 2 * IMG;  // [2][64][LDQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;

    const Unit u = unit_of(blockIdx.x, nblk, nH);
    const int C = nH * HD;
    const bf16* src = qkv + (long)u.b * N * 3 * C + u.h * HD;
    const int q0 = u.blk * BLKT;
    {
        RowStage<HD> sq, sk, sv;
        sq.load(src, 3L * C, q0, N, tid);
        sk.load(src + C, 3L * C, 0, N, tid);
        sv.load(src + 2 * C, 3L * C, 0, N, tid);
        sq.store(Qs, tid);
        sk.store(Kr, tid);
        sv.store(Vr, tid);
    }
    __syncthreads();
    const bool live = q0 + 16 * wave < N;  // does this wave's query tile hold a token at all (wave-uniform)

    Frag<bf16> qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = frag_kc<bf16>(Qs, LDQ, 16 * wave, 32 * ks, c, g);
    float m = -3.0e38f, l = 0.f;  // running max and sum of query slot 16 wave + c (the same in the four lanes g of a column)
    f32x4 o[DT];                  // O^T [channel][query], unnormalised
#pragma unroll
    for (int j = 0; j < DT; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int kb = 0; kb < nblk; ++kb) {
        const bool more = kb + 1 < nblk;
        RowStage<HD> sk, sv;
        if (more) {
            sk.load(src + C, 3L * C, (kb + 1) * BLKT, N, tid);
            sv.load(src + 2 * C, 3L * C, (kb + 1) * BLKT, N, tid);
        }
        const bf16* Ks = Kr + (kb & 1) * IMG;
        const bf16* Vs = Vr + (kb & 1) * IMG;
        if (live) {
            // S^T tiles: p[i][r] = score of key kb * 64 + 16 i + 4g + r and query slot 16 wave + c
            f32x4 p[NT16];
            float mb = -3.0e38f;
#pragma unroll
            for (int i = 0; i < NT16; ++i) {
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) mma(frag_kc<bf16>(Ks, LDQ, 16 * i, 32 * ks, c, g), qf[ks], s);
                const int key0 = kb * BLKT + 16 * i + 4 * g;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r] = key0 + r < N ? s[r] * scale : -1.0e30f;
                    mb = fmaxf(mb, s[r]);
                }
                p[i] = s;
            }
            mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
            mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
            const float mn = fmaxf(m, mb);
            const float alpha = __expf(m - mn);  // (first block: exp(-3e38 - mn) = 0 on O = 0, l = 0)
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < NT16; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __expf(p[i][r] - mn);
                    p[i][r] = e;
                    sum += e;
                }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            l = l * alpha + sum;
            m = mn;
#pragma unroll
            for (int j = 0; j < DT; ++j) o[j] = o[j] * alpha;
#pragma unroll
            for (int ks = 0; ks < BLKT / 32; ++ks) {
                const Frag<bf16> pf = frag_p_regs<bf16>(p[2 * ks], p[2 * ks + 1]);
#pragma unroll
                for (int j = 0; j < DT; ++j) mma(frag_v_perm<bf16>(Vs, LDQ, 16 * j, ks, c, g), pf, o[j]);  // O^T: operands exchanged
            }
        }
        if (more) {  // the other half of the ring: every wave left it at the barrier that ended block kb - 1
            sk.store(Kr + ((kb + 1) & 1) * IMG, tid);
            sv.store(Vr + ((kb + 1) & 1) * IMG, tid);
        }
        __syncthreads();
    }
    if (!live) return;
    const int qt = q0 + 16 * wave + c;
    const int tok = qt < N ? qt : -1;
    if (g == 0 && tok >= 0) lse_out[(long)u.z * N + tok] = m + __logf(l);
    store_tile_rows<HD>(o, 1.f / l, out + (long)u.b * N * C, N, C, u.h * HD, tok, g);
}

// delta[z][t] = sum_d dO[t][h, d] * O[t][h, d], one wave per 16 tokens of one (image, head).  chunk_attn.hip's chunk_delta sums on the
// VALU; here the sum is the diagonal of the MFMA tile O dO^T, formed with the k-order and the accumulation chain with which the
// backward kernels form dP = dO V^T: where a row of O IS a row of V (a one-token image, a softmax that is one-hot after rounding),
// dP - delta cancels to an exact zero as it does in exact arithmetic, instead of leaving the difference of two summation orders.
template <int HD>
__global__ __launch_bounds__(NTHR) void flash_delta_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ fout, int N, int nH, int ntile,
                                                           long nunits, float* __restrict__ delta) {
    constexpr int KS = FCfg<HD>::KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const long unit = (long)blockIdx.x * WAVES + wave;  // (z, tile), wave-uniform
    if (unit >= nunits) return;
    const int z = (int)(unit / ntile), tile = (int)(unit % ntile);
    const int b = z / nH, h = z % nH;
    const int t = 16 * tile + c;
    const long off = ((long)b * N + t) * (nH * HD) + h * HD + 8 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kd = 0; kd < KS; ++kd) {
        Frag<bf16> of, df;
        of.v = df.v = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
        if (t < N) {
            of.v = *reinterpret_cast<const bf16x8*>(fout + off + 32 * kd);
            df.v = *reinterpret_cast<const bf16x8*>(dout + off + 32 * kd);
        }
        mma(of, df, acc);  // acc[r] = O[token 4g + r] . dO[token c]
    }
    if (t < N && g == (c >> 2)) delta[(long)z * N + t] = acc[c & 3];
}

// -------------------------------------------------------------------------------------------------------------
// backward, dQ: own block = queries, ring = key blocks
// -------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(NTHR) void flash_bwd_dq_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                            const float* __restrict__ lse_in, const float* __restrict__ delta_in, int N,
                                                            int nH, int nblk, float scale, bf16* __restrict__ dqkv) {
    using Cfg = FCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, DT = Cfg::DT, IMG = Cfg::IMG;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16* Qs = reinterpret_cast<bf16*>(smem_raw);
    bf16* Os = Qs + IMG;      // dO rows of the block's queries
    bf16* Kr = Os + IMG;      // [2][64][LDQ]
    bf16* Vr = Kr + 2 * IMG;  // [2][64][LDQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;

    const Unit u = unit_of(blockIdx.x, nblk, nH);
    const int C = nH * HD;
    const bf16* src = qkv + (long)u.b * N * 3 * C + u.h * HD;
    const bf16* dsrc = dout + (long)u.b * N * C + u.h * HD;
    const int q0 = u.blk * BLKT;
    {
        RowStage<HD> sq, so, sk, sv;
        sq.load(src, 3L * C, q0, N, tid);
        so.load(dsrc, (long)C, q0, N, tid);
        sk.load(src + C, 3L * C, 0, N, tid);
        sv.load(src + 2 * C, 3L * C, 0, N, tid);
        sq.store(Qs, tid);
        so.store(Os, tid);
        sk.store(Kr, tid);
        sv.store(Vr, tid);
    }
    __syncthreads();
    const bool live = q0 + 16 * wave < N;

    const int qt = q0 + 16 * wave + c;
    const int tok = qt < N ? qt : -1;
    // a query slot >= N rebuilds P = exp(s - 3e38) = 0 (its row is not stored)
    const float lq = tok >= 0 ? lse_in[(long)u.z * N + tok] : 3.0e38f;
    const float dl = tok >= 0 ? delta_in[(long)u.z * N + tok] : 0.f;
    Frag<bf16> qf[KS], of[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = frag_kc<bf16>(Qs, LDQ, 16 * wave, 32 * ks, c, g);
        of[ks] = frag_kc<bf16>(Os, LDQ, 16 * wave, 32 * ks, c, g);
    }
    f32x4 acc[DT];  // dQ^T [channel][query]
#pragma unroll
    for (int j = 0; j < DT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int kb = 0; kb < nblk; ++kb) {
        const bool more = kb + 1 < nblk;
        RowStage<HD> sk, sv;
        if (more) {
            sk.load(src + C, 3L * C, (kb + 1) * BLKT, N, tid);
            sv.load(src + 2 * C, 3L * C, (kb + 1) * BLKT, N, tid);
        }
        const bf16* Ks = Kr + (kb & 1) * IMG;
        const bf16* Vs = Vr + (kb & 1) * IMG;
        if (live) {
#pragma unroll
            for (int ks = 0; ks < BLKT / 32; ++ks) {
                f32x4 ds2[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int i = 2 * ks + a;
                    f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kd = 0; kd < KS; ++kd) {
                        mma(frag_kc<bf16>(Ks, LDQ, 16 * i, 32 * kd, c, g), qf[kd], s);    // S^T = K Q^T
                        mma(frag_kc<bf16>(Vs, LDQ, 16 * i, 32 * kd, c, g), of[kd], dp);   // dP^T = V dO^T
                    }
                    const int key0 = kb * BLKT + 16 * i + 4 * g;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pe = key0 + r < N ? __expf(s[r] * scale - lq) : 0.f;
                        ds2[a][r] = pe * (dp[r] - dl);
                    }
                }
                const Frag<bf16> sf = frag_p_regs<bf16>(ds2[0], ds2[1]);
#pragma unroll
                for (int j = 0; j < DT; ++j) mma(frag_v_perm<bf16>(Ks, LDQ, 16 * j, ks, c, g), sf, acc[j]);  // dQ^T += K^T dS^T
            }
        }
        if (more) {
            sk.store(Kr + ((kb + 1) & 1) * IMG, tid);
            sv.store(Vr + ((kb + 1) & 1) * IMG, tid);
        }
        __syncthreads();
    }
    if (!live) return;
    store_tile_rows<HD>(acc, scale, dqkv + (long)u.b * N * 3 * C, N, 3 * C, u.h * HD, tok, g);
}

// -------------------------------------------------------------------------------------------------------------
// backward, dK and dV: own block = keys, ring = query blocks (Q, dO, lse, delta)
// -------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(NTHR) void flash_bwd_dkv_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                             const float* __restrict__ lse_in, const float* __restrict__ delta_in, int N,
                                                             int nH, int nblk, float scale, bf16* __restrict__ dqkv) {
    using Cfg = FCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, DT = Cfg::DT, IMG = Cfg::IMG;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* lser = reinterpret_cast<float*>(smem_raw);  // [2][64] log-sum-exp of the ring's queries
    float* delr = lser + 2 * BLKT;                     // [2][64] their delta
    bf16* Kt = reinterpret_cast<bf16*>(delr + 2 * BLKT);
    bf16* Vt = Kt + IMG;
    bf16* Qr = Vt + IMG;      // [2][64][LDQ]
    bf16* Or = Qr + 2 * IMG;  // [2][64][LDQ] dO rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;

    const Unit u = unit_of(blockIdx.x, nblk, nH);
    const int C = nH * HD;
    const bf16* src = qkv + (long)u.b * N * 3 * C + u.h * HD;
    const bf16* dsrc = dout + (long)u.b * N * C + u.h * HD;
    const float* lsez = lse_in + (long)u.z * N;
    const float* delz = delta_in + (long)u.z * N;
    const int k0 = u.blk * BLKT;
    {
        RowStage<HD> sk, sv, sq, so;
        sk.load(src + C, 3L * C, k0, N, tid);
        sv.load(src + 2 * C, 3L * C, k0, N, tid);
        sq.load(src, 3L * C, 0, N, tid);
        so.load(dsrc, (long)C, 0, N, tid);
        if (tid < BLKT) {  // a query slot >= N rebuilds P = exp(s - 3e38) = 0
            lser[tid] = tid < N ? lsez[tid] : 3.0e38f;
            delr[tid] = tid < N ? delz[tid] : 0.f;
        }
        sk.store(Kt, tid);
        sv.store(Vt, tid);
        sq.store(Qr, tid);
        so.store(Or, tid);
    }
    __syncthreads();
    const bool live = k0 + 16 * wave < N;  // (a key slot >= N of a live tile has k = v = 0: its columns are finite and not stored)

    Frag<bf16> kf[KS], vf[KS];
#pragma unroll
    for (int kd = 0; kd < KS; ++kd) {
        kf[kd] = frag_kc<bf16>(Kt, LDQ, 16 * wave, 32 * kd, c, g);
        vf[kd] = frag_kc<bf16>(Vt, LDQ, 16 * wave, 32 * kd, c, g);
    }
    f32x4 av[DT], ak[DT];  // dV^T, dK^T [channel][key]
#pragma unroll
    for (int j = 0; j < DT; ++j) av[j] = ak[j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int qb = 0; qb < nblk; ++qb) {
        const bool more = qb + 1 < nblk;
        RowStage<HD> sq, so;
        float nl = 3.0e38f, nd = 0.f;
        if (more) {
            sq.load(src, 3L * C, (qb + 1) * BLKT, N, tid);
            so.load(dsrc, (long)C, (qb + 1) * BLKT, N, tid);
            const int t = (qb + 1) * BLKT + tid;
            if (tid < BLKT && t < N) {
                nl = lsez[t];
                nd = delz[t];
            }
        }
        const bf16* Qs = Qr + (qb & 1) * IMG;
        const bf16* Os = Or + (qb & 1) * IMG;
        const float* ls = lser + (qb & 1) * BLKT;
        const float* de = delr + (qb & 1) * BLKT;
        if (live) {
#pragma unroll
            for (int ks = 0; ks < BLKT / 32; ++ks) {
                // oriented S: p2[a][r] = P[query 16 (2 ks + a) + 4g + r][key slot 16 wave + c]
                f32x4 p2[2], ds2[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int j = 2 * ks + a;
                    f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kd = 0; kd < KS; ++kd) {
                        mma(frag_kc<bf16>(Qs, LDQ, 16 * j, 32 * kd, c, g), kf[kd], s);    // S = Q K^T
                        mma(frag_kc<bf16>(Os, LDQ, 16 * j, 32 * kd, c, g), vf[kd], dp);   // dP = dO V^T
                    }
                    const f32x4 l4 = *reinterpret_cast<const f32x4*>(ls + 16 * j + 4 * g);
                    const f32x4 d4 = *reinterpret_cast<const f32x4*>(de + 16 * j + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pe = __expf(s[r] * scale - l4[r]);
                        p2[a][r] = pe;
                        ds2[a][r] = pe * (dp[r] - d4[r]);
                    }
                }
                const Frag<bf16> pf = frag_p_regs<bf16>(p2[0], p2[1]), sf = frag_p_regs<bf16>(ds2[0], ds2[1]);
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    mma(frag_v_perm<bf16>(Os, LDQ, 16 * j, ks, c, g), pf, av[j]);  // dV^T += dO^T P
                    mma(frag_v_perm<bf16>(Qs, LDQ, 16 * j, ks, c, g), sf, ak[j]);  // dK^T += Q^T dS
                }
            }
        }
        if (more) {
            sq.store(Qr + ((qb + 1) & 1) * IMG, tid);
            so.store(Or + ((qb + 1) & 1) * IMG, tid);
            if (tid < BLKT) {
                lser[((qb + 1) & 1) * BLKT + tid] = nl;
                delr[((qb + 1) & 1) * BLKT + tid] = nd;
            }
        }
        __syncthreads();
    }
    if (!live) return;
    const int kt = k0 + 16 * wave + c;
    const int tok = kt < N ? kt : -1;
    bf16* rows = dqkv + (long)u.b * N * 3 * C;
    store_tile_rows<HD>(ak, scale, rows, N, 3 * C, C + u.h * HD, tok, g);
    store_tile_rows<HD>(av, 1.f, rows, N, 3 * C, 2 * C + u.h * HD, tok, g);
}

// -------------------------------------------------------------------------------------------------------------
// attention statistics (ws = ESVIT_ATTN_GLOBAL | ESVIT_ATTN_STATS): what an attention analysis reads, without P and without V
// -------------------------------------------------------------------------------------------------------------
// entropy of every softmax row, in nats: the forward's work map and K ring, Q and K only.  Beside the running max m and sum l a query
// carries u = sum_k e^(s_k - m) (s_k - m); when the max moves to m' (alpha = e^(m - m')) every old term e^(s - m)(s - m) becomes
// alpha e^(s - m) ((s - m) + (m - m')), i.e. u <- alpha (u + (m - m') l).  H = ln l - u / l: l >= 1 (the maximum's own term is e^0) and
// u <= 0, both terms are >= 0 and nothing cancels.  A key slot >= N has e = 0 and adds an exact (signed) zero to l and u.
// ent: row 0 of the image-head's [rows][N] slab (row_stride = rows * N floats per (image, head)).
template <int HD>
__global__ __launch_bounds__(NTHR) void stats_entropy_kernel(const bf16* __restrict__ qkv, int N, int nH, int nblk, float scale,
                                                             long slab, float* __restrict__ ent, float* __restrict__ lse_out) {
    using Cfg = FCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, IMG = Cfg::IMG;
    __shared__ __attribute__((aligned(16))) bf16 Qs[IMG];
    __shared__ __attribute__((aligned(16))) bf16 Kr[2 * IMG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;

    const Unit u = unit_of(blockIdx.x, nblk, nH);
    const int C = nH * HD;
    const bf16* src = qkv + (long)u.b * N * 3 * C + u.h * HD;
    const int q0 = u.blk * BLKT;
    {
        RowStage<HD> sq, sk;
        sq.load(src, 3L * C, q0, N, tid);
        sk.load(src + C, 3L * C, 0, N, tid);
        sq.store(Qs, tid);
        sk.store(Kr, tid);
    }
    __syncthreads();
    const bool live = q0 + 16 * wave < N;

    Frag<bf16> qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = frag_kc<bf16>(Qs, LDQ, 16 * wave, 32 * ks, c, g);
    float m = -3.0e38f, l = 0.f, uu = 0.f;  // of query slot 16 wave + c (the same in the four lanes g of a column)

#pragma unroll 1
    for (int kb = 0; kb < nblk; ++kb) {
        const bool more = kb + 1 < nblk;
        RowStage<HD> sk;
        if (more) sk.load(src + C, 3L * C, (kb + 1) * BLKT, N, tid);
        const bf16* Ks = Kr + (kb & 1) * IMG;
        if (live) {
            f32x4 p[NT16];
            float mb = -3.0e38f;
#pragma unroll
            for (int i = 0; i < NT16; ++i) {
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) mma(frag_kc<bf16>(Ks, LDQ, 16 * i, 32 * ks, c, g), qf[ks], s);
                const int key0 = kb * BLKT + 16 * i + 4 * g;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r] = key0 + r < N ? s[r] * scale : -1.0e30f;
                    mb = fmaxf(mb, s[r]);
                }
                p[i] = s;
            }
            mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
            mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
            const float mn = fmaxf(m, mb);
            const float alpha = __expf(m - mn);  // (first block: 0 on l = u = 0, and (m - mn) l = -0)
            float sum = 0.f, usum = 0.f;
#pragma unroll
            for (int i = 0; i < NT16; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = p[i][r] - mn;
                    const float e = __expf(d);  // a slot >= N: exp(-1e30) = 0, 0 * -1e30 = -0
                    sum += e;
                    usum += e * d;
                }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            usum += __shfl_xor(usum, 16, 64);
            usum += __shfl_xor(usum, 32, 64);
            uu = alpha * (uu + (m - mn) * l) + usum;
            l = l * alpha + sum;
            m = mn;
        }
        if (more) sk.store(Kr + ((kb + 1) & 1) * IMG, tid);
        __syncthreads();
    }
    const int qt = q0 + 16 * wave + c;
    if (!live || g != 0 || qt >= N) return;
    const float ll = __logf(l);
    ent[(long)u.z * slab + qt] = ll - uu / l;
    if (lse_out) lse_out[(long)u.z * N + qt] = m + ll;
}

// probability rows of nq listed queries (the same list for every image and head): one workgroup per (image, head, 16 listed queries),
// whose Q rows are gathered straight into the operand fragment; the four waves take one 16-key tile each of every 64-key block of the
// K ring.  Two sweeps over K: the first for the row maximum and sum (online per wave, then combined across the waves through LDS), the
// second recomputes the scores and writes p = e^(s - m) / l.  Scores are formed as S = Q K^T (acc[r] = query 4g + r, key c), so that a
// store instruction writes 16 consecutive floats of a row.  rows: row 1 of the (image, head) slab; row j of the list is slab row 1 + j.
// An index outside [0, N) reads as a zero query row (never out of bounds; the callers validate the list).
template <int HD>
__global__ __launch_bounds__(NTHR) void stats_rows_kernel(const bf16* __restrict__ qkv, const int32_t* __restrict__ qidx, int nq, int ntile,
                                                          int N, int nH, int nblk, float scale, long slab, float* __restrict__ rows) {
    // the second sweep has to rebuild the first sweep's scaled scores bit for bit (the maximum's own term is e^0 = 1 exactly, a one-token
    // image gives p = 1): s * scale - m must not become one fused multiply-add, which would subtract m from the UNROUNDED product
#pragma clang fp contract(off)
    using Cfg = FCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, IMG = Cfg::IMG;
    __shared__ __attribute__((aligned(16))) bf16 Kr[2 * IMG];
    __shared__ float red[2][WAVES][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;

    const Unit u = unit_of(blockIdx.x, ntile, nH);
    const int C = nH * HD;
    const bf16* src = qkv + (long)u.b * N * 3 * C + u.h * HD;
    Frag<bf16> qf[KS];
    {
        const int j = 16 * u.blk + c;
        const int t = j < nq ? qidx[j] : -1;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks].v = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
            if (t >= 0 && t < N) qf[ks].v = *reinterpret_cast<const bf16x8*>(src + (long)t * 3 * C + 32 * ks + 8 * g);
        }
    }
    {
        RowStage<HD> sk;
        sk.load(src + C, 3L * C, 0, N, tid);
        sk.store(Kr, tid);
    }
    __syncthreads();

    float m[4], l[4], inv[4];  // of the listed queries 16 tile + 4g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        m[r] = -3.0e38f;
        l[r] = 0.f;
        inv[r] = 0.f;
    }
    float* out[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 16 * u.blk + 4 * g + r;
        out[r] = j < nq ? rows + (long)u.z * slab + (long)j * N : nullptr;
    }

#pragma unroll 1
    for (int step = 0; step < 2 * nblk; ++step) {
        const bool second = step >= nblk;
        const int kb = second ? step - nblk : step;
        const bool more = step + 1 < 2 * nblk;
        const int nkb = kb + 1 < nblk ? kb + 1 : 0;  // (the second sweep starts over at block 0)
        RowStage<HD> sk;
        if (more) sk.load(src + C, 3L * C, nkb * BLKT, N, tid);
        const bf16* Ks = Kr + (step & 1) * IMG;
        if (step == nblk) {  // the partial (m, l) of the four waves, written before the barrier that ended the first sweep
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mm = -3.0e38f;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) mm = fmaxf(mm, red[0][w][4 * g + r]);
                float ls = 0.f;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) ls += red[1][w][4 * g + r] * __expf(red[0][w][4 * g + r] - mm);
                m[r] = mm;
                inv[r] = 1.f / ls;  // (ls >= 1: the wave that holds the maximum adds e^0)
            }
        }
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) mma(qf[ks], frag_kc<bf16>(Ks, LDQ, 16 * wave, 32 * ks, c, g), s);
        const int key = kb * BLKT + 16 * wave + c;
        const bool valid = key < N;
        if (!second) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sr = valid ? s[r] * scale : -1.0e30f;
                float mb = sr;
#pragma unroll
                for (int x = 1; x < 16; x <<= 1) mb = fmaxf(mb, __shfl_xor(mb, x, 64));
                const float mn = fmaxf(m[r], mb);
                float e = valid ? __expf(sr - mn) : 0.f;
#pragma unroll
                for (int x = 1; x < 16; x <<= 1) e += __shfl_xor(e, x, 64);
                l[r] = l[r] * __expf(m[r] - mn) + e;
                m[r] = mn;
            }
            if (step == nblk - 1 && c == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    red[0][wave][4 * g + r] = m[r];
                    red[1][wave][4 * g + r] = l[r];
                }
            }
        } else if (valid) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (out[r]) out[r][key] = __expf(s[r] * scale - m[r]) * inv[r];
        }
        if (more) sk.store(Kr + ((step + 1) & 1) * IMG, tid);
        __syncthreads();
    }
}

template <int HD>
constexpr size_t lds_bytes(int images, bool stats) {
    return (size_t)images * FCfg<HD>::IMG * 2 + (stats ? 4 * BLKT * 4 : 0);
}

inline int blocks_of(int N) { return (N + BLKT - 1) / BLKT; }

template <int HD>
int fwd_launch(const bf16* qkv, int N, int nB, int nH, float scale, bf16* out, float* lse, hipStream_t stream) {
    const int nblk = blocks_of(N);
    auto kern = flash_fwd_kernel<HD>;
    constexpr size_t lds = lds_bytes<HD>(5, false);
    static unsigned long long raised = 0;
    esvit_raise_lds(kern, (int)lds, raised);
    hipLaunchKernelGGL(kern, dim3(nB * nH * nblk), dim3(NTHR), lds, stream, qkv, N, nH, nblk, scale, out, lse);
    ESVIT_CHECK_LAUNCH("window_attn_fwd(global)");
    return ESVIT_OK;
}

template <int HD>
int bwd_launch(const bf16* qkv, const bf16* dout, const bf16* fout, const float* lse, int N, int nB, int nH, float scale, bf16* dqkv,
               float* delta, hipStream_t stream) {
    const int nblk = blocks_of(N);
    {
        const int ntile = (N + 15) / 16;
        const long nunits = (long)nB * nH * ntile;
        hipLaunchKernelGGL(flash_delta_kernel<HD>, dim3(ceil_div(nunits, WAVES)), dim3(NTHR), 0, stream, dout, fout, N, nH, ntile, nunits, delta);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(global, delta)");
    }
    {
        auto kern = flash_bwd_dq_kernel<HD>;
        constexpr size_t lds = lds_bytes<HD>(6, false);
        static unsigned long long raised = 0;
        esvit_raise_lds(kern, (int)lds, raised);
        hipLaunchKernelGGL(kern, dim3(nB * nH * nblk), dim3(NTHR), lds, stream, qkv, dout, lse, (const float*)delta, N, nH, nblk, scale, dqkv);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(global, dQ)");
    }
    {
        auto kern = flash_bwd_dkv_kernel<HD>;
        constexpr size_t lds = lds_bytes<HD>(6, true);
        static unsigned long long raised = 0;
        esvit_raise_lds(kern, (int)lds, raised);
        hipLaunchKernelGGL(kern, dim3(nB * nH * nblk), dim3(NTHR), lds, stream, qkv, dout, lse, (const float*)delta, N, nH, nblk, scale, dqkv);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(global, dK dV)");
    }
    return ESVIT_OK;
}

template <int HD>
int stats_launch(const bf16* qkv, const int32_t* qidx, int nq, int N, int nB, int nH, float scale, float* attn_out, float* lse,
                 hipStream_t stream) {
    const int nblk = blocks_of(N);
    const long slab = (long)(1 + nq) * N;
    hipLaunchKernelGGL(stats_entropy_kernel<HD>, dim3(nB * nH * nblk), dim3(NTHR), 0, stream, qkv, N, nH, nblk, scale, slab, attn_out, lse);
    ESVIT_CHECK_LAUNCH("window_attn_fwd(global, stats: entropy)");
    if (nq > 0) {
        const int ntile = (nq + 15) / 16;
        hipLaunchKernelGGL(stats_rows_kernel<HD>, dim3(nB * nH * ntile), dim3(NTHR), 0, stream, qkv, qidx, nq, ntile, N, nH, nblk, scale, slab,
                           attn_out + N);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(global, stats: rows)");
    }
    return ESVIT_OK;
}

// argument checks shared by the entries; no HIP call before they pass.  stats: the statistics mode (forward only), nW = 1 + listed queries
int check_mode(const char* who, int dtype, int L, int ws, int nW, int nB, int N, int nH, int hd, bool stats = false) {
    ESVIT_CHECK_ARG(!(ws & ESVIT_ATTN_SLIDING_CHUNK), "%s: both mode flags at once (ESVIT_ATTN_GLOBAL | ESVIT_ATTN_SLIDING_CHUNK)", who);
    ESVIT_CHECK_ARG(stats || !(ws & ESVIT_ATTN_STATS), "%s (global): ESVIT_ATTN_STATS is a mode of esvit_window_attn_fwd only", who);
    ESVIT_CHECK_ARG(ws == (stats ? ESVIT_ATTN_GLOBAL | ESVIT_ATTN_STATS : ESVIT_ATTN_GLOBAL), "%s (global): ws carries the mode flag%s alone, not 0x%x",
                    who, stats ? "s" : "", (unsigned)ws);
    ESVIT_CHECK_ARG(dtype == ESVIT_BF16, "%s (global): bf16 only (the fp32 parity mode keeps the batched-GEMM route)", who);
    ESVIT_CHECK_ARG(hd == 32 || hd == 64, "%s (global): head_dim %d unsupported (32 or 64)", who, hd);
    ESVIT_CHECK_ARG(L >= 1, "%s (global): L=%d, at least one token per image", who, L);
    if (stats)
        ESVIT_CHECK_ARG(nW >= 1 && N == L && nB > 0 && nH > 0,
                        "%s (global, stats): bad geometry L=%d nW=%d N=%d nB=%d nH=%d (nW = 1 + listed queries >= 1, N = L)", who, L, nW, N, nB, nH);
    else
        ESVIT_CHECK_ARG(nW == 1 && N == L && nB > 0 && nH > 0, "%s (global): bad geometry L=%d nW=%d N=%d nB=%d nH=%d (nW = 1, N = L)", who, L, nW, N, nB, nH);
    ESVIT_CHECK_ARG((long)L * 3 * nH * hd * 2 < 0x7fff0000L, "%s (global): one image's qkv rows must fit a 2 GiB buffer descriptor", who);
    ESVIT_CHECK_ARG((long)nB * nH * blocks_of(L) < 0x7fffffffL, "%s (global): too many (image, head, block) units for one grid", who);
    return ESVIT_OK;
}

}  // namespace

// the statistics mode of the forward entry (ws = ESVIT_ATTN_GLOBAL | ESVIT_ATTN_STATS, include/esvit_hip.h)
int esvit_flash_attn_stats(int dtype, const void* qkv, const int32_t* queries, int L, int ws, int nW, int nB, int N, int nH, int hd, float scale,
                           const void* out, float* lse, float* attn_out, bool unused_are_null, hipStream_t stream) {
    const char* who = "esvit_window_attn_fwd";
    const int rc = check_mode(who, dtype, L, ws, nW, nB, N, nH, hd, true);
    if (rc != ESVIT_OK) return rc;
    const int nq = nW - 1;
    ESVIT_CHECK_ARG(!out, "%s (global, stats): out must be NULL (the mode reads q and k only and writes no attention output)", who);
    ESVIT_CHECK_ARG(attn_out, "%s (global, stats): attn_out (fp32 [nB, nH, nW, L]) is required", who);
    ESVIT_CHECK_ARG(qkv && (queries || nq == 0), "%s (global, stats): qkv is required, and win2tok (the query list) for nW - 1 = %d queries", who, nq);
    ESVIT_CHECK_ARG(unused_are_null, "%s (global, stats): qkv_bias, rel_table, region_ids and bias_frag_ws are not used, pass NULL", who);
    ESVIT_CHECK_ARG((long)nB * nH * ((nq + 15) / 16) < 0x7fffffffL, "%s (global, stats): too many (image, head, query tile) units for one grid", who);
    if (hd == 32) return stats_launch<32>((const bf16*)qkv, queries, nq, L, nB, nH, scale, attn_out, lse, stream);
    return stats_launch<64>((const bf16*)qkv, queries, nq, L, nB, nH, scale, attn_out, lse, stream);
}

// esvit_query(ESVIT_Q_GLOBAL_ATTN_WS, nB * nH, L, backward): floats of the scratch the mode takes through bias_frag_ws (delta)
int64_t esvit_i_global_attn_ws(int64_t Z, int64_t L, int64_t backward) {
    if (Z <= 0 || L <= 0) return 0;
    return backward ? Z * L : 0;
}

int esvit_flash_attn_fwd(int dtype, const void* qkv, int L, int ws, int nW, int nB, int N, int nH, int hd, float scale, void* out, float* lse,
                         float* attn_out, hipStream_t stream) {
    const int rc = check_mode("esvit_window_attn_fwd", dtype, L, ws, nW, nB, N, nH, hd);
    if (rc != ESVIT_OK) return rc;
    ESVIT_CHECK_ARG(lse && out, "esvit_window_attn_fwd (global): lse and out are required");
    ESVIT_CHECK_ARG(qkv && !attn_out, "esvit_window_attn_fwd (global): qkv is required, attn_out is not available");
    if (hd == 32) return fwd_launch<32>((const bf16*)qkv, L, nB, nH, scale, (bf16*)out, lse, stream);
    return fwd_launch<64>((const bf16*)qkv, L, nB, nH, scale, (bf16*)out, lse, stream);
}

int esvit_flash_attn_bwd(int dtype, const void* qkv, int L, const void* dout, const void* fwd_out, const float* lse, int ws, float* scratch,
                         int nW, int nB, int N, int nH, int hd, float scale, void* dqkv, hipStream_t stream) {
    const int rc = check_mode("esvit_window_attn_bwd", dtype, L, ws, nW, nB, N, nH, hd);
    if (rc != ESVIT_OK) return rc;
    ESVIT_CHECK_ARG(lse && fwd_out, "esvit_window_attn_bwd (global): lse and out (fwd_out) are required");
    ESVIT_CHECK_ARG(qkv && dout && dqkv && scratch, "esvit_window_attn_bwd (global): qkv, dout, dqkv and the scratch (bias_frag_ws) are required");
    if (hd == 32)
        return bwd_launch<32>((const bf16*)qkv, (const bf16*)dout, (const bf16*)fwd_out, lse, L, nB, nH, scale, (bf16*)dqkv, scratch, stream);
    return bwd_launch<64>((const bf16*)qkv, (const bf16*)dout, (const bf16*)fwd_out, lse, L, nB, nH, scale, (bf16*)dqkv, scratch, stream);
}
