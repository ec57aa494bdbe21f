// Fused Swin MLP branch backward with the weight gradients accumulated on the chip (bf16, C = 96: stage 0 of Swin-T / -S).
//
// mlp_fused16.hip's backward writes GELU(A), dA and xhat (18 B per token-channel) only so that two split-K GEMMs can read them back.
// Here ONE persistent workgroup per CU keeps its share of dW2 = dy^T GELU(A) and of G = dA^T xhat in registers across a static loop
// over 64-token tiles (workgroup b takes tiles b, b + grid, ...: the summation order depends on (M, grid) only), so x and gy are read
// once and nothing hidden-sized leaves the chip.  Workgroup b writes partial b; a second launch sums the partials in index order.  No
// atomics, no inter-workgroup synchronisation.
//
// Work split (8 waves, 2 per SIMD, at most 256 registers each).  Wave w owns hidden units 48w .. 48w + 47:
//   * accumulators dW2^T[slice][96] and G[slice][96] as 2 x 3 x 6 MFMA tiles = 144 registers, updated in place by the MFMA builtin.
//     (Pinning them to the AccVGPR half with inline-asm "+a" operands, as gemm_p8.hip does, does not work at two waves per SIMD: hipcc
//     then splits the 256 registers 128 / 128 and spills 16 accumulators.  With the builtin the kernel has no AccVGPR operand, all 256
//     are ordinary registers, and the ISA holds no accumulator copies: 254 registers, ScratchSize 0.)
//   * W1 [384][96] is resident in LDS once and serves two products: its rows are the B fragments of the pre-activation (16-byte
//     reads) and, read through ds_read_tr16_b64, the A fragments of dxhat^T = W1^T dA^T.  The wave's 48 rows of W2^T are nine B
//     fragments = 36 registers that do not fit beside the accumulators; the 12 of one hidden tile are re-read from L2 once per tile.
// Per tile:
//   L  512 threads (8 per token) take x and gy (requested during phase D of the tile before: 25 registers, free there), LayerNorm in
//      registers; LN(x), xhat and rowscale * gy go to LDS as bf16 [64][96]
//   C  per 16-token sub-tile and 16-hidden tile, with the TOKENS as MFMA rows:  P = LN(x) W1_slice^T,  Q = dy W2_slice;  GELU and GELU'
//      (gelu_both);  lane (c, g) then holds hidden unit c, tokens 4g + r -- two sub-tiles side by side ARE an A fragment of the two
//      products that contract over the tokens (mfma.h: frag_p_regs), whose B fragments are transpose reads of the dy / xhat images with
//      the same token permutation (frag_v_perm).  dA also goes to LDS as [64 tok][384] (the one transposition of the kernel).
//   D  wave w forms dxhat^T for tokens 16 (w >> 1) .. + 15 and channel tiles 3 (w & 1) .. + 2 over all 384 hidden units, then the
//      LayerNorm backward and the residual add as mlp_fused16.hip's epilogue; the two waves of a token exchange their row sums in LDS.
// Rounding points are those of mlp_fused16.hip / oracle mlp_fused_bwd: LN(x), xhat, GELU(A), dA and the scaled dy are rounded to
// bf16 before they enter an MFMA; db1 / db2 sum the rounded dA / dy in fp32, as the GEMMs' column sums did.  Rows past M enter with
// dy = 0 (so dA = 0): they add nothing to any sum and are not stored.
//
// LDS (160 KiB): W1 72 KiB | LN(x), xhat, dy 3 x 12 KiB | dA 49 KiB (rows padded to 784 B) | row statistics and sums 1.5 KiB.
// The [*][96] images use the 16-byte-unit XOR of fused16.h's image A (unit ^ (row >> 2) inside aligned groups of four).
#include "common.h"
#include "img96.h"
#include "../../include/esvit_hip.h"

namespace {

constexpr int DW_C = 96, DW_H = 384, DW_T = 64, DW_NW = 8;
constexpr int DW_OFF_W2 = 0, DW_OFF_G = DW_C * DW_H, DW_OFF_B1 = 2 * DW_C * DW_H, DW_OFF_B2 = DW_OFF_B1 + DW_H;
constexpr int DW_PART = DW_OFF_B2 + DW_C;  // floats per workgroup partial: dW2 [96][384] | G [384][96] | db1 [384] | db2 [96]

constexpr int DA_ROW = 784;  // bytes per dA row: 768 + 16 (rows 196 dwords apart: the 16 lanes of a 16-byte read hit 16 different bank quads)
constexpr int L_W1 = 0, L_XW = L_W1 + DW_H * 192, L_XH = L_XW + DW_T * 192, L_DY = L_XH + DW_T * 192, L_DA = L_DY + DW_T * 192,
              L_ST = L_DA + DW_T * DA_ROW, L_EX = L_ST + 2 * DW_T * 4, L_END = L_EX + DW_NW * 16 * 8;
static_assert(L_END <= 160 * 1024, "LDS budget");

// Phases C and D address the images (img96.h) as a lane-dependent base plus a compile-time constant that goes into the 16-bit offset
// field of the LDS instruction: a phase C trip forms its five bases (6 integer instructions, 77 before), phase D advances its seven
// bases once per six k-steps.  16 rows further is IMG_ROWS16 bytes, 32 channels further IMG_CH32; of a 16-channel step only its parity
// reaches the XOR (two bases, 32 bytes apart under XOR);  in phase D, where a transpose read's rows step by 4, the second row of a
// pair has a base of its own and 32 rows further is +6144.  The images lie a constant apart, so one base serves all of them.
constexpr bool img_immediates_hold() {
    for (int c = 0; c < 16; ++c)
        for (int g = 0; g < 4; ++g) {
            // A / B fragment reads of C: row 16 k + c, channels 32 ks + 8 g
            for (int k = 0; k < 24; ++k)
                for (int ks = 0; ks < 3; ++ks)
                    if (img_off(16 * k + c, 32 * ks + 8 * g) != img_off(c, 8 * g) + IMG_ROWS16 * k + IMG_CH32 * ks) return false;
            // transpose reads of C: rows 32 p + 4 g + (c >> 2) and 16 on, channels 16 n + 4 (c & 3)
            for (int k = 0; k < 4; ++k)
                for (int n = 0; n < 6; ++n)
                    if (img_off(16 * k + 4 * g + (c >> 2), 16 * n + 4 * (c & 3)) !=
                        img_off(4 * g + (c >> 2), 16 * (n & 1) + 4 * (c & 3)) + IMG_ROWS16 * k + IMG_CH32 * (n >> 1))
                        return false;
            if (img_off(4 * g + (c >> 2), 16 + 4 * (c & 3)) != (img_off(4 * g + (c >> 2), 4 * (c & 3)) ^ 32)) return false;
            // transpose reads of D: rows 32 ks + 8 g + (c >> 2) and 4 on, channels 16 n + 4 (c & 3)
            for (int ks = 0; ks < 12; ++ks)
                for (int n = 0; n < 6; ++n)
                    for (int rw = 0; rw < 2; ++rw)
                        if (img_off(32 * ks + 8 * g + (c >> 2) + 4 * rw, 16 * n + 4 * (c & 3)) !=
                            img_off(8 * g + (c >> 2) + 4 * rw, 16 * n + 4 * (c & 3)) + 2 * IMG_ROWS16 * ks)
                            return false;
        }
    return true;
}
static_assert(img_immediates_hold(), "base + immediate addressing of the [*][96] images");

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void mfma_acc(const bf16x8& a, const bf16x8& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// the L phase's share of one tile: 12 channels of x and gy of token (t >> 3) and the token's DropPath factor; rows past M read row M - 1
// (no address beyond the operands is formed) and get factor 0
__device__ __forceinline__ void request_rows(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ rs_mlp, long M,
                                             int tile, int t, f32x4 (&xv)[3], f32x4 (&gv)[3], float& sm) {
    const long row = (long)tile * DW_T + (t >> 3);
    const bool ok = row < M;
    const long rrow = ok ? row : (M - 1);
    const float* xr = x + rrow * DW_C + 12 * (t & 7);
    const float* gr = gy + rrow * DW_C + 12 * (t & 7);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        xv[q] = *reinterpret_cast<const f32x4*>(xr + 4 * q);
        gv[q] = *reinterpret_cast<const f32x4*>(gr + 4 * q);
    }
    sm = ok ? (rs_mlp ? rs_mlp[rrow] : 1.f) : 0.f;  // (rows past M contribute nothing: dy = 0 gives dA = 0)
}

__global__ __launch_bounds__(DW_NW * 64, 1) void mlp_dw_kernel(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ rs_mlp,
                                                               const float* __restrict__ rs_out, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, const bf16* __restrict__ W1p,
                                                               const bf16* __restrict__ W2Tp, const float* __restrict__ b1, long M, int ntiles,
                                                               float* __restrict__ gx, bf16* __restrict__ gxa, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int hid0 = 48 * wave;

    // ---- once: W1 into LDS in natural channel order (the copy's 32-blocks are permuted: position 8gg + e holds channel 4gg + e / 16 + 4gg + e - 4)
#pragma unroll
    for (int i = 0; i < (DW_H * 12) / (DW_NW * 64); ++i) {
        const int p = tid + DW_NW * 64 * i;
        const int h = p / 12, u = p % 12;
        const u32x4 v = *reinterpret_cast<const u32x4*>(W1p + h * DW_C + 8 * u);
        const int ch = 32 * (u >> 2) + 4 * (u & 3);
        *reinterpret_cast<u32x2*>(smem + L_W1 + img_off(h, ch)) = u32x2{v[0], v[1]};
        *reinterpret_cast<u32x2*>(smem + L_W1 + img_off(h, ch + 16)) = u32x2{v[2], v[3]};
    }
    // this wave's rows of W2^T as B fragments: hidden unit c of tile t, channels 32 ks + 8g .. + 7 = two 8-byte pieces of the permuted copy's
    // row.  Held for the whole loop their 36 registers do not fit beside the accumulators (the allocator spilled them, and address registers
    // with them), so a tile re-reads the 12 of one hidden tile from L2, where the 72 KiB copy that every workgroup reads stays resident.
    // (The row pointer `w2row` itself is formed per tile, below: the pointers derived from it were spilled when it lived across the loop.)
    float b1v[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) b1v[t] = b1[hid0 + 16 * t + c];

    f32x4 accW[3][6], accG[3][6];  // [hidden tile][channel tile]: element r <-> hidden 16 t + 4g + r, channel 16 n + c
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            accW[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            accG[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    float db1s[3] = {0.f, 0.f, 0.f};
    float db2s = 0.f;

    // the rows of a tile are requested one trip ahead, at the start of phase D of the tile before (which holds the accumulators and
    // little else), so that phase L does not wait for a round trip to HBM with nothing else in flight; the last tile requests nothing
    f32x4 xv[3], gv[3];
    float sm;
    if ((int)blockIdx.x < ntiles) request_rows(x, gy, rs_mlp, M, blockIdx.x, tid, xv, gv, sm);

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long row0 = (long)tile * DW_T;
        // (opaque per tile: hoisted out of the loop, the LayerNorm parameters would hold 36 registers across it)
        const float* gamma_t = gamma;
        const float* beta_t = beta;
        asm volatile("" : "+s"(gamma_t), "+s"(beta_t));
        int tid_t = tid;  // (likewise the lane-dependent global addresses of the L and D phases: recomputed per tile, not kept -- and spilled -- across it)
        asm volatile("" : "+v"(tid_t));
        // ---- L: inputs -> LDS (8 lanes per token, 12 channels each)
        {
            const int tok = tid_t >> 3, sub = tid_t & 7;
            float s1 = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) s1 += (xv[q][0] + xv[q][1]) + (xv[q][2] + xv[q][3]);
            s1 += __shfl_xor(s1, 1, 64);
            s1 += __shfl_xor(s1, 2, 64);
            s1 += __shfl_xor(s1, 4, 64);
            const float mean = s1 * (1.f / DW_C);
            float s2 = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = xv[q][e] - mean;
                    s2 += d * d;
                }
            s2 += __shfl_xor(s2, 1, 64);
            s2 += __shfl_xor(s2, 2, 64);
            s2 += __shfl_xor(s2, 4, 64);
            const float rstd = rsqrtf(s2 * (1.f / DW_C) + eps);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int ch = 12 * sub + 4 * q;
                const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma_t + ch), bt = *reinterpret_cast<const f32x4*>(beta_t + ch);
                float h[4], w[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    h[e] = (xv[q][e] - mean) * rstd;
                    w[e] = h[e] * gm[e] + bt[e];
                }
                const int o = img_off(tok, ch);
                *reinterpret_cast<u32x2*>(smem + L_XW + o) = u32x2{esvit_pack2_bf16(w[0], w[1]), esvit_pack2_bf16(w[2], w[3])};
                *reinterpret_cast<u32x2*>(smem + L_XH + o) = u32x2{esvit_pack2_bf16(h[0], h[1]), esvit_pack2_bf16(h[2], h[3])};
                *reinterpret_cast<u32x2*>(smem + L_DY + o) =
                    u32x2{esvit_pack2_bf16(sm * gv[q][0], sm * gv[q][1]), esvit_pack2_bf16(sm * gv[q][2], sm * gv[q][3])};
            }
            if (sub == 0) {
                reinterpret_cast<float*>(smem + L_ST)[tok] = mean;
                reinterpret_cast<float*>(smem + L_ST)[DW_T + tok] = rstd;
            }
        }
        __syncthreads();

        // ---- db2: column sums of the rounded dy (4 x 96 threads, 16 tokens each)
        if (tid < 4 * DW_C) {
            const int ch = tid % DW_C, r0 = 16 * (tid / DW_C);
#pragma unroll
            for (int k = 0; k < 16; ++k) db2s += (float)*reinterpret_cast<const bf16*>(smem + L_DY + img_off(r0 + k, ch));
        }

        // ---- C: hidden tiles of this wave's slice; the token-contracting products
        // lane bases of the tile (from the opaque tid_t: kept across the tile loop they would be spilled)
        const int c_t = tid_t & 15, g_t = (tid_t >> 4) & 3;
        const int frag_b = img_off(c_t, 8 * g_t);                             // row c, channels 8g: A fragments of P / Q, W1's B fragments
        const int tr_b = img_off(4 * g_t + (c_t >> 2), 4 * (c_t & 3));        // transpose reads, even channel tiles (odd: ^ 32)
        const int da_b = L_DA + 4 * g_t * DA_ROW + (hid0 + c_t) * 2;          // dA column of this lane's hidden unit, token 4g
        const char* w1_frag = smem + L_W1 + hid0 * 192 + frag_b;
        const bf16* w2row = W2Tp + (hid0 + c_t) * DW_C + (g_t < 2 ? 16 * g_t : 16 * (g_t - 2) + 4);  // (see above; per tile like the bases)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            bf16x8 w2f[3];
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) {
                const bf16* wr = w2row + 16 * t * DW_C + 32 * ks;
                const u32x2 lo = *reinterpret_cast<const u32x2*>(wr), hi = *reinterpret_cast<const u32x2*>(wr + 8);
                w2f[ks] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
            }
#pragma unroll 1
            for (int p = 0; p < 2; ++p) {
                bf16x8 hfA, dfA;  // hidden unit hid0 + 16 t + c, tokens 32 p + {4g + r, 16 + 4g + r}: A fragments over the pair's tokens
                const char* xw_frag = smem + L_XW + 2 * IMG_ROWS16 * p + frag_b;   // the pair's first row of LN(x); dy lies L_DY - L_XW on
                const char* xh_tr = smem + L_XH + 2 * IMG_ROWS16 * p + tr_b;       // likewise xhat for the transpose reads
                char* da_pair = smem + 32 * DA_ROW * p + da_b;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    f32x4 P = f32x4{0.f, 0.f, 0.f, 0.f}, Q = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 3; ++ks) {
                        const bf16x8 a = *reinterpret_cast<const bf16x8*>(xw_frag + IMG_ROWS16 * jj + IMG_CH32 * ks);
                        const bf16x8 d = *reinterpret_cast<const bf16x8*>(xw_frag + (L_DY - L_XW) + IMG_ROWS16 * jj + IMG_CH32 * ks);
                        const bf16x8 b = *reinterpret_cast<const bf16x8*>(w1_frag + IMG_ROWS16 * t + IMG_CH32 * ks);
                        P = mfma(a, b, P);
                        Q = mfma(d, w2f[ks], Q);
                    }
                    char* da_col = da_pair + 16 * DA_ROW * jj + 32 * t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float gl, dg;
                        gelu_both(P[r] + b1v[t], gl, dg);
                        const bf16 da = (bf16)(Q[r] * dg);
                        hfA[4 * jj + r] = (bf16)gl;
                        dfA[4 * jj + r] = da;
                        db1s[t] += (float)da;
                        *reinterpret_cast<bf16*>(da_col + r * DA_ROW) = da;
                    }
                }
                // (the B fragments are re-read for every hidden tile: keeping the pair's six of each live costs 48 registers the loop does not have)
                const char* xh_tr_odd = smem + L_XH + 2 * IMG_ROWS16 * p + (tr_b ^ 32);
#pragma unroll
                for (int n = 0; n < 6; ++n) {
                    const char* tr = ((n & 1) ? xh_tr_odd : xh_tr) + IMG_CH32 * (n >> 1);
                    const bf16x8 bd = tr_pair(tr + (L_DY - L_XH), tr + (L_DY - L_XH) + IMG_ROWS16);
                    const bf16x8 bx = tr_pair(tr, tr + IMG_ROWS16);
                    mfma_acc(hfA, bd, accW[t][n]);
                    mfma_acc(dfA, bx, accG[t][n]);
                }
            }
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) request_rows(x, gy, rs_mlp, M, tile + gridDim.x, tid_t, xv, gv, sm);

        // ---- D: dxhat^T [channels][tokens] for 16 tokens x 48 channels per wave, LayerNorm backward, residual add
        {
            const int j = wave >> 1, n0 = 3 * (wave & 1);
            const int c = tid_t & 15, g = (tid_t >> 4) & 3;
            f32x4 acc3[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) acc3[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            // bases of the dA row and of W1's transpose reads (both rows of a pair, three channel tiles); 32 hidden units further is
            // +64 / +6144 bytes, which leaves the offset field after ten steps: the bases advance once, half way
            const char* da_row = smem + L_DA + (16 * j + c) * DA_ROW + 16 * g;
            const char* w1_tr[3][2];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int rw = 0; rw < 2; ++rw) w1_tr[i][rw] = smem + L_W1 + img_off(8 * g + (c >> 2) + 4 * rw, 16 * (n0 + i) + 4 * (c & 3));
            constexpr int KH = DW_H / 64;
#pragma unroll 1
            for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
                for (int ks = 0; ks < KH; ++ks) {
                    const bf16x8 b = *reinterpret_cast<const bf16x8*>(da_row + IMG_CH32 * ks);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const bf16x8 a = tr_pair(w1_tr[i][0] + 2 * IMG_ROWS16 * ks, w1_tr[i][1] + 2 * IMG_ROWS16 * ks);
                        acc3[i] = mfma(a, b, acc3[i]);
                    }
                }
                da_row += IMG_CH32 * KH;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    w1_tr[i][0] += 2 * IMG_ROWS16 * KH;
                    w1_tr[i][1] += 2 * IMG_ROWS16 * KH;
                }
            }
            const int tok = 16 * j + c;
            const long row = row0 + tok;
            const bool ok = row < M;
            const long rrow = ok ? row : (M - 1);
            const float mean = reinterpret_cast<const float*>(smem + L_ST)[tok], rstd = reinterpret_cast<const float*>(smem + L_ST)[DW_T + tok];
            float xh[3][4], gd[3][4];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int c0 = 16 * (n0 + i) + 4 * g;
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + rrow * DW_C + c0);
                const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma_t + c0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    xh[i][r] = (xv[r] - mean) * rstd;
                    gd[i][r] = acc3[i][r] * gm[r];
                    s1 += gd[i][r];
                    s2 += gd[i][r] * xh[i][r];
                }
            }
            s1 += __shfl_xor(s1, 16, 64);
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 16, 64);
            s2 += __shfl_xor(s2, 32, 64);
            f32x2* ex = reinterpret_cast<f32x2*>(smem + L_EX);
            if (g == 0) ex[wave * 16 + c] = f32x2{s1, s2};
            __syncthreads();
            const f32x2 e0 = ex[(wave & ~1) * 16 + c], e1 = ex[(wave | 1) * 16 + c];
            const float m1 = (e0[0] + e1[0]) * (1.f / DW_C), m2 = (e0[1] + e1[1]) * (1.f / DW_C);
            const float ro = rs_out ? rs_out[rrow] : 1.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int c0 = 16 * (n0 + i) + 4 * g;
                const f32x4 gv = *reinterpret_cast<const f32x4*>(gy + rrow * DW_C + c0);
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = gv[r] + rstd * (gd[i][r] - m1 - xh[i][r] * m2);
                if (ok) {
                    *reinterpret_cast<f32x4*>(gx + row * DW_C + c0) = o;
                    *reinterpret_cast<u32x2*>(gxa + row * DW_C + c0) = u32x2{esvit_pack2_bf16(ro * o[0], ro * o[1]), esvit_pack2_bf16(ro * o[2], ro * o[3])};
                }
            }
        }
        // (the next tile's L phase overwrites images whose readers all passed the barrier after C; the row statistics were read before
        // the barrier inside D, the exchanged sums are rewritten two barriers from here)
    }

    // ---- partial of this workgroup
    float* pw = part + (long)blockIdx.x * DW_PART;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int h = hid0 + 16 * t + 4 * g;
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            *reinterpret_cast<f32x4*>(pw + DW_OFF_W2 + (16 * n + c) * DW_H + h) = accW[t][n];
#pragma unroll
            for (int r = 0; r < 4; ++r) pw[DW_OFF_G + (h + r) * DW_C + 16 * n + c] = accG[t][n][r];
        }
        float v = db1s[t];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) pw[DW_OFF_B1 + hid0 + 16 * t + c] = v;
    }
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem + L_DA);
    if (tid < 4 * DW_C) red[tid] = db2s;
    __syncthreads();
    if (tid < DW_C) pw[DW_OFF_B2 + tid] = ((red[tid] + red[DW_C + tid]) + red[2 * DW_C + tid]) + red[3 * DW_C + tid];
}

// sums the workgroup partials in index order into the four outputs
__global__ __launch_bounds__(256) void mlp_dw_reduce_kernel(const float* __restrict__ part, int nblk, float* __restrict__ dW2, float* __restrict__ G,
                                                            float* __restrict__ db1, float* __restrict__ db2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= DW_PART) return;
    const float* p = part + i;
    float s = 0.f;
    int b = 0;
    for (; b + 8 <= nblk; b += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(long)(b + k) * DW_PART];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; b < nblk; ++b) s += p[(long)b * DW_PART];
    if (i < DW_OFF_G) dW2[i] = s;
    else if (i < DW_OFF_B1) G[i - DW_OFF_G] = s;
    else if (i < DW_OFF_B2) db1[i - DW_OFF_B1] = s;
    else db2[i - DW_OFF_B2] = s;
}

int dw_grid(long M) {
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
    const long ntiles = (M + DW_T - 1) / DW_T;
    return (int)(ntiles < n ? ntiles : n);
}

}  // namespace

// esvit_query(ESVIT_Q_MLP_DW_WS, dtype, C, M): bytes of partials_ws -- one partial of 74208 floats per workgroup of the launch
int64_t esvit_i_mlp_dw_ws(int dtype, int C, int64_t M) {
    if (dtype != ESVIT_BF16 || C != DW_C || M <= 0) return 0;
    return (int64_t)dw_grid((long)M) * DW_PART * 4;
}

int esvit_i_mlp_dw_bwd(const float* x, const float* gy, const float* rs_mlp, const float* rs_out, const float* gamma, const float* beta, float eps,
                       const void* W1p, const void* W2Tp, const float* b1, long M, float* gx, void* gxa, float* dW2, float* G, float* db1, float* db2,
                       float* ws, hipStream_t stream) {
    const int grid = dw_grid(M);
    const int ntiles = (int)((M + DW_T - 1) / DW_T);
    auto k = mlp_dw_kernel;
    static unsigned long long lds_set = 0;
    esvit_raise_lds(k, L_END, lds_set);
    hipLaunchKernelGGL(k, dim3(grid), dim3(DW_NW * 64), L_END, stream, x, gy, rs_mlp, rs_out, gamma, beta, eps, (const bf16*)W1p, (const bf16*)W2Tp, b1, M,
                       ntiles, gx, (bf16*)gxa, ws);
    ESVIT_CHECK_LAUNCH("esvit_mlp_fused_bwd(dw)");
    hipLaunchKernelGGL(mlp_dw_reduce_kernel, dim3((DW_PART + 255) / 256), dim3(256), 0, stream, ws, grid, dW2, G, db1, db2);
    ESVIT_CHECK_LAUNCH("esvit_mlp_fused_bwd(dw reduce)");
    return ESVIT_OK;
}
