// Tail of the Swin attention-branch backward at stage 0 (bf16, C = 96): everything after the window-attention backward that has no
// window structure, in ONE pass over the rows (the qkv-tail mode of esvit_layernorm_bwd).
//
// The unfused chain reads dqkv twice (data gradient, weight gradient), writes dxw = dqkv Wqkv only to read it back in the LayerNorm
// backward, and reads xw = LayerNorm(x), which the forward stores for the weight gradient alone: 32 B per token-channel in four
// launches and a side-stream hand-over.  Here one persistent workgroup per CU walks 64-row tiles in a static order (workgroup b takes
// tiles b, b + grid, ...: the summation order depends on (M, grid) only) with its share of dWqkv = dqkv^T xw in registers, so dqkv, x
// and g_in are read once and gx (with its activation-dtype copy, when asked for) is the only row-sized output: 18 - 20 B.  Workgroup b
// writes partial b; a second launch sums the partials in index order.  No atomics, no inter-workgroup synchronisation.
//
// Work split (8 waves).  Per tile:
//   L  the tile's 36 KiB of dqkv are contiguous: 512 threads move 4.5 16-byte pieces each from registers (requested two tiles ahead) to
//      the LDS image [64 tok][288] (rows padded to 592 B: 16-byte reads of 16 rows hit 16 different bank quads).  Two images take turns:
//      the next tile's is filled in the middle of phase D of this one, before the stores (see there).
//   D  wave w forms dxw^T = Wqkv^T dqkv^T for tokens 16 (w >> 1) .. + 15 and channel tiles 3 (w & 1) .. + 2 over all 288 qkv units:
//      Wqkv [288][96] is resident in LDS once, its A fragments come through ds_read_tr16_b64 (as mlp_dw_kernel's phase D reads W1).
//      dxw is rounded to bf16 as the data-gradient GEMM's output is.  Lane (c, g) then holds channels 16 n + 4 g + r of token c, for
//      which it received x, mean, rstd and g_in a tile ahead: LayerNorm from the saved statistics with ln_fwd_kernel's expression
//      (the bf16 image of xw goes to LDS for phase C), then ln_bwd_kernel's formula; the two waves of a token exchange their row sums
//      in LDS.  dgamma / dbeta stay in 24 registers per lane.
//   C  dWqkv += dqkv^T xw, contracting over the tile's tokens: both operands are transpose reads of the two images.  The 18 x 6
//      accumulator tiles are split 5 / 5 / 4 / 4 unit tiles x 3 channel tiles over the wave pairs (60 registers).
// dbqkv sums the bf16 dqkv image in fp32 (288 threads, two half-tiles of rows).  Rows past M enter with dqkv = 0 and xw = 0: they add
// nothing to any sum and are not stored; their loads re-read row M - 1 (no address beyond the operands is formed).
//
// LDS (141 KiB): Wqkv 54 KiB | xw 12 KiB | dqkv 2 x 37 KiB | exchanged row sums 1 KiB | gamma, beta 768 B.
#include "common.h"
#include "img96.h"
#include "../../include/esvit_hip.h"

int64_t esvit_i_mlp_dw_ws(int dtype, int C, int64_t M);  // mlp_fused_dw.hip

namespace {

constexpr int AT_C = 96, AT_J = 288, AT_T = 64, AT_NW = 8, AT_NT = AT_NW * 64;
constexpr int AT_OFF_B = AT_J * AT_C, AT_OFF_DG = AT_OFF_B + AT_J, AT_OFF_DB = AT_OFF_DG + AT_C;
constexpr int AT_PART = AT_OFF_DB + AT_C;  // floats per workgroup partial: dWqkv [288][96] | dbqkv [288] | dgamma [96] | dbeta [96]
static_assert(AT_PART == ESVIT_ATTN_TAIL_PARTIAL_FLOATS, "include/esvit_hip.h");

constexpr int DQ_ROW = 592;                            // bytes per dqkv row: 576 + 16 (rows 148 dwords apart)
constexpr int DQ_PIECES = AT_T * AT_J * 2 / 16;        // 16-byte pieces of a tile: 2304 = 4.5 per thread
constexpr int DQ_REGS = (DQ_PIECES + AT_NT - 1) / AT_NT;
constexpr int L_W = 0, L_XW = L_W + AT_J * 192, L_DQ = L_XW + AT_T * 192, L_EX = L_DQ + 2 * AT_T * DQ_ROW, L_GB = L_EX + AT_NW * 16 * 8,
              L_END = L_GB + 2 * AT_C * 4;
static_assert(L_END <= 160 * 1024, "LDS budget");
static_assert((2 * AT_NW * 48 + 2 * AT_J) * 4 <= AT_T * DQ_ROW, "the final fold's scratch lies in the first dqkv image");

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// what a thread keeps of the tile after next
struct TileRegs {
    u32x4 dq[DQ_REGS];  // pieces tid + 512 i of the tile's dqkv
    f32x4 x[3], gi[3];  // phase D's share of x and g_in: token 16 (w >> 1) + c, channels 16 (3 (w & 1) + i) + 4 g .. + 3
    float mean, rstd, sc;  // the token's statistics and the factor of its activation-dtype copy
};

__device__ __forceinline__ void request_dq(const bf16* __restrict__ dqkv, long M, int tile, int tid, TileRegs& t) {
#pragma unroll
    for (int i = 0; i < DQ_REGS; ++i) {
        // (every thread loads in every round -- the upper half of the last one re-reads a piece nobody uses -- so that no branch stands
        // between the requests and the compiler can count them)
        int p = tid + AT_NT * i;
        if (p >= DQ_PIECES) p -= AT_NT / 2;
        const int row = p / 36, u = p - 36 * row;
        const long grow = (long)tile * AT_T + row;
        const long rrow = grow < M ? grow : (M - 1);
        t.dq[i] = *reinterpret_cast<const u32x4*>(dqkv + rrow * AT_J + 8 * u);
    }
}

// the requested pieces -> the LDS image of tile `tile`; rows past M as zeros
__device__ __forceinline__ void store_dq(char* img, long M, int tile, int tid, const TileRegs& t) {
    const long row0 = (long)tile * AT_T;
#pragma unroll
    for (int i = 0; i < DQ_REGS; ++i) {
        const int p = tid + AT_NT * i;
        if (p < DQ_PIECES) {
            const int row = p / 36, u = p - 36 * row;
            *reinterpret_cast<u32x4*>(img + row * DQ_ROW + 16 * u) = (row0 + row < M) ? t.dq[i] : u32x4{0u, 0u, 0u, 0u};
        }
    }
}

__device__ __forceinline__ void request_rows(const float* __restrict__ x, const float* __restrict__ g_in, const float* __restrict__ mean,
                                             const float* __restrict__ rstd, const float* __restrict__ rowscale, int rows_per_sample, long M, int tile,
                                             int tok, int ch0, TileRegs& t) {
    const long grow = (long)tile * AT_T + tok;
    const long rrow = grow < M ? grow : (M - 1);
    const float* xr = x + rrow * AT_C + ch0;
    const float* gr = g_in + rrow * AT_C + ch0;
    // (in the order of their use: a wait for x leaves g_in in flight)
    t.mean = mean[rrow];
    t.rstd = rstd[rrow];
#pragma unroll
    for (int i = 0; i < 3; ++i) t.x[i] = *reinterpret_cast<const f32x4*>(xr + 16 * i);
    t.sc = rowscale ? rowscale[rrow / rows_per_sample] : 1.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) t.gi[i] = *reinterpret_cast<const f32x4*>(gr + 16 * i);
}

__global__ __launch_bounds__(AT_NT, 1) void attn_tail_kernel(const bf16* __restrict__ dqkv, const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ g_in,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const bf16* __restrict__ W, const float* __restrict__ rowscale, int rows_per_sample, long M,
                                                             int ntiles, float* __restrict__ gx, bf16* __restrict__ gxa, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    // phase D: token tile and channel tiles of this wave; phase C: unit tiles [tb, tb + nt) and channel tiles 3 hc .. + 2
    const int tj = wave >> 1, n0 = 3 * (wave & 1);
    const int tok = 16 * tj + c, ch0 = 16 * n0 + 4 * g;
    const int tb = (wave >> 1) < 2 ? 5 * (wave >> 1) : 2 + 4 * (wave >> 1), nt = (wave >> 1) < 2 ? 5 : 4;
    const int hc = wave & 1;

    TileRegs nx;
    request_dq(dqkv, M, blockIdx.x, tid, nx);
    request_rows(x, g_in, mean, rstd, rowscale, rows_per_sample, M, blockIdx.x, tok, ch0, nx);

    // ---- once: Wqkv into LDS (16-byte units of 8 channels keep their order inside the image's unit); all loads first, no branch between them
    {
        constexpr int WR = (AT_J * 12 + AT_NT - 1) / AT_NT;
        u32x4 wv[WR];
#pragma unroll
        for (int i = 0; i < WR; ++i) {
            int p = tid + AT_NT * i;
            if (p >= AT_J * 12) p -= AT_NT;
            wv[i] = *reinterpret_cast<const u32x4*>(W + 8 * p);
        }
        const f32x4 gb = *reinterpret_cast<const f32x4*>(tid < AT_C / 4 ? gamma + 4 * tid : beta + (tid < 2 * AT_C / 4 ? 4 * tid - AT_C : 0));
#pragma unroll
        for (int i = 0; i < WR; ++i) {
            const int p = tid + AT_NT * i;
            if (p < AT_J * 12) {
                const int h = p / 12, u = p - 12 * h;
                *reinterpret_cast<u32x4*>(smem + L_W + img_off(h, 8 * u)) = wv[i];
            }
        }
        if (tid < 2 * AT_C / 4) *reinterpret_cast<f32x4*>(smem + L_GB + 16 * tid) = gb;  // gamma | beta
    }

    f32x4 accW[5][3];  // [unit tile][channel tile]: element r <-> unit 16 (tb + t) + 4g + r, channel 16 (3 hc + n) + c
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int n = 0; n < 3; ++n) accW[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 dgam[3], dbet[3];  // token c's terms of channels 16 (n0 + i) + 4g + r
#pragma unroll
    for (int i = 0; i < 3; ++i) dgam[i] = dbet[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float cs0 = 0.f, cs1 = 0.f;  // threads < 288: column sums of units 2 (tid % 144), + 1 over rows 32 (tid / 144) .. + 31

    // the first tile's dqkv -> image 0; the registers take the second tile's
    store_dq(smem + L_DQ, M, blockIdx.x, tid, nx);
    request_dq(dqkv, M, blockIdx.x + gridDim.x < ntiles ? blockIdx.x + gridDim.x : blockIdx.x, tid, nx);

    int buf = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 1) {
        const long row0 = (long)tile * AT_T;
        char* dq_img = smem + L_DQ + buf * (AT_T * DQ_ROW);
        // (the last tiles request themselves again: no branch around a request)
        const int tnext = tile + (int)gridDim.x < ntiles ? tile + (int)gridDim.x : tile;
        const int tnext2 = tnext + (int)gridDim.x < ntiles ? tnext + (int)gridDim.x : tnext;
        // (opaque per tile, as in mlp_dw_kernel: hoisted out of the loop, the LayerNorm parameters -- read from LDS at a lane-dependent
        // address -- and the lane-dependent LDS and global addresses of the three phases would be held, and spilled, across it)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int c = lane_t & 15, g = lane_t >> 4;
        const int tok = 16 * tj + c, ch0 = 16 * n0 + 4 * g;
        __syncthreads();  // the tile's dqkv image is complete (phase L of the trip before), phase C of the trip before is over

        // ---- dbqkv: column sums of the image
        if (tid < AT_J) {
            const char* col = dq_img + (tid >= 144 ? 32 * DQ_ROW + 4 * (tid - 144) : 4 * tid);
#pragma unroll 8
            for (int k = 0; k < 32; ++k) {
                const unsigned v = *reinterpret_cast<const unsigned*>(col + k * DQ_ROW);
                cs0 += __builtin_bit_cast(float, v << 16);
                cs1 += __builtin_bit_cast(float, v & 0xffff0000u);
            }
        }

        // ---- D: dxw^T [channels][tokens], LayerNorm forward (xw image) and backward, residual add
        const bool ok = row0 + tok < M;
        const long row = row0 + tok;
        f32x4 xh[3], gd[3];
        float mean_t, rstd_t;
        {
            f32x4 acc3[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) acc3[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            const char* dq_row = dq_img + tok * DQ_ROW + 16 * g;
            const char* w_tr[3][2];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int rw = 0; rw < 2; ++rw) w_tr[i][rw] = smem + L_W + img_off(8 * g + (c >> 2) + 4 * rw, 16 * (n0 + i) + 4 * (c & 3));
#pragma unroll 3  // (unrolled in full, the nine steps' fragments are all read ahead: 256 registers and scratch)
            for (int ks = 0; ks < AT_J / 32; ++ks) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(dq_row + 64 * ks);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const bf16x8 a = tr_pair(w_tr[i][0] + 2 * IMG_ROWS16 * ks, w_tr[i][1] + 2 * IMG_ROWS16 * ks);
                    acc3[i] = mfma(a, b, acc3[i]);
                }
            }
            mean_t = nx.mean;
            rstd_t = nx.rstd;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const f32x4 gm = *reinterpret_cast<const f32x4*>(smem + L_GB + (ch0 + 16 * i) * 4),
                            bt = *reinterpret_cast<const f32x4*>(smem + L_GB + (AT_C + ch0 + 16 * i) * 4);
                const f32x4 w = (nx.x[i] - mean_t) * rstd_t * gm + bt;  // ln_fwd_kernel's expression
                xh[i] = (nx.x[i] - mean_t) * rstd_t;                     // ln_bwd_kernel's
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = (float)(bf16)acc3[i][r];
                gd[i] = d * gm;
                dgam[i] += d * xh[i];
                dbet[i] += d;
                s1 += (gd[i][0] + gd[i][1]) + (gd[i][2] + gd[i][3]);
                const f32x4 gx_ = gd[i] * xh[i];
                s2 += (gx_[0] + gx_[1]) + (gx_[2] + gx_[3]);
                *reinterpret_cast<u32x2*>(smem + L_XW + img_off(tok, ch0 + 16 * i)) =
                    ok ? u32x2{esvit_pack2_bf16(w[0], w[1]), esvit_pack2_bf16(w[2], w[3])} : u32x2{0u, 0u};
            }
            s1 += __shfl_xor(s1, 16, 64);
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 16, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (g == 0) reinterpret_cast<f32x2*>(smem + L_EX)[wave * 16 + c] = f32x2{s1, s2};
        }
        __syncthreads();
        {
            const f32x2* ex = reinterpret_cast<const f32x2*>(smem + L_EX);
            const f32x2 e0 = ex[(wave & ~1) * 16 + c], e1 = ex[(wave | 1) * 16 + c];
            const float m1 = (e0[0] + e1[0]) / AT_C, m2 = (e0[1] + e1[1]) / AT_C;
            const float sc = nx.sc;
            f32x4 o[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                o[i] = (gd[i] - m1 - xh[i] * m2) * rstd_t;
                o[i] += nx.gi[i];
            }
            // ---- L (of the next tile): its dqkv -> the other image, the registers take the tile after's.  This stands BEFORE the stores:
            // g_in above is the youngest request in flight, so everything has landed here, and every later wait of the loop is for loads
            // requested after the stores below -- no counted wait spans a store (stores retire out of order with respect to loads,
            // DESIGN.md 4.1e)
            store_dq(smem + L_DQ + (buf ^ 1) * (AT_T * DQ_ROW), M, tnext, tid, nx);
            request_dq(dqkv, M, tnext2, tid, nx);
            if (ok) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    *reinterpret_cast<f32x4*>(gx + row * AT_C + ch0 + 16 * i) = o[i];
                    if (gxa)
                        *reinterpret_cast<u32x2*>(gxa + row * AT_C + ch0 + 16 * i) =
                            u32x2{esvit_pack2_bf16(o[i][0] * sc, o[i][1] * sc), esvit_pack2_bf16(o[i][2] * sc, o[i][3] * sc)};
                }
            }
        }
        request_rows(x, g_in, mean, rstd, rowscale, rows_per_sample, M, tnext, tok, ch0, nx);

        // ---- C: dWqkv += dqkv^T xw over the tile's 64 tokens
        {
            const char* dq_tr = dq_img + (8 * g + (c >> 2)) * DQ_ROW + 2 * (16 * tb + 4 * (c & 3));
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 bx[3];
#pragma unroll
                for (int n = 0; n < 3; ++n) {
                    const int ch = 16 * (3 * hc + n) + 4 * (c & 3);
                    bx[n] = tr_pair(smem + L_XW + img_off(32 * ks + 8 * g + (c >> 2), ch), smem + L_XW + img_off(32 * ks + 8 * g + (c >> 2) + 4, ch));
                }
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    if (t < nt) {
                        const char* p = dq_tr + 32 * ks * DQ_ROW + 32 * t;
                        const bf16x8 a = tr_pair(p, p + 4 * DQ_ROW);
#pragma unroll
                        for (int n = 0; n < 3; ++n) accW[t][n] = mfma(a, bx[n], accW[t][n]);
                    }
                }
            }
        }
        // (the xw image and the exchanged sums are rewritten behind the next barrier, which every wave reaches only after this phase; the
        // other dqkv image was filled behind this trip's second barrier, when nobody read it any more)
    }

    // ---- partial of this workgroup
    float* pw = part + (long)blockIdx.x * AT_PART;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        if (t < nt) {
#pragma unroll
            for (int n = 0; n < 3; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) pw[(16 * (tb + t) + 4 * g + r) * AT_C + 16 * (3 * hc + n) + c] = accW[t][n][r];
        }
    }
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem + L_DQ);  // [wave][dgamma | dbeta][48], then the column sums [2][288]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a = dgam[i][r], b = dbet[i][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                a += __shfl_xor(a, o, 64);
                b += __shfl_xor(b, o, 64);
            }
            if (c == 0) {
                red[(wave * 2 + 0) * 48 + 16 * i + 4 * g + r] = a;
                red[(wave * 2 + 1) * 48 + 16 * i + 4 * g + r] = b;
            }
        }
    float* red2 = red + 2 * AT_NW * 48;
    if (tid < AT_J) {
        const int half = tid >= 144, cp = tid - 144 * half;
        red2[half * AT_J + 2 * cp] = cs0;
        red2[half * AT_J + 2 * cp + 1] = cs1;
    }
    __syncthreads();
    if (tid < AT_J) pw[AT_OFF_B + tid] = red2[tid] + red2[AT_J + tid];
    if (tid < 2 * AT_C) {  // the four token tiles in order: waves (w & 1) == channel half
        const int which = tid / AT_C, ch = tid - AT_C * which;
        const int half = ch / 48, lc = ch - 48 * half;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += red[((2 * j + half) * 2 + which) * 48 + lc];
        pw[(which ? AT_OFF_DB : AT_OFF_DG) + ch] = s;
    }
}

// sums the workgroup partials in index order into the four outputs
__global__ __launch_bounds__(256) void attn_tail_reduce_kernel(const float* __restrict__ part, int nblk, float* __restrict__ dW, float* __restrict__ db,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= AT_PART) return;
    const float* p = part + i;
    float s = 0.f;
    int b = 0;
    for (; b + 8 <= nblk; b += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(long)(b + k) * AT_PART];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; b < nblk; ++b) s += p[(long)b * AT_PART];
    if (i < AT_OFF_B) dW[i] = s;
    else if (i < AT_OFF_DG) db[i - AT_OFF_B] = s;
    else if (i < AT_OFF_DB) dgamma[i - AT_OFF_DG] = s;
    else dbeta[i - AT_OFF_DB] = s;
}

// the walk of mlp_dw_kernel: one workgroup per CU, at most one per 64-row tile
int tail_grid(long M) { return (int)(esvit_i_mlp_dw_ws(ESVIT_BF16, AT_C, M) / (4L * ESVIT_MLP_DW_PARTIAL_FLOATS)); }

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// esvit_query(ESVIT_Q_ATTN_TAIL_WS, dtype, C, M): bytes of the partials -- one of 28128 floats per workgroup of the launch
int64_t esvit_i_attn_tail_ws(int dtype, int C, int64_t M) {
    if (dtype != ESVIT_BF16 || C != AT_C || M <= 0) return 0;
    return (int64_t)tail_grid((long)M) * AT_PART * 4;
}

// the qkv-tail mode of esvit_layernorm_bwd (norm.hip hands its arguments over as they came)
int esvit_i_attn_tail_bwd(int dtype, const void* dqkv, const float* x, const float* mean, const float* rstd, const float* gamma, const float* g_in,
                          int64_t rows, int C, float* dx, float* dgamma, float* dbeta, float* ws, const esvit_ln_qkv_tail* tail, int tokens, void* dx_act,
                          int act_dtype, const float* rowscale, int rows_per_sample, hipStream_t stream) {
    ESVIT_CHECK_ARG(dtype == ESVIT_BF16 && C == AT_C, "esvit_layernorm_bwd(qkv tail): bf16 and C = 96 only (dtype=%d C=%d)", dtype, C);
    ESVIT_CHECK_ARG(dqkv && x && mean && rstd && gamma && g_in && dx && dgamma && dbeta && ws && tail && rows > 0 && rows < (1L << 31) && tokens == 0,
                    "esvit_layernorm_bwd(qkv tail): null pointer / empty input / tokens != 0");
    ESVIT_CHECK_ARG(tail->Wqkv && tail->beta && tail->dWqkv && tail->dbqkv, "esvit_layernorm_bwd(qkv tail): the record needs Wqkv, beta, dWqkv and dbqkv");
    if (dx_act) ESVIT_CHECK_ARG(act_dtype == ESVIT_BF16, "esvit_layernorm_bwd(qkv tail): dx_act is bf16");
    if (rowscale) ESVIT_CHECK_ARG(dx_act && rows_per_sample > 0, "esvit_layernorm_bwd: rowscale scales dx_act and needs rows_per_sample");
    ESVIT_CHECK_ARG(al16(dqkv) && al16(x) && al16(g_in) && al16(gamma) && al16(tail->beta) && al16(tail->Wqkv) && al16(dx) && al16(dx_act) && al16(ws),
                    "esvit_layernorm_bwd(qkv tail): dqkv, x, g_in, gamma, beta, Wqkv, dx, dx_act and ws are accessed in 16-byte pieces: align them");
    const int grid = tail_grid((long)rows);
    const int ntiles = (int)((rows + AT_T - 1) / AT_T);
    auto k = attn_tail_kernel;
    static unsigned long long lds_set = 0;
    esvit_raise_lds(k, L_END, lds_set);
    hipLaunchKernelGGL(k, dim3(grid), dim3(AT_NT), L_END, stream, (const bf16*)dqkv, x, mean, rstd, g_in, gamma, tail->beta, (const bf16*)tail->Wqkv, rowscale,
                       rows_per_sample > 0 ? rows_per_sample : 1, (long)rows, ntiles, dx, (bf16*)dx_act, ws);
    ESVIT_CHECK_LAUNCH("esvit_layernorm_bwd(qkv tail)");
    hipLaunchKernelGGL(attn_tail_reduce_kernel, dim3((AT_PART + 255) / 256), dim3(256), 0, stream, ws, grid, tail->dWqkv, tail->dbqkv, dgamma, dbeta);
    ESVIT_CHECK_LAUNCH("esvit_layernorm_bwd(qkv tail reduce)");
    return ESVIT_OK;
}
