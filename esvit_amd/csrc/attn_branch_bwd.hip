// Backward of the fused attention branch of a Swin block with the weight gradients accumulated on the chip (bf16, C = 96, nH = 3,
// head_dim 32, 7x7 windows: stage 0 of Swin-T / -S).  The present chain (proj weight- and data-gradient GEMMs, window_attn_bwd, the
// qkv weight- and data-gradient GEMMs, the pad-row column sums, layernorm_bwd) reads LayerNorm(x), qkv and the attention output that
// the forward wrote for it.  Here ONE launch per resolution group reads x and dL/dx1, recomputes the forward per window, and writes
// dL/dx (and, optionally, its scaled bf16 copy); dWqkv, dWproj and the relative-position-bias gradient stay in registers across a
// static loop over windows (workgroup b takes windows b, b + grid, ...: the summation order depends on (windows, grid) only).
// Workgroup b writes partial b and one bias-gradient slab; a second launch sums the partials in index order, and -- when the caller
// gives the table's gradient a place -- two small launches sum the slabs in index order and gather the table's rows.  No atomics.
//
// Work split: 12 waves (3 per SIMD, <= 168 registers), wave (h, j) = (wave / 4, wave % 4) owns head h and the 16 slots 16j .. 16j+15
// of the window, as query tile in the attention and as key tile in dK / dV.  Accumulators per wave, updated in place by the MFMA
// builtin: 12 tiles of weight gradient (j < 3: the 32 rows of part j = q | k | v of head h of dWqkv x 96 columns; j = 3: the 32
// columns of head h of dWproj x 96 rows), 4 tiles of dS^T = the head's bias gradient for its queries, already in the fragment layout
// esvit_relpos_bias_bwd folds, and one register of dgamma / dbeta.
//
// Per window (phases separated by workgroup barriers; MFMA fragment convention: A lane (c, g) = row c, k 8g .. 8g+7; B = column c,
// k 8g .. 8g+7; D element r = row 4g + r, column c; a product is formed in BOTH orientations by exchanging its operands wherever
// both the [token][channel] and the [channel][token] image of its result are needed, so nothing is transposed through memory):
//   L  8 lanes per slot read x and dL/dx1; LayerNorm in registers; h = bf16(LN(x)) and dy = bf16(rowscale * dL/dx1) go to LDS in both
//      layouts (pad and idle slots carry 0)
//   Q  qkv = bf16(h Wqkv^T + b) of head h, slots of tile j (both layouts);  dao = bf16(dy Wproj) likewise
//   A  S^T = scale K q^T + bias + shift mask, softmax over keys in registers (fp32), P rounded to bf16 for P v and P^T dao;
//      ao^T = V^T P^T with P from registers (k-slots permuted, as attn_branch.hip), delta = rowsum(dao o ao), dP^T = V dao^T,
//      dS^T = P o (dP^T - delta) (fp32, accumulated into the bias gradient, then rounded), dQ^T = scale K^T dS^T from registers
//   B  dV = P^T dao, dK = scale dS^T q for key tile j from the [key][query] images of P / dS; dqkv overwrites qkv head by head
//   W  dWqkv += dqkv^T h, dWproj += dy^T ao, dbqkv / dbproj column sums;  dh^T = Wqkv^T dqkv^T, LayerNorm backward, gx = gin + LN'(dh)
// Rounding points kept from the chain: h, qkv, P (normalised), ao, dy, dao, dqkv.  dh stays fp32 (the chain rounded it to bf16); the
// score scale is applied in fp32 after the product instead of to a rounded q.
//
// Departures from the plan of record: twelve waves instead of eight (the (head, tile) split is the natural one for
// three heads); ONE window per iteration; all three weight matrices are read as fragments from L2 (128 KiB of bf16 copies that
// every workgroup reads) instead of LDS; both layouts of every image in LDS, at the price of forming the qkv, dao, dV and dK products
// twice (32 of a wave's 122 MFMAs per window); the table's gradient finished here, without atomics, instead of by esvit_relpos_bias_bwd.
// The images of one window in both layouts take the LDS:
//   HT, DYT [96][72] | H -> DAO -> AOT | DY -> DAOT | QKV -> DQKV [64][296] | QKVT -> DQKVT [288][72] | P^T -> dS^T 3 x [64][72] | row
//   statistics = 163 328 bytes.
#include "common.h"
#include "relpos_fold.h"
#include "../../include/esvit_hip.h"

namespace {

constexpr int BW_C = 96, BW_NH = 3, BW_T = 64, BW_NW = 12, BW_NT = BW_NW * 64;
constexpr int BW_FRAG = 4096;
constexpr int P_WQKV = 0, P_WPROJ = 3 * BW_C * BW_C, P_BQKV = P_WPROJ + BW_C * BW_C, P_BPROJ = P_BQKV + 3 * BW_C, P_GAMMA = P_BPROJ + BW_C,
              P_BETA = P_GAMMA + BW_C, P_FLOATS = P_BETA + BW_C;
static_assert(P_FLOATS == ESVIT_ATTN_BWD_PARTIAL_FLOATS, "partial layout");

// leading dimensions (elements) of the bf16 images
constexpr int LDC = 104;   // [slot][96]
constexpr int LDT = 72;    // [channel][64 slots]
constexpr int LDQ = 296;   // [slot][288]
constexpr int O_HT = 0, O_DYT = O_HT + BW_C * LDT * 2, O_H = O_DYT + BW_C * LDT * 2, O_DY = O_H + BW_C * LDT * 2, O_QKV = O_DY + BW_C * LDT * 2,
              O_QKVT = O_QKV + BW_T * LDQ * 2, O_PT = O_QKVT + 3 * BW_C * LDT * 2, O_ST = O_PT + BW_NH * BW_T * LDT * 2, O_END = O_ST + 4 * BW_T * 4;
static_assert(BW_T * LDC <= BW_C * LDT, "the [slot][96] images share the regions of the [96][slot] ones");
static_assert(O_END <= 160 * 1024, "LDS budget");

struct BwdParams {
    const float* x;
    const float* gin;
    const float* rowscale;
    const float* rowscale_out;
    const float* gamma;
    const float* beta;
    float eps;
    const bf16* Wqkv;    // [3C][C]
    const bf16* WqkvT;   // [C][3C]
    const bf16* WprojT;  // [C][C]: row j = column j of proj.weight
    const float* bqkv;
    const float* bias_frag;
    const int* win2tok;
    const int* region_ids;
    int nW, Bw, N, L;
    float scale;
    float* gx;
    bf16* gx_act;
    float* part;   // this launch's first partial
    float* dbias;  // this launch's first slab
};

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x8 ld44(const bf16* p0, const bf16* p1) {
    const u32x2 lo = *reinterpret_cast<const u32x2*>(p0), hi = *reinterpret_cast<const u32x2*>(p1);
    return __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
}
__device__ __forceinline__ void st4(bf16* p, const f32x4& v) {
    *reinterpret_cast<u32x2*>(p) = u32x2{esvit_pack2_bf16(v[0], v[1]), esvit_pack2_bf16(v[2], v[3])};
}
__device__ __forceinline__ void st4(bf16* p, const bf16x4& v) { *reinterpret_cast<bf16x4*>(p) = v; }
__device__ __forceinline__ bf16x4 rnd4(const f32x4& v) { return bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]}; }
__device__ __forceinline__ bf16x8 cat(const bf16x4& a, const bf16x4& b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
constexpr f32x4 Z4 = {0.f, 0.f, 0.f, 0.f};

__global__ __launch_bounds__(BW_NT, 1) void attn_branch_bwd_kernel(const BwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* const HT = reinterpret_cast<bf16*>(smem + O_HT);      // [96][LDT]  LN(x)^T
    bf16* const DYT = reinterpret_cast<bf16*>(smem + O_DYT);    // [96][LDT]  dy^T
    bf16* const Hn = reinterpret_cast<bf16*>(smem + O_H);       // [64][LDC]  LN(x); then dao [64][LDC]; then ao^T [96][LDT]
    bf16* const DYn = reinterpret_cast<bf16*>(smem + O_DY);     // [64][LDC]  dy; then dao^T [96][LDT]
    bf16* const QKV = reinterpret_cast<bf16*>(smem + O_QKV);    // [64][LDQ]  qkv, overwritten by dqkv
    bf16* const QKVT = reinterpret_cast<bf16*>(smem + O_QKVT);  // [288][LDT] qkv^T, overwritten by dqkv^T
    bf16* const PTa = reinterpret_cast<bf16*>(smem + O_PT);     // [3][64 keys][LDT queries]  P^T, then dS^T
    float* const st_mean = reinterpret_cast<float*>(smem + O_ST);
    float* const st_rstd = st_mean + BW_T;
    int* const st_row = reinterpret_cast<int*>(st_rstd + BW_T);
    int* const st_reg = st_row + BW_T;
    bf16* const DAO = Hn;
    bf16* const AOT = Hn;
    bf16* const DAOT = DYn;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = wave >> 2, j = wave & 3;
    const bool masked = p.region_ids != nullptr;
    bf16* const PT = PTa + h * BW_T * LDT;

    f32x4 accw[2][6];  // j < 3: dWqkv rows part j, head h (tile a) x columns 16 b;  j == 3: dWproj^T rows 32h + 16a (columns of dWproj) x 16 b
    f32x4 accb[4];     // dS^T tiles: keys 16 i + 4g + r, query 16 j + c
    float acc_gb = 0.f;  // lane (c, g): c < 8 dgamma, c >= 8 dbeta of channel 32h + 16 ((c >> 2) & 1) + 4g + (c & 3) over this wave's slots
    float s_bqkv = 0.f, s_bproj = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) accw[a][b] = Z4;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) accb[i] = Z4;

    for (int bw = blockIdx.x; bw < p.Bw; bw += gridDim.x) {
        const int img = bw / p.nW, wi = bw - img * p.nW;
        // (opaque per window: hoisted out of the loop, the lane-dependent addresses of all phases would be held -- and spilled -- across it)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int c = lane_t & 15, g = lane_t >> 4;
        const int tid = wave * 64 + lane_t;
        // ---- L: rows in, LayerNorm, images of h and dy in both layouts
        if (tid < 512) {
            const int slot = tid >> 3, sub = tid & 7;
            int tok = -1;
            if (slot < p.N) tok = p.win2tok[(long)wi * p.N + slot];
            const bool live = tok >= 0;
            const long row = live ? (long)img * p.L + tok : 0;
            const float* xr = p.x + row * BW_C + 12 * sub;
            const float* gr = p.gin + row * BW_C + 12 * sub;
            f32x4 xv[3], gv[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                xv[q] = *reinterpret_cast<const f32x4*>(xr + 4 * q);
                gv[q] = *reinterpret_cast<const f32x4*>(gr + 4 * q);
            }
            float s1 = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) s1 += (xv[q][0] + xv[q][1]) + (xv[q][2] + xv[q][3]);
            s1 += __shfl_xor(s1, 1, 64);
            s1 += __shfl_xor(s1, 2, 64);
            s1 += __shfl_xor(s1, 4, 64);
            const float mean = s1 * (1.f / BW_C);
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
            const float rstd = rsqrtf(s2 * (1.f / BW_C) + p.eps);
            const float lv = live ? 1.f : 0.f;
            const float sm = live ? (p.rowscale ? p.rowscale[row] : 1.f) : 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int ch = 12 * sub + 4 * q;
                const f32x4 gm = *reinterpret_cast<const f32x4*>(p.gamma + ch), bt = *reinterpret_cast<const f32x4*>(p.beta + ch);
                f32x4 hv, dv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    hv[e] = lv * ((xv[q][e] - mean) * rstd * gm[e] + bt[e]);
                    dv[e] = sm * gv[q][e];
                }
                const bf16x4 hb = rnd4(hv), db = rnd4(dv);
                st4(Hn + slot * LDC + ch, hb);
                st4(DYn + slot * LDC + ch, db);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    HT[(ch + e) * LDT + slot] = hb[e];
                    DYT[(ch + e) * LDT + slot] = db[e];
                }
            }
            if (sub == 0) {
                st_mean[slot] = mean;
                st_rstd[slot] = rstd;
                st_row[slot] = live ? (int)row : -1;  // (rows of one call are below 2^31 / C: checked by the host)
                st_reg[slot] = (masked && slot < p.N) ? p.region_ids[(long)wi * p.N + slot] : -1;
            }
        }
        __syncthreads();

        // ---- Q: qkv of head h for the slots of tile j, both layouts; dao likewise (kept in registers until H and DY are no longer read)
        f32x4 dao_n[2], dao_t[2];
        {
            bf16x8 hf[3];
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) hf[ks] = ld8(Hn + (16 * j + c) * LDC + 32 * ks + 8 * g);
#pragma unroll 1
            for (int pt = 0; pt < 6; ++pt) {  // part pt / 2 (q | k | v), 16-channel tile pt % 2
                const int ch0 = (pt >> 1) * BW_C + 32 * h + 16 * (pt & 1);
                f32x4 an = Z4, at = Z4;
#pragma unroll
                for (int ks = 0; ks < 3; ++ks) {
                    const bf16x8 wf = ld8(p.Wqkv + (ch0 + c) * BW_C + 32 * ks + 8 * g);
                    an = mfma(wf, hf[ks], an);  // rows: channels, columns: slots
                    at = mfma(hf[ks], wf, at);  // rows: slots, columns: channels
                }
                const f32x4 bn = *reinterpret_cast<const f32x4*>(p.bqkv + ch0 + 4 * g);
                const float bt = p.bqkv[ch0 + c];
                st4(QKV + (16 * j + c) * LDQ + ch0 + 4 * g, an + bn);
                st4(QKVT + (ch0 + c) * LDT + 16 * j + 4 * g, at + bt);
            }
            bf16x8 df[3];
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) df[ks] = ld8(DYn + (16 * j + c) * LDC + 32 * ks + 8 * g);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                dao_n[t] = Z4;
                dao_t[t] = Z4;
#pragma unroll
                for (int ks = 0; ks < 3; ++ks) {
                    const bf16x8 wf = ld8(p.WprojT + (32 * h + 16 * t + c) * BW_C + 32 * ks + 8 * g);
                    dao_n[t] = mfma(wf, df[ks], dao_n[t]);
                    dao_t[t] = mfma(df[ks], wf, dao_t[t]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            st4(DAO + (16 * j + c) * LDC + 32 * h + 16 * t + 4 * g, dao_n[t]);
            st4(DAOT + (32 * h + 16 * t + c) * LDT + 16 * j + 4 * g, dao_t[t]);
        }
        __syncthreads();

        // ---- A: attention of (head h, queries 16j .. 16j+15), recomputed, and its backward up to dS and dQ
        bf16x4 dsb[4];  // bf16(dS^T) tiles
        bf16x4 aob[2];  // ao^T: channels 32h + 16 dt + 4g + r, query 16j + c
        bf16x4 dqb[2];  // dQ^T likewise
        {
            const bf16x8 qf = ld8(QKV + (16 * j + c) * LDQ + 32 * h + 8 * g);
            const bf16x8 dof = ld8(DAO + (16 * j + c) * LDC + 32 * h + 8 * g);
            const int rq = st_reg[16 * j + c];
            f32x4 pr[4];
            float m = -3.0e38f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16x8 kf = ld8(QKV + (16 * i + c) * LDQ + BW_C + 32 * h + 8 * g);
                const f32x4 bf = *reinterpret_cast<const f32x4*>(p.bias_frag + h * BW_FRAG + ((i * 4 + j) * 64 + lane_t) * 4);
                const f32x4 s = mfma(kf, qf, Z4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = s[r] * p.scale + bf[r];
                    if (masked && st_reg[16 * i + 4 * g + r] != rq) v += -100.f;
                    pr[i][r] = v;
                    m = fmaxf(m, v);
                }
            }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __expf(pr[i][r] - m);
                    pr[i][r] = e;
                    sum += e;
                }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.f / sum;
            bf16x4 pb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pr[i] = pr[i] * inv;
                pb[i] = rnd4(pr[i]);
#pragma unroll
                for (int r = 0; r < 4; ++r) PT[(16 * i + 4 * g + r) * LDT + 16 * j + c] = pb[i][r];
            }
            // ao^T = V^T P^T: k-slot 8g + e of k-step ks <-> key 32 ks + 4g + e (e < 4) / 32 ks + 16 + 4g + e - 4, the order the registers hold P in
            float dl = 0.f;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                f32x4 o = Z4;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16* vr = QKVT + (2 * BW_C + 32 * h + 16 * dt + c) * LDT + 32 * ks + 4 * g;
                    o = mfma(ld44(vr, vr + 16), cat(pb[2 * ks], pb[2 * ks + 1]), o);
                }
                aob[dt] = rnd4(o);
                const bf16x4 dv = *reinterpret_cast<const bf16x4*>(DAO + (16 * j + c) * LDC + 32 * h + 16 * dt + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) dl += (float)dv[r] * (float)aob[dt][r];
            }
            dl += __shfl_xor(dl, 16, 64);
            dl += __shfl_xor(dl, 32, 64);
            // dP^T = V dao^T, dS^T = P o (dP^T - delta)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16x8 vf = ld8(QKV + (16 * i + c) * LDQ + 2 * BW_C + 32 * h + 8 * g);
                const f32x4 dp = mfma(vf, dof, Z4);
                f32x4 ds;
#pragma unroll
                for (int r = 0; r < 4; ++r) ds[r] = pr[i][r] * (dp[r] - dl);
                accb[i] += ds;
                dsb[i] = rnd4(ds);
            }
            // dQ^T = scale K^T dS^T, dS from registers as P above
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                f32x4 o = Z4;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16* kr = QKVT + (BW_C + 32 * h + 16 * dt + c) * LDT + 32 * ks + 4 * g;
                    o = mfma(ld44(kr, kr + 16), cat(dsb[2 * ks], dsb[2 * ks + 1]), o);
                }
                dqb[dt] = rnd4(o * p.scale);
            }
        }
        __syncthreads();  // P^T complete; dao (natural layout) no longer read

        // ---- B: ao^T out; dV of key tile j (both layouts) over the V images, which nobody reads any more
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) AOT[(32 * h + 16 * dt + 4 * g + r) * LDT + 16 * j + c] = aob[dt][r];
        {
            bf16x8 pf[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) pf[ks] = ld8(PT + (16 * j + c) * LDT + 32 * ks + 8 * g);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                f32x4 vn = Z4, vt = Z4;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 df = ld8(DAOT + (32 * h + 16 * dt + c) * LDT + 32 * ks + 8 * g);
                    vn = mfma(df, pf[ks], vn);  // rows: channels, columns: keys
                    vt = mfma(pf[ks], df, vt);  // rows: keys, columns: channels
                }
                st4(QKV + (16 * j + c) * LDQ + 2 * BW_C + 32 * h + 16 * dt + 4 * g, vn);
                st4(QKVT + (2 * BW_C + 32 * h + 16 * dt + c) * LDT + 16 * j + 4 * g, vt);
            }
        }
        __syncthreads();  // P^T read
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) PT[(16 * i + 4 * g + r) * LDT + 16 * j + c] = dsb[i][r];
        __syncthreads();  // dS^T complete
        {
            bf16x8 sf[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) sf[ks] = ld8(PT + (16 * j + c) * LDT + 32 * ks + 8 * g);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                f32x4 kn = Z4, kt = Z4;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 qt = ld8(QKVT + (32 * h + 16 * dt + c) * LDT + 32 * ks + 8 * g);
                    kn = mfma(qt, sf[ks], kn);
                    kt = mfma(sf[ks], qt, kt);
                }
                // (the K images were last read in phase A)
                st4(QKV + (16 * j + c) * LDQ + BW_C + 32 * h + 16 * dt + 4 * g, kn * p.scale);
                st4(QKVT + (BW_C + 32 * h + 16 * dt + c) * LDT + 16 * j + 4 * g, kt * p.scale);
                // (q rows of the own queries: only this wave read them)
                st4(QKV + (16 * j + c) * LDQ + 32 * h + 16 * dt + 4 * g, dqb[dt]);
            }
        }
        __syncthreads();  // q^T read
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) QKVT[(32 * h + 16 * dt + 4 * g + r) * LDT + 16 * j + c] = dqb[dt][r];
        __syncthreads();  // dqkv complete in both layouts

        // ---- W: the token-contracting products
        {
            const bf16* Ab = j < 3 ? QKVT + (j * BW_C + 32 * h) * LDT : AOT + 32 * h * LDT;
            const bf16* Bb = j < 3 ? HT : DYT;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 af[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) af[a] = ld8(Ab + (16 * a + c) * LDT + 32 * ks + 8 * g);
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    const bf16x8 bf = ld8(Bb + (16 * b + c) * LDT + 32 * ks + 8 * g);
#pragma unroll
                    for (int a = 0; a < 2; ++a) accw[a][b] = mfma(af[a], bf, accw[a][b]);
                }
            }
        }
        // column sums of the rounded dqkv (all slots: pad slots carry dK / dV rows) and of the rounded dy
        if (tid < 576) {
            const int ch = tid % 288, half = tid / 288;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bf16x8 v = ld8(QKVT + ch * LDT + 32 * half + 8 * k);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += (float)v[e];
            }
            s_bqkv += s;
        } else {
            const int ch = (tid - 576) % BW_C, half = (tid - 576) / BW_C;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bf16x8 v = ld8(DYT + ch * LDT + 32 * half + 8 * k);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += (float)v[e];
            }
            s_bproj += s;
        }
        // dh^T for the slots of tile j, channels 32h .. 32h + 31; LayerNorm backward; the three waves of a slot tile exchange their row sums
        {
            f32x4 dh[2] = {Z4, Z4};
#pragma unroll 3
            for (int ks = 0; ks < 9; ++ks) {
                const bf16x8 b = ld8(QKV + (16 * j + c) * LDQ + 32 * ks + 8 * g);
#pragma unroll
                for (int t = 0; t < 2; ++t) dh[t] = mfma(ld8(p.WqkvT + (32 * h + 16 * t + c) * (3 * BW_C) + 32 * ks + 8 * g), b, dh[t]);
            }
            const int slot = 16 * j + c;
            const int row = st_row[slot];
            const bool live = row >= 0;
            const long rr = live ? row : 0;
            const float mean = st_mean[slot], rstd = st_rstd[slot];
            float xh[2][4], gd[2][4];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int c0 = 32 * h + 16 * t + 4 * g;
                const f32x4 xv = *reinterpret_cast<const f32x4*>(p.x + rr * BW_C + c0);
                const f32x4 gm = *reinterpret_cast<const f32x4*>(p.gamma + c0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    xh[t][r] = (xv[r] - mean) * rstd;
                    gd[t][r] = dh[t][r] * gm[r];
                    s1 += gd[t][r];
                    s2 += gd[t][r] * xh[t][r];
                    // (the sums over the tile's 16 slots land in one register: lane c keeps value c of the sixteen)
                    const float dg = row16_sum(live ? dh[t][r] * xh[t][r] : 0.f), db = row16_sum(live ? dh[t][r] : 0.f);
                    if (c == 4 * t + r) acc_gb += dg;
                    if (c == 8 + 4 * t + r) acc_gb += db;
                }
            }
            s1 += __shfl_xor(s1, 16, 64);
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 16, 64);
            s2 += __shfl_xor(s2, 32, 64);
            f32x2* ex = reinterpret_cast<f32x2*>(PTa);  // (P^T / dS^T are no longer read)
            if (g == 0) ex[wave * 16 + c] = f32x2{s1, s2};
            __syncthreads();
            const f32x2 e0 = ex[j * 16 + c], e1 = ex[(4 + j) * 16 + c], e2 = ex[(8 + j) * 16 + c];
            const float m1 = ((e0[0] + e1[0]) + e2[0]) * (1.f / BW_C), m2 = ((e0[1] + e1[1]) + e2[1]) * (1.f / BW_C);
            if (live) {
                const float ro = p.rowscale_out ? p.rowscale_out[rr] : 1.f;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int c0 = 32 * h + 16 * t + 4 * g;
                    const f32x4 gv = *reinterpret_cast<const f32x4*>(p.gin + rr * BW_C + c0);
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = gv[r] + rstd * (gd[t][r] - m1 - xh[t][r] * m2);
                    *reinterpret_cast<f32x4*>(p.gx + rr * BW_C + c0) = o;
                    if (p.gx_act) st4(p.gx_act + rr * BW_C + c0, o * ro);
                }
            }
        }
        __syncthreads();  // every image may be overwritten
    }

    // ---- this workgroup's partial and bias-gradient slab
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int c = lane_e & 15, g = lane_e >> 4;
    const int tid = wave * 64 + lane_e;
    float* pw = p.part + (long)blockIdx.x * P_FLOATS;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ra = 32 * h + 16 * a + 4 * g + r, cb = 16 * b + c;
                if (j < 3) pw[P_WQKV + (j * BW_C + ra) * BW_C + cb] = accw[a][b][r];
                else pw[P_WPROJ + cb * BW_C + ra] = accw[a][b][r];
            }
    float* ds = p.dbias + ((long)blockIdx.x * BW_NH + h) * BW_FRAG;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(ds + ((i * 4 + j) * 64 + lane_e) * 4) = accb[i];
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [768] column sums | [12 waves][64 lanes] dgamma / dbeta
    red[tid] = tid < 576 ? s_bqkv : s_bproj;
    red[BW_NT + tid] = acc_gb;
    __syncthreads();
    if (tid < 288) pw[P_BQKV + tid] = red[tid] + red[288 + tid];
    else if (tid < 384) pw[P_BPROJ + tid - 288] = red[576 + tid - 288] + red[576 + BW_C + tid - 288];
    else if (tid < 576) {  // channel ch of dgamma (kind 0) / dbeta (kind 1): slot tiles j = 0..3 in order
        const int ch = (tid - 384) % BW_C, kind = (tid - 384) / BW_C;
        const int hh = ch >> 5, t = (ch >> 4) & 1, gg = (ch >> 2) & 3, r = ch & 3;
        float s = 0.f;
        for (int jj = 0; jj < 4; ++jj) s += red[BW_NT + (4 * hh + jj) * 64 + 16 * gg + 8 * kind + 4 * t + r];
        pw[(kind ? P_BETA : P_GAMMA) + ch] = s;
    }
}

// sums partials [0, nblk) in index order into the six outputs
__global__ __launch_bounds__(256) void attn_branch_bwd_reduce_kernel(const float* __restrict__ part, int nblk, float* __restrict__ dWqkv,
                                                                     float* __restrict__ dWproj, float* __restrict__ dbqkv, float* __restrict__ dbproj,
                                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P_FLOATS) return;
    const float* p = part + i;
    float s = 0.f;
    int b = 0;
    for (; b + 8 <= nblk; b += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(long)(b + k) * P_FLOATS];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; b < nblk; ++b) s += p[(long)b * P_FLOATS];
    if (i < P_WPROJ) dWqkv[i] = s;
    else if (i < P_BQKV) dWproj[i - P_WPROJ] = s;
    else if (i < P_BPROJ) dbqkv[i - P_BQKV] = s;
    else if (i < P_GAMMA) dbproj[i - P_BPROJ] = s;
    else if (i < P_BETA) dgamma[i - P_GAMMA] = s;
    else dbeta[i - P_BETA] = s;
}

// The table's gradient without atomics (esvit_relpos_bias_bwd scatters with atomicAdd unless it is asked for ESVIT_RELPOS_ORDERED: the
// same slabs give sums that differ in the last bits from launch to launch): the fold and the gather of relpos_fold.h.

int bwd_grid(long windows) {
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
    return (int)(windows < n ? windows : n);
}

}  // namespace

// esvit_query(ESVIT_Q_ATTN_BWD_FUSED_GRID, dtype, C, windows): workgroups (= partials, = bias-gradient slabs) of one backward launch; 0: no such mode
int64_t esvit_i_attn_branch_bwd_grid(int dtype, int C, int64_t windows) {
    if (dtype != ESVIT_BF16 || C != BW_C || windows <= 0 || windows >= (1L << 22)) return 0;
    return bwd_grid((long)windows);
}

// backward mode of esvit_attn_branch_fwd (attn_branch.hip checks the arguments that both modes share)
int esvit_i_attn_branch_bwd(const float* x, const float* gamma, const float* beta, float eps, const void* Wqkv, const float* bqkv, const void* WprojT,
                            const int32_t* win2tok, int L, const float* bias_frag, const int32_t* region_ids, int nW, int nB, int N, int nH, float scale,
                            const float* rowscale, const esvit_attn_bwd_desc* d, hipStream_t stream) {
    ESVIT_CHECK_ARG(nH == BW_NH && N == 49, "esvit_attn_branch_fwd(backward): C = 96, three heads of 32 channels, 7x7 windows only (nH=%d N=%d)", nH, N);
    ESVIT_CHECK_ARG(d->gin && d->gx && d->WqkvT && d->dWqkv && d->dbqkv && d->dWproj && d->dbproj && d->dgamma && d->dbeta && d->dbias_ws && d->partials_ws,
                    "esvit_attn_branch_fwd(backward): gin, gx, WqkvT, the six gradient outputs and the two workspaces are required");
    ESVIT_CHECK_ARG((((uintptr_t)d->gin | (uintptr_t)d->gx | (uintptr_t)d->gx_act | (uintptr_t)d->WqkvT | (uintptr_t)d->dbias_ws | (uintptr_t)d->partials_ws) & 15) == 0,
                    "esvit_attn_branch_fwd(backward): gin, gx, gx_act, WqkvT and the workspaces are accessed in 16-byte pieces: align them");
    const int grid = bwd_grid((long)nB * nW);
    ESVIT_CHECK_ARG(!d->dtable || (d->index && d->table_rows > 0), "esvit_attn_branch_fwd(backward): dtable comes with index and table_rows");
    ESVIT_CHECK_ARG(d->first_partial >= 0 && d->finish >= 0 && (d->finish == 0 || d->finish >= d->first_partial + grid),
                    "esvit_attn_branch_fwd(backward): finish = %d leaves out partials of this call (first %d, %d workgroups)", d->finish, d->first_partial, grid);
    BwdParams prm;
    prm.x = x; prm.gin = d->gin; prm.rowscale = rowscale; prm.rowscale_out = d->rowscale_out; prm.gamma = gamma; prm.beta = beta; prm.eps = eps;
    prm.Wqkv = (const bf16*)Wqkv; prm.WqkvT = (const bf16*)d->WqkvT; prm.WprojT = (const bf16*)WprojT; prm.bqkv = bqkv; prm.bias_frag = bias_frag;
    prm.win2tok = win2tok; prm.region_ids = region_ids; prm.nW = nW; prm.Bw = nB * nW; prm.N = N; prm.L = L; prm.scale = scale;
    prm.gx = d->gx; prm.gx_act = (bf16*)d->gx_act;
    prm.part = d->partials_ws + (long)d->first_partial * P_FLOATS;
    prm.dbias = d->dbias_ws + (long)d->first_partial * BW_NH * BW_FRAG;
    auto k = attn_branch_bwd_kernel;
    static unsigned long long lds_set = 0;
    esvit_raise_lds(k, O_END, lds_set);
    hipLaunchKernelGGL(k, dim3(grid), dim3(BW_NT), O_END, stream, prm);
    ESVIT_CHECK_LAUNCH("esvit_attn_branch_fwd(backward)");
    if (d->finish > 0) {
        hipLaunchKernelGGL(attn_branch_bwd_reduce_kernel, dim3((P_FLOATS + 255) / 256), dim3(256), 0, stream, d->partials_ws, d->finish, d->dWqkv, d->dWproj,
                           d->dbqkv, d->dbproj, d->dgamma, d->dbeta);
        ESVIT_CHECK_LAUNCH("esvit_attn_branch_fwd(backward reduce)");
        if (d->dtable) {
            relpos_ordered_launch(d->dbias_ws, d->finish, 4, d->index, N, BW_NH, d->table_rows, d->dtable, 0, stream);
            ESVIT_CHECK_LAUNCH("esvit_attn_branch_fwd(backward table)");
        }
    }
    return ESVIT_OK;
}
