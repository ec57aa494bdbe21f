// Fused sliding-chunk attention of Vision Longformer (layers/slidingchunk_2d.py mode 0, exact 0; layers/longformer2d.py), bf16, gfx950:
// the sliding-chunk mode of esvit_window_attn_fwd / esvit_window_attn_bwd (ws | ESVIT_ATTN_SLIDING_CHUNK, include/esvit_hip.h).
// Token-ordered I/O (qkv [B L, 3C], columns [3][nH][hd], tokens [globals | (x, y) row-major]; out [B L, C]), the scores stay on the
// chip, nothing grows with L^2.  The predicate is oracle/ops_ref.chunk_mask; the slot -> token maps are chunk_geom.h.
//
//   local queries   chunk_fwd_local: one workgroup per (image, head, chunk), four waves, one 16-slot query tile each (49 live of 64
//                   slots).  K and V of the neighbourhood [globals | 21 x 21 square, clipped] are staged once by slot (448 slots,
//                   dead slots are zero rows whose scores are set to -1e30); a wave forms S^T = scale K Q^T for its tile (28 MFMA
//                   tiles in registers), the softmax in registers, P V with the transpose read of V (mfma.h: frag_v_perm), as window_attn_big.hip's
//                   attn_big_fwd3 does for 224 slots.  The per-query log-sum-exp is saved.
//   global queries  nglo rows against all L keys: chunk_fwd_global_part walks 512-key ranges on the VALU (nglo L hd products: a
//                   thousandth of the local work), one (max, sum, P V) partial per range; chunk_fwd_global_combine merges the
//                   partials in range order.  Linear in L.
//   backward        delta = rowsum(dO o O) once (chunk_delta); then
//                   chunk_bwd_dq_local   dQ of a chunk's queries from its key neighbourhood, P rebuilt from the saved log-sum-exp
//                   chunk_bwd_dkv_local  dK, dV of a chunk's keys from [global queries | the queries of its neighbourhood]: the
//                                        same geometry with the roles exchanged (the neighbourhood relation is symmetric)
//                   chunk_bwd_global_part / _combine  dK, dV of the global keys from all L queries and dQ of the global queries
//                                        from all L keys, per 512-token range on the VALU, summed in range order.
//                   Every output row is written by exactly one workgroup: no atomics, bit-reproducible launch to launch.
//   statistics      ws | ESVIT_ATTN_SLIDING_CHUNK | ESVIT_ATTN_CHUNK_STATS: the entropy of every softmax row (chunk_stats_local: the local
//                   forward up to its probabilities, K only; chunk_stats_global_part / _combine: the range-split global rows without
//                   the V loop) and the probability rows of a few listed queries over all L tokens (chunk_stats_rows, VALU).
//
// Q, K, V and dO enter the MFMAs as the bf16 values they are and the scale multiplies the fp32 scores: scaling Q in LDS, as
// window_attn_big.hip does, rounds scale * q to bf16 again (2^-9 relative for head dims 32 and 48, whose scale is no power of two),
// which measured 3x the dense route's gradient-norm error on vil_small's first stage.  P and dS are rounded to bf16 for their MFMAs.
//
// Head dims 32, 48 and 64.  48 (vil_tiny stage 1) is not a multiple of the 32-deep bf16 MFMA k-step: its LDS images are padded to
// 64 columns with zeros (the products add zeros; the store drops channels >= 48).  Chunk side w = 7 only, nglo <= 7.
//
// LDS (bf16 rows padded by 8 elements, as window_attn_big.hip): two [448][hdp + 8] images + four per-wave [16][hdp + 8] tiles
// (forward: one per wave, backward: two) + tables: 77 KB (hd 32) / 137 KB (hd 48, 64) forward, 82-86 / 146-150 KB backward:
// two workgroups per CU at head_dim 32, one otherwise.  148-216 VGPRs, no scratch (tools/kernel_regs.sh chunk_attn).
#include "common.h"
#include "chunk_geom.h"
#include "mfma.h"
#include "../../include/esvit_hip.h"

namespace {

constexpr int NBS = CG_NB_SLOTS;    // 448
constexpr int NBT = NBS / 16;       // 28 score tiles per 16 own slots
constexpr int OWS = CG_OWN_SLOTS;   // 64
constexpr int WAVES = OWS / 16;     // 4
constexpr int NTHR = WAVES * 64;
constexpr int GSPLIT = 512;         // tokens per range of the global-token kernels
constexpr int GMAX = 8;             // rows reserved per range for the global tokens (nglo <= 7)
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int HD>
struct CCfg {
    static constexpr int HDP = HD <= 32 ? 32 : 64;  // columns of the LDS images (zero past HD)
    static constexpr int LDQ = HDP + 8;
    static constexpr int VPR = HD / 8;    // 16-byte pieces of a row in memory
    static constexpr int VPRP = HDP / 8;  // and in LDS
    static constexpr int KS = HDP / 32, DT = HDP / 16;
    static constexpr int FULL = NBS * LDQ, TILE = 16 * LDQ;
};

struct Unit {
    int z, b, h, cr, cc;
};
__device__ __forceinline__ Unit unit_of(int u, const ChunkGeom& gm, int nH) {
    const int nch = cg_chunks(gm);
    Unit x;
    x.z = u / nch;
    const int ch = u % nch;
    x.b = x.z / nH;
    x.h = x.z % nH;
    x.cr = ch / gm.ncy;
    x.cc = ch % gm.ncy;
    return x;
}

__device__ __forceinline__ void fill_tables(int* nbtok, int* owntok, const ChunkGeom& gm, int cr, int cc) {
    for (int s = threadIdx.x; s < NBS; s += NTHR) nbtok[s] = cg_nb_token(gm, cr, cc, s);
    for (int s = threadIdx.x; s < OWS; s += NTHR) owntok[s] = cg_own_token(gm, cr, cc, s);
}

// stage NROWS slots (tokens tok[0 .. NROWS)) of a token-ordered bf16 matrix into a [NROWS][LDQ] image, zero for dead slots and
// for the columns past HD; NT threads cooperate.  Every global load of the thread is issued before its first LDS store.
template <int NROWS, int NT, int HD>
struct RowStage {
    using Cfg = CCfg<HD>;
    static constexpr int ITERS = (NROWS * Cfg::VPRP + NT - 1) / NT;
    bf16x8 x[ITERS];
    __device__ __forceinline__ void load(const bf16* __restrict__ g, long row_stride, const int* tok, long tok_base, int tid) {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int v = tid + it * NT;
            const int rl = v / Cfg::VPRP, dv = v % Cfg::VPRP;
            bf16x8 y = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
            if (v < NROWS * Cfg::VPRP && dv < Cfg::VPR) {
                const int t = tok[rl];
                if (t >= 0) y = *reinterpret_cast<const bf16x8*>(g + (tok_base + t) * row_stride + dv * 8);
            }
            x[it] = y;
        }
    }
    __device__ __forceinline__ void store(bf16* lds, int tid) {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int v = tid + it * NT;
            if (v >= NROWS * Cfg::VPRP) continue;
            *reinterpret_cast<bf16x8*>(lds + (v / Cfg::VPRP) * Cfg::LDQ + (v % Cfg::VPRP) * 8) = x[it];
        }
    }
};

// does this wave's tile of own slots hold a live token at all (wave-uniform)
__device__ __forceinline__ bool tile_live(const int* owntok, int wave, int lane) {
    return __ballot(lane < 16 && owntok[16 * wave + lane] >= 0) != 0ull;
}

// -------------------------------------------------------------------------------------------------------------
// forward, local queries
// -------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_fwd_local_kernel(const bf16* __restrict__ qkv, ChunkGeom gm, int L, int nH, float scale,
                                                               bf16* __restrict__ out, float* __restrict__ lse_out) {
    using Cfg = CCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, DT = Cfg::DT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int* nbtok = reinterpret_cast<int*>(smem_raw);
    int* owntok = nbtok + NBS;
    bf16* Ks = reinterpret_cast<bf16*>(owntok + OWS);
    bf16* Vs = Ks + Cfg::FULL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    bf16* Qs = Vs + Cfg::FULL + wave * Cfg::TILE;

    const Unit u = unit_of(blockIdx.x, gm, nH);
    const int C = nH * HD;
    const long tok_base = (long)u.b * L;
    const bf16* src = qkv + u.h * HD;

    fill_tables(nbtok, owntok, gm, u.cr, u.cc);
    __syncthreads();
    {
        RowStage<NBS, NTHR, HD> sk, sv;
        RowStage<16, 64, HD> sq;
        sk.load(src + C, 3L * C, nbtok, tok_base, threadIdx.x);
        sv.load(src + 2 * C, 3L * C, nbtok, tok_base, threadIdx.x);
        sq.load(src, 3L * C, owntok + 16 * wave, tok_base, lane);
        sk.store(Ks, threadIdx.x);
        sv.store(Vs, threadIdx.x);
        sq.store(Qs, lane);
    }
    __syncthreads();  // K, V complete; everything below is private to the wave
    if (!tile_live(owntok, wave, lane)) return;

    Frag<bf16> qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = frag_kc<bf16>(Qs, LDQ, 0, 32 * ks, c, g);
    // S^T tiles: p[i][r] = score of key slot 16 i + 4g + r and query slot 16 wave + c
    f32x4 p[NBT];
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) mma(frag_kc<bf16>(Ks, LDQ, 16 * i, 32 * ks, c, g), qf[ks], s);
        const i32x4 tk = *reinterpret_cast<const i32x4*>(nbtok + 16 * i + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = tk[r] >= 0 ? s[r] * scale : -1.0e30f;
            m = fmaxf(m, s[r]);
        }
        p[i] = s;
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NBT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(p[i][r] - m);
            p[i][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    const int tok = owntok[16 * wave + c];
    if (g == 0 && tok >= 0) lse_out[(long)u.z * L + tok] = m + __logf(sum);
    f32x4 o[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NBS / 32; ++ks) {
        const Frag<bf16> pf = frag_p_regs<bf16>(p[2 * ks] * inv, p[2 * ks + 1] * inv);
#pragma unroll
        for (int j = 0; j < DT; ++j) mma(frag_v_perm<bf16>(Vs, LDQ, 16 * j, ks, c, g), pf, o[j]);  // O^T [channel][query]: operands exchanged
    }
    store_tile_rows<HD, Cfg::HDP>(o, 1.f, out + tok_base * C, L, C, u.h * HD, tok, g);
}

// -------------------------------------------------------------------------------------------------------------
// backward, dQ of the local queries
// -------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_bwd_dq_local_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                                  const float* __restrict__ lse_in, const float* __restrict__ delta_in,
                                                                  ChunkGeom gm, int L, int nH, float scale, bf16* __restrict__ dqkv) {
    using Cfg = CCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, DT = Cfg::DT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int* nbtok = reinterpret_cast<int*>(smem_raw);
    int* owntok = nbtok + NBS;
    bf16* Ks = reinterpret_cast<bf16*>(owntok + OWS);
    bf16* Vs = Ks + Cfg::FULL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    bf16* Qs = Vs + Cfg::FULL + wave * (2 * Cfg::TILE);
    bf16* Os = Qs + Cfg::TILE;  // dO rows of this wave's queries

    const Unit u = unit_of(blockIdx.x, gm, nH);
    const int C = nH * HD;
    const long tok_base = (long)u.b * L;
    const bf16* src = qkv + u.h * HD;

    fill_tables(nbtok, owntok, gm, u.cr, u.cc);
    __syncthreads();
    {
        RowStage<NBS, NTHR, HD> sk, sv;
        RowStage<16, 64, HD> sq, so;
        sk.load(src + C, 3L * C, nbtok, tok_base, threadIdx.x);
        sv.load(src + 2 * C, 3L * C, nbtok, tok_base, threadIdx.x);
        sq.load(src, 3L * C, owntok + 16 * wave, tok_base, lane);
        so.load(dout + u.h * HD, (long)C, owntok + 16 * wave, tok_base, lane);
        sk.store(Ks, threadIdx.x);
        sv.store(Vs, threadIdx.x);
        sq.store(Qs, lane);
        so.store(Os, lane);
    }
    __syncthreads();
    if (!tile_live(owntok, wave, lane)) return;

    const int tok = owntok[16 * wave + c];
    // a dead query slot rebuilds P = exp(s - 3e38) = 0 (its row is not stored)
    const float lq = tok >= 0 ? lse_in[(long)u.z * L + tok] : 3.0e38f;
    const float dl = tok >= 0 ? delta_in[(long)u.z * L + tok] : 0.f;
    Frag<bf16> qf[KS], of[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = frag_kc<bf16>(Qs, LDQ, 0, 32 * ks, c, g);
        of[ks] = frag_kc<bf16>(Os, LDQ, 0, 32 * ks, c, g);
    }
    // P^T tiles (rows = key slots) from the saved log-sum-exp
    f32x4 pj[NBT];
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) mma(frag_kc<bf16>(Ks, LDQ, 16 * i, 32 * ks, c, g), qf[ks], s);
        const i32x4 tk = *reinterpret_cast<const i32x4*>(nbtok + 16 * i + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = tk[r] >= 0 ? __expf(s[r] * scale - lq) : 0.f;
        pj[i] = s;
    }
    // dP^T = V dO^T, dS = P o (dP - delta), dQ = scale dS K
    f32x4 acc[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NBS / 32; ++ks) {
        f32x4 ds2[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int i = 2 * ks + a;
            f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kd = 0; kd < KS; ++kd) mma(frag_kc<bf16>(Vs, LDQ, 16 * i, 32 * kd, c, g), of[kd], dp);
            ds2[a] = pj[i] * (dp - dl);
        }
        const Frag<bf16> sf = frag_p_regs<bf16>(ds2[0], ds2[1]);
#pragma unroll
        for (int j = 0; j < DT; ++j) mma(frag_v_perm<bf16>(Ks, LDQ, 16 * j, ks, c, g), sf, acc[j]);  // dQ^T [channel][query]
    }
    store_tile_rows<HD, Cfg::HDP>(acc, scale, dqkv + tok_base * 3 * C, L, 3 * C, u.h * HD, tok, g);
}

// -------------------------------------------------------------------------------------------------------------
// backward, dK and dV of the local keys: own slots = keys, neighbourhood slots = [global queries | local queries]
// -------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_bwd_dkv_local_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                                   const float* __restrict__ lse_in, const float* __restrict__ delta_in,
                                                                   ChunkGeom gm, int L, int nH, float scale, bf16* __restrict__ dqkv) {
    using Cfg = CCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS, DT = Cfg::DT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int* nbtok = reinterpret_cast<int*>(smem_raw);
    int* owntok = nbtok + NBS;
    float* nblse = reinterpret_cast<float*>(owntok + OWS);
    float* nbdelta = nblse + NBS;
    bf16* Qs = reinterpret_cast<bf16*>(nbdelta + NBS);  // Q of the neighbourhood's queries
    bf16* Os = Qs + Cfg::FULL;                           // their dO rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    bf16* Kb = Os + Cfg::FULL + wave * (2 * Cfg::TILE);
    bf16* Vb = Kb + Cfg::TILE;

    const Unit u = unit_of(blockIdx.x, gm, nH);
    const int C = nH * HD;
    const long tok_base = (long)u.b * L;
    const bf16* src = qkv + u.h * HD;

    fill_tables(nbtok, owntok, gm, u.cr, u.cc);
    __syncthreads();
    {
        RowStage<NBS, NTHR, HD> sq, so;
        RowStage<16, 64, HD> sk, sv;
        sq.load(src, 3L * C, nbtok, tok_base, threadIdx.x);
        so.load(dout + u.h * HD, (long)C, nbtok, tok_base, threadIdx.x);
        sk.load(src + C, 3L * C, owntok + 16 * wave, tok_base, lane);
        sv.load(src + 2 * C, 3L * C, owntok + 16 * wave, tok_base, lane);
        for (int s = threadIdx.x; s < NBS; s += NTHR) {
            const int t = nbtok[s];
            // a dead query slot rebuilds P = exp(s - 3e38) = 0
            nblse[s] = t >= 0 ? lse_in[(long)u.z * L + t] : 3.0e38f;
            nbdelta[s] = t >= 0 ? delta_in[(long)u.z * L + t] : 0.f;
        }
        sq.store(Qs, threadIdx.x);
        so.store(Os, threadIdx.x);
        sk.store(Kb, lane);
        sv.store(Vb, lane);
    }
    __syncthreads();
    if (!tile_live(owntok, wave, lane)) return;

    Frag<bf16> kf[KS], vf[KS];
#pragma unroll
    for (int kd = 0; kd < KS; ++kd) {
        kf[kd] = frag_kc<bf16>(Kb, LDQ, 0, 32 * kd, c, g);
        vf[kd] = frag_kc<bf16>(Vb, LDQ, 0, 32 * kd, c, g);
    }
    // P tiles, oriented S: p[j][r] = P[query slot 16 j + 4g + r][key slot 16 wave + c]
    f32x4 p[NBT];
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kd = 0; kd < KS; ++kd) mma(frag_kc<bf16>(Qs, LDQ, 16 * j, 32 * kd, c, g), kf[kd], s);
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(nblse + 16 * j + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = __expf(s[r] * scale - l4[r]);
        p[j] = s;
    }
    const int tok = owntok[16 * wave + c];
    {  // dV[key][d] = sum_q P[q][key] dO[q][d]
        f32x4 av[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) av[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NBS / 32; ++ks) {
            const Frag<bf16> pf = frag_p_regs<bf16>(p[2 * ks], p[2 * ks + 1]);
#pragma unroll
            for (int j = 0; j < DT; ++j) mma(frag_v_perm<bf16>(Os, LDQ, 16 * j, ks, c, g), pf, av[j]);  // dV^T [channel][key]
        }
        store_tile_rows<HD, Cfg::HDP>(av, 1.f, dqkv + tok_base * 3 * C, L, 3 * C, 2 * C + u.h * HD, tok, g);
    }
    // dS = P o (dP - delta), dP[q][key] = sum_d dO[q][d] V[key][d]; dS overwrites P
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
        f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kd = 0; kd < KS; ++kd) mma(frag_kc<bf16>(Os, LDQ, 16 * j, 32 * kd, c, g), vf[kd], dp);
        const f32x4 dl4 = *reinterpret_cast<const f32x4*>(nbdelta + 16 * j + 4 * g);
        p[j] = p[j] * (dp - dl4);
    }
    {  // dK[key][d] = scale sum_q dS[q][key] q[q][d]
        f32x4 ak[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) ak[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NBS / 32; ++ks) {
            const Frag<bf16> sf = frag_p_regs<bf16>(p[2 * ks], p[2 * ks + 1]);
#pragma unroll
            for (int j = 0; j < DT; ++j) mma(frag_v_perm<bf16>(Qs, LDQ, 16 * j, ks, c, g), sf, ak[j]);  // dK^T [channel][key]
        }
        store_tile_rows<HD, Cfg::HDP>(ak, scale, dqkv + tok_base * 3 * C, L, 3 * C, C + u.h * HD, tok, g);
    }
}

// -------------------------------------------------------------------------------------------------------------
// the global tokens: nglo rows / columns against all L tokens, per 512-token range on the VALU
// -------------------------------------------------------------------------------------------------------------
// row t of a token-ordered matrix (HD channels at g) as floats, 8 at a time: acc[r] += sum_d x[d] * w[r][d] for the GMAX rows of w (LDS)
template <int HD>
__device__ __forceinline__ void row_dots(const bf16* __restrict__ row, const float (*w)[64], int nrow, float (&acc)[GMAX]) {
#pragma unroll
    for (int r = 0; r < GMAX; ++r) acc[r] = 0.f;
#pragma unroll
    for (int dv = 0; dv < HD / 8; ++dv) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(row + dv * 8);
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            if (r < nrow) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[r] += (float)x[e] * w[r][dv * 8 + e];
            }
        }
    }
}

// rows of the global tokens of image b, head h (column block col0 of a matrix with row_elems columns) -> float [GMAX][64], zero elsewhere
__device__ __forceinline__ void load_global_rows(float (*dst)[64], const bf16* __restrict__ m, long tok_base, int row_elems, int col0, int hd,
                                                 int nglo, float mul) {
    for (int i = threadIdx.x; i < GMAX * 64; i += NTHR) {
        const int r = i >> 6, d = i & 63;
        dst[r][d] = (r < nglo && d < hd) ? mul * (float)m[(tok_base + r) * row_elems + col0 + d] : 0.f;
    }
}

// sum of v[GMAX] over the four waves of the block for channel lane -> out[r] valid in wave 0; red: [WAVES][GMAX][64] floats
__device__ __forceinline__ void wave_fold(float (&v)[GMAX], float* red, int lane, int wave) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GMAX; ++r) red[(wave * GMAX + r) * 64 + lane] = v[r];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < GMAX; ++r) v[r] = (red[r * 64 + lane] + red[(GMAX + r) * 64 + lane]) + (red[(2 * GMAX + r) * 64 + lane] + red[(3 * GMAX + r) * 64 + lane]);
    }
}

constexpr int FWD_PART = GMAX * 66;      // per (z, range): [GMAX][64 channels | max | sum]
constexpr int BWD_PART = GMAX * 3 * 64;  // per (z, range): [GMAX][dq | dk | dv][64]

template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_fwd_global_part_kernel(const bf16* __restrict__ qkv, int nglo, int L, int nH, float scale,
                                                                     int nsplit, float* __restrict__ part) {
    // (one dynamic block: with separate static arrays the compiler hoists all of qg into registers, 512 of them at head_dim 64)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    typedef float row64[64];
    typedef float rowsp[GSPLIT];
    row64* qg = reinterpret_cast<row64*>(smem_raw);   // scale * q of the global queries
    rowsp* sc = reinterpret_cast<rowsp*>(qg + GMAX);  // scores, then probabilities of this range
    float* red = reinterpret_cast<float*>(sc + GMAX);
    float* scratch = red + WAVES * GMAX * 64;
    const int sp = blockIdx.x, z = blockIdx.y;
    const int b = z / nH, h = z % nH, C = nH * HD;
    const long tok_base = (long)b * L;
    const int t0 = sp * GSPLIT, cnt = min(GSPLIT, L - t0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    load_global_rows(qg, qkv, tok_base, 3 * C, h * HD, HD, nglo, scale);
    __syncthreads();
    float mx[GMAX], sm[GMAX];
#pragma unroll
    for (int r = 0; r < GMAX; ++r) mx[r] = -3.0e38f;
#pragma unroll 1
    for (int jj = threadIdx.x; jj < cnt; jj += NTHR) {
        float s[GMAX];
        row_dots<HD>(qkv + (tok_base + t0 + jj) * 3L * C + C + h * HD, qg, nglo, s);
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            sc[r][jj] = s[r];
            mx[r] = fmaxf(mx[r], s[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < GMAX; ++r) {
        mx[r] = block_max<NTHR>(mx[r], scratch);
        sm[r] = 0.f;
    }
#pragma unroll 1
    for (int jj = threadIdx.x; jj < cnt; jj += NTHR) {  // (a thread re-reads the entries it wrote)
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            const float pe = r < nglo ? __expf(sc[r][jj] - mx[r]) : 0.f;
            sc[r][jj] = pe;
            sm[r] += pe;
        }
    }
#pragma unroll
    for (int r = 0; r < GMAX; ++r) sm[r] = block_sum<NTHR>(sm[r], scratch);
    __syncthreads();
    float acc[GMAX];
#pragma unroll
    for (int r = 0; r < GMAX; ++r) acc[r] = 0.f;
    if (lane < HD) {
        const bf16* vcol = qkv + (tok_base + t0) * 3L * C + 2 * C + h * HD + lane;
        for (int jj = wave; jj < cnt; jj += WAVES) {
            const float v = (float)vcol[(long)jj * 3 * C];
#pragma unroll
            for (int r = 0; r < GMAX; ++r) acc[r] += sc[r][jj] * v;
        }
    }
    wave_fold(acc, red, lane, wave);
    if (wave == 0) {
        float* pw = part + ((long)z * nsplit + sp) * FWD_PART;
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            pw[r * 66 + lane] = acc[r];
            if (lane == 0) {
                pw[r * 66 + 64] = mx[r];
                pw[r * 66 + 65] = sm[r];
            }
        }
    }
}

template <int HD>
__global__ __launch_bounds__(64) void chunk_fwd_global_combine_kernel(const float* __restrict__ part, int nglo, int L, int nH, int nsplit,
                                                                      bf16* __restrict__ out, float* __restrict__ lse_out) {
    const int z = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const int b = z / nH, h = z % nH, C = nH * HD;
    const float* pz = part + (long)z * nsplit * FWD_PART + r * 66;
    float M = -3.0e38f;
    for (int sp = 0; sp < nsplit; ++sp) M = fmaxf(M, pz[(long)sp * FWD_PART + 64]);
    float den = 0.f, num = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) {  // range order: the same sum in every launch
        const float wgt = __expf(pz[(long)sp * FWD_PART + 64] - M);
        den += wgt * pz[(long)sp * FWD_PART + 65];
        num += wgt * pz[(long)sp * FWD_PART + lane];
    }
    if (lane < HD) out[((long)b * L + r) * C + h * HD + lane] = (bf16)(num / den);
    if (lane == 0) lse_out[(long)z * L + r] = M + __logf(den);
}

// delta[z][t] = sum_d dO[t][h, d] * O[t][h, d]
template <int HD>
__global__ void chunk_delta_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ fout, int L, int nH, long total, float* __restrict__ delta) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (b, t, h)
    if (i >= total) return;
    const int h = (int)(i % nH);
    const long bt = i / nH;
    const int b = (int)(bt / L), t = (int)(bt % L);
    const bf16* o = fout + bt * (long)(nH * HD) + h * HD;
    const bf16* d = dout + bt * (long)(nH * HD) + h * HD;
    float s = 0.f;
#pragma unroll
    for (int dv = 0; dv < HD / 8; ++dv) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(o + dv * 8), y = *reinterpret_cast<const bf16x8*>(d + dv * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (float)x[e] * (float)y[e];
    }
    delta[((long)b * nH + h) * L + t] = s;
}

// tokens of one range as QUERIES against the global keys (-> dK, dV of the global keys) and as KEYS of the global queries (-> dQ of
// the global queries)
template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_bwd_global_part_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                                     const float* __restrict__ lse_in, const float* __restrict__ delta_in, int nglo,
                                                                     int L, int nH, float scale, int nsplit, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    typedef float row64[64];
    row64* qg = reinterpret_cast<row64*>(smem_raw);  // scale * q of the global queries
    row64* kg = qg + GMAX;                           // scale * k of the global keys
    row64* vg = kg + GMAX;
    row64* og = vg + GMAX;                           // dO of the global queries
    float* pA = reinterpret_cast<float*>(og + GMAX);  // [GMAX][GSPLIT] P[query jj][global key r]
    float* sA = pA + GMAX * GSPLIT;                   // dS[query jj][global key r]
    float* sB = sA + GMAX * GSPLIT;                   // dS[global query r][key jj]
    float* red = sB + GMAX * GSPLIT;                  // [WAVES][GMAX][64]
    const int sp = blockIdx.x, z = blockIdx.y;
    const int b = z / nH, h = z % nH, C = nH * HD;
    const long tok_base = (long)b * L;
    const int t0 = sp * GSPLIT, cnt = min(GSPLIT, L - t0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    load_global_rows(qg, qkv, tok_base, 3 * C, h * HD, HD, nglo, scale);
    load_global_rows(kg, qkv, tok_base, 3 * C, C + h * HD, HD, nglo, scale);
    load_global_rows(vg, qkv, tok_base, 3 * C, 2 * C + h * HD, HD, nglo, 1.f);
    load_global_rows(og, dout, tok_base, C, h * HD, HD, nglo, 1.f);
    __syncthreads();
#pragma unroll 1
    for (int jj = threadIdx.x; jj < cnt; jj += NTHR) {
        const long t = tok_base + t0 + jj;
        const bf16* qrow = qkv + t * 3L * C + h * HD;
        const bf16* orow = dout + t * (long)C + h * HD;
        float a[GMAX], d[GMAX];
        {  // this token as a query of the global keys
            const float lq = lse_in[(long)z * L + t0 + jj], dl = delta_in[(long)z * L + t0 + jj];
            row_dots<HD>(qrow, kg, nglo, a);
            row_dots<HD>(orow, vg, nglo, d);
#pragma unroll
            for (int r = 0; r < GMAX; ++r) {
                const float pe = r < nglo ? __expf(a[r] - lq) : 0.f;
                pA[r * GSPLIT + jj] = pe;
                sA[r * GSPLIT + jj] = pe * (d[r] - dl);
            }
        }
        {  // this token as a key of the global queries
            row_dots<HD>(qrow + C, qg, nglo, a);
            row_dots<HD>(qrow + 2 * C, og, nglo, d);
#pragma unroll
            for (int r = 0; r < GMAX; ++r) {
                float ds = 0.f;
                if (r < nglo) ds = __expf(a[r] - lse_in[(long)z * L + r]) * (d[r] - delta_in[(long)z * L + r]);
                sB[r * GSPLIT + jj] = ds;
            }
        }
    }
    __syncthreads();
    float aq[GMAX], ak[GMAX], av[GMAX];
#pragma unroll
    for (int r = 0; r < GMAX; ++r) aq[r] = ak[r] = av[r] = 0.f;
    if (lane < HD) {
        const bf16* qcol = qkv + (tok_base + t0) * 3L * C + h * HD + lane;
        const bf16* ocol = dout + (tok_base + t0) * (long)C + h * HD + lane;
        for (int jj = wave; jj < cnt; jj += WAVES) {
            const float qv = (float)qcol[(long)jj * 3 * C], kv = (float)qcol[(long)jj * 3 * C + C], ov = (float)ocol[(long)jj * C];
#pragma unroll
            for (int r = 0; r < GMAX; ++r) {
                av[r] += pA[r * GSPLIT + jj] * ov;
                ak[r] += sA[r * GSPLIT + jj] * qv;
                aq[r] += sB[r * GSPLIT + jj] * kv;
            }
        }
    }
    wave_fold(aq, red, lane, wave);
    wave_fold(ak, red, lane, wave);
    wave_fold(av, red, lane, wave);
    if (wave == 0) {
        float* pw = part + ((long)z * nsplit + sp) * BWD_PART;
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            pw[(r * 3 + 0) * 64 + lane] = aq[r] * scale;
            pw[(r * 3 + 1) * 64 + lane] = ak[r] * scale;
            pw[(r * 3 + 2) * 64 + lane] = av[r];
        }
    }
}

template <int HD>
__global__ __launch_bounds__(64) void chunk_bwd_global_combine_kernel(const float* __restrict__ part, int nglo, int L, int nH, int nsplit,
                                                                      bf16* __restrict__ dqkv) {
    const int z = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const int b = z / nH, h = z % nH, C = nH * HD;
    const float* pz = part + (long)z * nsplit * BWD_PART + r * 3 * 64 + lane;
    float s[3] = {0.f, 0.f, 0.f};
    for (int sp = 0; sp < nsplit; ++sp)  // range order: the same sum in every launch
#pragma unroll
        for (int w = 0; w < 3; ++w) s[w] += pz[(long)sp * BWD_PART + w * 64];
    if (lane < HD) {
#pragma unroll
        for (int w = 0; w < 3; ++w) dqkv[((long)b * L + r) * 3 * C + w * C + h * HD + lane] = (bf16)s[w];
    }
}

// -------------------------------------------------------------------------------------------------------------
// attention statistics (ws | ESVIT_ATTN_SLIDING_CHUNK | ESVIT_ATTN_CHUNK_STATS): what an attention analysis reads, without P and without V
// -------------------------------------------------------------------------------------------------------------
// entropy of the local queries' softmax rows, in nats: chunk_fwd_local_kernel up to its probabilities -- the same staging of K by slot,
// the same 28 score tiles, scale, dead-slot value, maximum and exponentials -- and beside sum = sum_k e^(s_k - m) the second reduction
// us = sum_k e^(s_k - m) (s_k - m), across the tile's lanes as the forward reduces sum.  H = ln sum - us / sum: sum >= 1 (the maximum's
// own term is e^0) and us <= 0, both terms are >= 0 and nothing cancels.  A dead slot has e = exp(-1e30 - m) = 0 and adds an exact
// (signed) zero to both.  No V image, no P V, no out: LDS 42 KB (hd 32) / 74 KB (hd 48, 64).
template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_stats_local_kernel(const bf16* __restrict__ qkv, ChunkGeom gm, int L, int nH, float scale,
                                                                 float* __restrict__ ent) {
    using Cfg = CCfg<HD>;
    constexpr int LDQ = Cfg::LDQ, KS = Cfg::KS;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int* nbtok = reinterpret_cast<int*>(smem_raw);
    int* owntok = nbtok + NBS;
    bf16* Ks = reinterpret_cast<bf16*>(owntok + OWS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    bf16* Qs = Ks + Cfg::FULL + wave * Cfg::TILE;

    const Unit u = unit_of(blockIdx.x, gm, nH);
    const int C = nH * HD;
    const long tok_base = (long)u.b * L;
    const bf16* src = qkv + u.h * HD;

    fill_tables(nbtok, owntok, gm, u.cr, u.cc);
    __syncthreads();
    {
        RowStage<NBS, NTHR, HD> sk;
        RowStage<16, 64, HD> sq;
        sk.load(src + C, 3L * C, nbtok, tok_base, threadIdx.x);
        sq.load(src, 3L * C, owntok + 16 * wave, tok_base, lane);
        sk.store(Ks, threadIdx.x);
        sq.store(Qs, lane);
    }
    __syncthreads();  // K complete; everything below is private to the wave
    if (!tile_live(owntok, wave, lane)) return;

    Frag<bf16> qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = frag_kc<bf16>(Qs, LDQ, 0, 32 * ks, c, g);
    f32x4 p[NBT];
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) mma(frag_kc<bf16>(Ks, LDQ, 16 * i, 32 * ks, c, g), qf[ks], s);
        const i32x4 tk = *reinterpret_cast<const i32x4*>(nbtok + 16 * i + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = tk[r] >= 0 ? s[r] * scale : -1.0e30f;
            m = fmaxf(m, s[r]);
        }
        p[i] = s;
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f, us = 0.f;
#pragma unroll
    for (int i = 0; i < NBT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = p[i][r] - m;
            const float e = __expf(d);  // a dead slot: exp(-1e30 - m) = 0, 0 * -1e30 = -0
            sum += e;
            us += e * d;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    us += __shfl_xor(us, 16, 64);
    us += __shfl_xor(us, 32, 64);
    const int tok = owntok[16 * wave + c];
    if (g == 0 && tok >= 0) ent[(long)u.z * L + tok] = __logf(sum) - us / sum;
}

// the global queries: per 512-key range (m_r, l_r = sum e^(s - m_r), T_r = sum e^(s - m_r)(s - m_r)) per global query, scores as
// chunk_fwd_global_part_kernel forms them, no V loop
constexpr int STAT_PART = GMAX * 3;  // per (z, range): [GMAX][max | sum | T]  (<= FWD_PART: the forward's scratch suffices)
static_assert(STAT_PART <= FWD_PART, "the statistics partials must fit the forward's scratch");

template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_stats_global_part_kernel(const bf16* __restrict__ qkv, int nglo, int L, int nH, float scale,
                                                                       int nsplit, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    typedef float row64[64];
    typedef float rowsp[GSPLIT];
    row64* qg = reinterpret_cast<row64*>(smem_raw);   // scale * q of the global queries
    rowsp* sc = reinterpret_cast<rowsp*>(qg + GMAX);  // scores of this range
    float* scratch = reinterpret_cast<float*>(sc + GMAX);
    const int sp = blockIdx.x, z = blockIdx.y;
    const int b = z / nH, h = z % nH, C = nH * HD;
    const long tok_base = (long)b * L;
    const int t0 = sp * GSPLIT, cnt = min(GSPLIT, L - t0);
    load_global_rows(qg, qkv, tok_base, 3 * C, h * HD, HD, nglo, scale);
    __syncthreads();
    float mx[GMAX], sm[GMAX], tt[GMAX];
#pragma unroll
    for (int r = 0; r < GMAX; ++r) mx[r] = -3.0e38f;
#pragma unroll 1
    for (int jj = threadIdx.x; jj < cnt; jj += NTHR) {
        float s[GMAX];
        row_dots<HD>(qkv + (tok_base + t0 + jj) * 3L * C + C + h * HD, qg, nglo, s);
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            sc[r][jj] = s[r];
            mx[r] = fmaxf(mx[r], s[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < GMAX; ++r) {
        mx[r] = block_max<NTHR>(mx[r], scratch);
        sm[r] = 0.f;
        tt[r] = 0.f;
    }
#pragma unroll 1
    for (int jj = threadIdx.x; jj < cnt; jj += NTHR) {  // (a thread re-reads the entries it wrote)
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            const float d = sc[r][jj] - mx[r];
            const float pe = r < nglo ? __expf(d) : 0.f;
            sm[r] += pe;
            tt[r] += pe * d;
        }
    }
#pragma unroll
    for (int r = 0; r < GMAX; ++r) {
        sm[r] = block_sum<NTHR>(sm[r], scratch);
        tt[r] = block_sum<NTHR>(tt[r], scratch);
    }
    if (threadIdx.x == 0) {
        float* pw = part + ((long)z * nsplit + sp) * STAT_PART;
#pragma unroll
        for (int r = 0; r < GMAX; ++r) {
            pw[r * 3 + 0] = mx[r];
            pw[r * 3 + 1] = sm[r];
            pw[r * 3 + 2] = tt[r];
        }
    }
}

// the ranges merged in range order: with M the row's maximum and w_r = e^(m_r - M), l = sum w_r l_r and T = sum w_r (T_r + (m_r - M) l_r)
// (every term e^(s - m_r)(s - m_r) of range r becomes w_r e^(s - m_r)((s - m_r) + (m_r - M))); H = ln l - T / l.  An underflowed w_r is
// 0 and multiplies finite numbers: it contributes an exact zero.  One thread per (image, head, global query).
__global__ __launch_bounds__(64) void chunk_stats_global_combine_kernel(const float* __restrict__ part, int nglo, int L, int nsplit,
                                                                        float* __restrict__ ent) {
    const int z = blockIdx.x, r = threadIdx.x;
    if (r >= nglo) return;
    const float* pz = part + (long)z * nsplit * STAT_PART + r * 3;
    float M = -3.0e38f;
    for (int sp = 0; sp < nsplit; ++sp) M = fmaxf(M, pz[(long)sp * STAT_PART]);
    float l = 0.f, T = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) {  // range order: the same sum in every launch
        const float dm = pz[(long)sp * STAT_PART] - M, lr = pz[(long)sp * STAT_PART + 1], Tr = pz[(long)sp * STAT_PART + 2];
        const float wgt = __expf(dm);
        l += wgt * lr;
        T += wgt * (Tr + dm * lr);
    }
    ent[(long)z * L + r] = __logf(l) - T / l;
}

// probability rows of the listed queries: one workgroup per (image, head, listed query) walks ALL L keys on the VALU.  A key the query
// does not see (chunk_geom.h's neighbourhood in closed form: a local query sees the globals and the tokens whose chunk differs from its
// own by at most one in both directions; a global query sees everything) gets an exact 0; a key it sees gets its score in the first
// sweep, which the same thread replaces by e^(s - m) / l in the second (every element of the row has one writing thread; m and l are
// the row's own maximum and sum).  A listed index outside [0, L) is skipped: its row stays unwritten, nothing is read.
template <int HD>
__global__ __launch_bounds__(NTHR) void chunk_stats_rows_kernel(const bf16* __restrict__ qkv, const int32_t* __restrict__ qidx, int nq,
                                                                ChunkGeom gm, int L, int nH, float scale, float* __restrict__ rows) {
    __shared__ float qs[64];
    __shared__ float scratch[WAVES];
    const int j = blockIdx.x, z = blockIdx.y;
    const int t = qidx[j];
    if (t < 0 || t >= L) return;  // (uniform over the workgroup)
    const int b = z / nH, h = z % nH, C = nH * HD;
    const long tok_base = (long)b * L;
    if (threadIdx.x < 64) qs[threadIdx.x] = threadIdx.x < HD ? scale * (float)qkv[(tok_base + t) * 3L * C + h * HD + threadIdx.x] : 0.f;
    __syncthreads();
    const int nglo = gm.nglo;
    const bool qglob = t < nglo;
    const int qcx = qglob ? 0 : ((t - nglo) / gm.ny) / gm.w, qcy = qglob ? 0 : ((t - nglo) % gm.ny) / gm.w;
    float* row = rows + ((long)z * nq + j) * L;
    float m = -3.0e38f;
#pragma unroll 1
    for (int k = threadIdx.x; k < L; k += NTHR) {
        bool see = qglob || k < nglo;
        if (!see) {
            const int dx = ((k - nglo) / gm.ny) / gm.w - qcx, dy = ((k - nglo) % gm.ny) / gm.w - qcy;
            see = dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1;
        }
        float s = 0.f;
        if (see) {
            const bf16* krow = qkv + (tok_base + k) * 3L * C + C + h * HD;
#pragma unroll
            for (int dv = 0; dv < HD / 8; ++dv) {
                const bf16x8 x = *reinterpret_cast<const bf16x8*>(krow + dv * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += (float)x[e] * qs[dv * 8 + e];
            }
            m = fmaxf(m, s);
        }
        row[k] = s;
    }
    m = block_max<NTHR>(m, scratch);
    float l = 0.f;
#pragma unroll 1
    for (int k = threadIdx.x; k < L; k += NTHR) {  // (a thread re-reads the entries it wrote)
        bool see = qglob || k < nglo;
        if (!see) {
            const int dx = ((k - nglo) / gm.ny) / gm.w - qcx, dy = ((k - nglo) % gm.ny) / gm.w - qcy;
            see = dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1;
        }
        if (see) {
            const float e = __expf(row[k] - m);
            row[k] = e;
            l += e;
        }
    }
    l = block_sum<NTHR>(l, scratch);
#pragma unroll 1
    for (int k = threadIdx.x; k < L; k += NTHR) row[k] = row[k] / l;  // (l >= 1: the maximum's own term; an unseen key stays 0)
}

template <int HD>
size_t local_lds(int per_wave_tiles, bool stats) {
    using Cfg = CCfg<HD>;
    return (size_t)(NBS + OWS) * 4 + (stats ? 2 * NBS * 4 : 0) + (size_t)(2 * Cfg::FULL + WAVES * per_wave_tiles * Cfg::TILE) * 2;
}
constexpr size_t FWD_GLOBAL_LDS = (size_t)(GMAX * 64 + GMAX * GSPLIT + WAVES * GMAX * 64 + WAVES) * 4;
constexpr size_t STATS_GLOBAL_LDS = (size_t)(GMAX * 64 + GMAX * GSPLIT + WAVES) * 4;
constexpr size_t BWD_GLOBAL_LDS =(size_t)(4 * GMAX * 64 + 3 * GMAX * GSPLIT + WAVES * GMAX * 64) * 4;

inline int nsplit_of(int L) { return (L + GSPLIT - 1) / GSPLIT; }

template <int HD>
int fwd_launch(const bf16* qkv, const ChunkGeom& gm, int L, int nB, int nH, float scale, bf16* out, float* lse, float* ws, hipStream_t stream) {
    const int Z = nB * nH, nsplit = nsplit_of(L);
    {
        auto kern = chunk_fwd_local_kernel<HD>;
        const size_t lds = local_lds<HD>(1, false);
        static unsigned long long raised = 0;
        esvit_raise_lds(kern, (int)lds, raised);
        hipLaunchKernelGGL(kern, dim3(Z * cg_chunks(gm)), dim3(NTHR), lds, stream, qkv, gm, L, nH, scale, out, lse);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(sliding chunk, local)");
    }
    if (gm.nglo > 0) {
        hipLaunchKernelGGL(chunk_fwd_global_part_kernel<HD>, dim3(nsplit, Z), dim3(NTHR), FWD_GLOBAL_LDS, stream, qkv, gm.nglo, L, nH, scale, nsplit, ws);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(sliding chunk, global rows)");
        hipLaunchKernelGGL(chunk_fwd_global_combine_kernel<HD>, dim3(Z, gm.nglo), dim3(64), 0, stream, ws, gm.nglo, L, nH, nsplit, out, lse);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(sliding chunk, global rows combine)");
    }
    return ESVIT_OK;
}

template <int HD>
int stats_launch(const bf16* qkv, const ChunkGeom& gm, int L, int nB, int nH, float scale, const int32_t* qidx, int nq, float* ent, float* rows,
                 float* ws, hipStream_t stream) {
    using Cfg = CCfg<HD>;
    const int Z = nB * nH, nsplit = nsplit_of(L);
    {
        auto kern = chunk_stats_local_kernel<HD>;
        const size_t lds = (size_t)(NBS + OWS) * 4 + (size_t)(Cfg::FULL + WAVES * Cfg::TILE) * 2;
        static unsigned long long raised = 0;
        esvit_raise_lds(kern, (int)lds, raised);
        hipLaunchKernelGGL(kern, dim3(Z * cg_chunks(gm)), dim3(NTHR), lds, stream, qkv, gm, L, nH, scale, ent);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(sliding chunk stats, local)");
    }
    if (gm.nglo > 0) {
        hipLaunchKernelGGL(chunk_stats_global_part_kernel<HD>, dim3(nsplit, Z), dim3(NTHR), STATS_GLOBAL_LDS, stream, qkv, gm.nglo, L, nH, scale, nsplit, ws);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(sliding chunk stats, global rows)");
        hipLaunchKernelGGL(chunk_stats_global_combine_kernel, dim3(Z), dim3(64), 0, stream, (const float*)ws, gm.nglo, L, nsplit, ent);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(sliding chunk stats, global rows combine)");
    }
    if (nq > 0) {
        hipLaunchKernelGGL(chunk_stats_rows_kernel<HD>, dim3(nq, Z), dim3(NTHR), 0, stream, qkv, qidx, nq, gm, L, nH, scale, rows);
        ESVIT_CHECK_LAUNCH("window_attn_fwd(sliding chunk stats, listed rows)");
    }
    return ESVIT_OK;
}

template <int HD>
int bwd_launch(const bf16* qkv, const bf16* dout, const bf16* fout, const float* lse, const ChunkGeom& gm, int L, int nB, int nH, float scale,
               bf16* dqkv, float* ws, hipStream_t stream) {
    const int Z = nB * nH, nsplit = nsplit_of(L);
    float* delta = ws;                 // [Z, L]
    float* part = ws + (long)Z * L;    // [Z, nsplit, BWD_PART]
    {
        const long total = (long)nB * L * nH;
        hipLaunchKernelGGL(chunk_delta_kernel<HD>, dim3(ceil_div(total, 256)), dim3(256), 0, stream, dout, fout, L, nH, total, delta);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(sliding chunk, delta)");
    }
    {
        auto kern = chunk_bwd_dq_local_kernel<HD>;
        const size_t lds = local_lds<HD>(2, false);
        static unsigned long long raised = 0;
        esvit_raise_lds(kern, (int)lds, raised);
        hipLaunchKernelGGL(kern, dim3(Z * cg_chunks(gm)), dim3(NTHR), lds, stream, qkv, dout, lse, (const float*)delta, gm, L, nH, scale, dqkv);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(sliding chunk, dQ)");
    }
    {
        auto kern = chunk_bwd_dkv_local_kernel<HD>;
        const size_t lds = local_lds<HD>(2, true);
        static unsigned long long raised = 0;
        esvit_raise_lds(kern, (int)lds, raised);
        hipLaunchKernelGGL(kern, dim3(Z * cg_chunks(gm)), dim3(NTHR), lds, stream, qkv, dout, lse, (const float*)delta, gm, L, nH, scale, dqkv);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(sliding chunk, dK dV)");
    }
    if (gm.nglo > 0) {
        auto kern = chunk_bwd_global_part_kernel<HD>;
        static unsigned long long raised = 0;
        esvit_raise_lds(kern, (int)BWD_GLOBAL_LDS, raised);
        hipLaunchKernelGGL(kern, dim3(nsplit, Z), dim3(NTHR), BWD_GLOBAL_LDS, stream, qkv, dout, lse, (const float*)delta, gm.nglo, L, nH, scale,
                           nsplit, part);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(sliding chunk, global tokens)");
        hipLaunchKernelGGL(chunk_bwd_global_combine_kernel<HD>, dim3(Z, gm.nglo), dim3(64), 0, stream, (const float*)part, gm.nglo, L, nH, nsplit, dqkv);
        ESVIT_CHECK_LAUNCH("window_attn_bwd(sliding chunk, global tokens combine)");
    }
    return ESVIT_OK;
}

// argument checks shared by the two entries; no HIP call before they pass
int check_mode(const char* who, int dtype, int L, int ws, int nx, int ny, int nB, int nH, int hd, int* nglo_out) {
    ESVIT_CHECK_ARG(dtype == ESVIT_BF16, "%s (sliding chunk): bf16 only (the fp32 parity mode keeps the dense route)", who);
    ESVIT_CHECK_ARG(hd == 32 || hd == 48 || hd == 64, "%s (sliding chunk): head_dim %d unsupported (32, 48 or 64)", who, hd);
    ESVIT_CHECK_ARG(ws == CG_W, "%s (sliding chunk): chunk side %d unsupported (7)", who, ws);
    ESVIT_CHECK_ARG(nB > 0 && nH > 0 && nx > 0 && ny > 0 && L >= (long)nx * ny, "%s (sliding chunk): bad geometry L=%d grid %dx%d", who, L, nx, ny);
    const int nglo = L - nx * ny;
    ESVIT_CHECK_ARG(nglo <= CG_MAX_NGLO && cg_supported(nglo, nx, ny, ws), "%s (sliding chunk): %d global tokens, at most %d", who, nglo, CG_MAX_NGLO);
    ESVIT_CHECK_ARG((long)L * 3 * nH * hd * 2 < 0x7fff0000L, "%s (sliding chunk): one image's qkv rows must fit a 2 GiB buffer descriptor", who);
    *nglo_out = nglo;
    return ESVIT_OK;
}

}  // namespace

// esvit_query(ESVIT_Q_CHUNK_ATTN_WS, nB * nH, L, backward): floats of the scratch the mode takes through bias_frag_ws
int64_t esvit_i_chunk_attn_ws(int64_t Z, int64_t L, int64_t backward) {
    if (Z <= 0 || L <= 0) return 0;
    const int64_t nsplit = (L + GSPLIT - 1) / GSPLIT;
    return backward ? Z * L + Z * nsplit * BWD_PART : Z * nsplit * FWD_PART;
}

int esvit_chunk_attn_fwd(int dtype, const void* qkv, const int32_t* chunk_table, int L, int ws, float* scratch, int nx, int nB, int ny, int nH,
                         int hd, float scale, void* out, float* lse, float* attn_out, hipStream_t stream) {
    int nglo = 0;
    const int rc = check_mode("esvit_window_attn_fwd", dtype, L, ws, nx, ny, nB, nH, hd, &nglo);
    if (rc != ESVIT_OK) return rc;
    ESVIT_CHECK_ARG(qkv && chunk_table && out && lse && scratch && !attn_out,
                    "esvit_window_attn_fwd (sliding chunk): qkv, the chunk table, out, lse and the scratch are required, attn_out is not available");
    const ChunkGeom gm = cg_make(nglo, nx, ny, ws);
    if (hd == 32) return fwd_launch<32>((const bf16*)qkv, gm, L, nB, nH, scale, (bf16*)out, lse, scratch, stream);
    if (hd == 48) return fwd_launch<48>((const bf16*)qkv, gm, L, nB, nH, scale, (bf16*)out, lse, scratch, stream);
    return fwd_launch<64>((const bf16*)qkv, gm, L, nB, nH, scale, (bf16*)out, lse, scratch, stream);
}

int esvit_chunk_attn_bwd(int dtype, const void* qkv, const int32_t* chunk_table, int L, const void* dout, const void* fwd_out, const float* lse,
                         int ws, float* scratch, int nx, int nB, int ny, int nH, int hd, float scale, void* dqkv, hipStream_t stream) {
    int nglo = 0;
    const int rc = check_mode("esvit_window_attn_bwd", dtype, L, ws, nx, ny, nB, nH, hd, &nglo);
    if (rc != ESVIT_OK) return rc;
    ESVIT_CHECK_ARG(qkv && chunk_table && dout && fwd_out && lse && dqkv && scratch,
                    "esvit_window_attn_bwd (sliding chunk): qkv, the chunk table, dout, fwd_out, lse, dqkv and the scratch are required");
    const ChunkGeom gm = cg_make(nglo, nx, ny, ws);
    if (hd == 32) return bwd_launch<32>((const bf16*)qkv, (const bf16*)dout, (const bf16*)fwd_out, lse, gm, L, nB, nH, scale, (bf16*)dqkv, scratch, stream);
    if (hd == 48) return bwd_launch<48>((const bf16*)qkv, (const bf16*)dout, (const bf16*)fwd_out, lse, gm, L, nB, nH, scale, (bf16*)dqkv, scratch, stream);
    return bwd_launch<64>((const bf16*)qkv, (const bf16*)dout, (const bf16*)fwd_out, lse, gm, L, nB, nH, scale, (bf16*)dqkv, scratch, stream);
}

// the statistics mode of the forward entry (ws | ESVIT_ATTN_SLIDING_CHUNK | ESVIT_ATTN_CHUNK_STATS, include/esvit_hip.h): every check
// before any launch.  ws arrives with all its flags; forward_entry = false: the call came through esvit_window_attn_bwd
int esvit_chunk_attn_stats(bool forward_entry, int dtype, const void* qkv, const float* qkv_bias, const int32_t* chunk_table, int L,
                           const float* rel_table, int ws, float* scratch, const int32_t* region_ids, int nx, int nB, int Nq, int nH, int hd,
                           float scale, const void* out, float* lse, float* attn_out, hipStream_t stream) {
    const char* who = "esvit_window_attn_fwd (sliding chunk stats)";
    ESVIT_CHECK_ARG(forward_entry, "esvit_window_attn_bwd: ESVIT_ATTN_CHUNK_STATS is valid in esvit_window_attn_fwd only (ws = 0x%x)", (unsigned)ws);
    ESVIT_CHECK_ARG(!(ws & ESVIT_ATTN_GLOBAL), "%s: ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_GLOBAL (ws = 0x%x)", who, (unsigned)ws);
    ESVIT_CHECK_ARG(!(ws & ESVIT_ATTN_STATS), "%s: ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_STATS (ws = 0x%x)", who, (unsigned)ws);
    ESVIT_CHECK_ARG(!(ws & ESVIT_ATTN_WINDOW_STATS), "%s: ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_WINDOW_STATS (ws = 0x%x)", who, (unsigned)ws);
    ESVIT_CHECK_ARG(!(ws & ESVIT_ATTN_SPLIT_DBIAS), "%s: ESVIT_ATTN_CHUNK_STATS together with ESVIT_ATTN_SPLIT_DBIAS (ws = 0x%x)", who, (unsigned)ws);
    ESVIT_CHECK_ARG(ws & ESVIT_ATTN_SLIDING_CHUNK, "%s: ESVIT_ATTN_CHUNK_STATS is a mode of the sliding-chunk forward, ESVIT_ATTN_SLIDING_CHUNK is missing (ws = 0x%x)",
                    who, (unsigned)ws);
    ws &= ~(ESVIT_ATTN_SLIDING_CHUNK | ESVIT_ATTN_CHUNK_STATS);
    ESVIT_CHECK_ARG(Nq > 0, "%s: N = ny | nq << 16 must be positive (got %d)", who, Nq);
    const int ny = Nq & 0xffff, nq = Nq >> 16;
    int nglo = 0;
    const int rc = check_mode(who, dtype, L, ws, nx, ny, nB, nH, hd, &nglo);
    if (rc != ESVIT_OK) return rc;
    ESVIT_CHECK_ARG(qkv && chunk_table && scratch, "%s: qkv, the chunk table and the scratch are required", who);
    ESVIT_CHECK_ARG(!qkv_bias && !rel_table && !region_ids, "%s: qkv_bias, rel_table and region_ids are not used, pass NULL", who);
    ESVIT_CHECK_ARG(attn_out != nullptr, "%s: attn_out (the entropies, fp32 [nB, nH, L]) is required", who);
    ESVIT_CHECK_ARG(nq == 0 || out != nullptr, "%s: nq = %d listed queries without the list (out: int32 [nq] on the device)", who, nq);
    ESVIT_CHECK_ARG(nq == 0 || lse != nullptr, "%s: nq = %d listed queries without the rows output (lse: fp32 [nB, nH, nq, L])", who, nq);
    ESVIT_CHECK_ARG(nq > 0 || !out, "%s: out must be NULL when no query is listed (nq = 0)", who);
    ESVIT_CHECK_ARG(nq > 0 || !lse, "%s: lse must be NULL when no query is listed (nq = 0)", who);
    ESVIT_CHECK_ARG((long)nB * nH <= 65535, "%s: nB * nH = %ld exceeds the 65535 rows of a launch grid", who, (long)nB * nH);
    const ChunkGeom gm = cg_make(nglo, nx, ny, ws);
    const int32_t* qidx = static_cast<const int32_t*>(out);
    if (hd == 32) return stats_launch<32>((const bf16*)qkv, gm, L, nB, nH, scale, qidx, nq, attn_out, lse, scratch, stream);
    if (hd == 48) return stats_launch<48>((const bf16*)qkv, gm, L, nB, nH, scale, qidx, nq, attn_out, lse, scratch, stream);
    return stats_launch<64>((const bf16*)qkv, gm, L, nB, nH, scale, qidx, nq, attn_out, lse, scratch, stream);
}
