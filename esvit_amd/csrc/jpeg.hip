// JPEG decoder: baseline Huffman JPEG (SOF0 / SOF1, 8-bit) from encoded bytes to the packed HWC images esvit_aug_crops reads,
// bit-exact with Pillow's default decode (libjpeg islow IDCT, fancy upsampling, jdcolor.c tables; arithmetic in jpeg_math.h).
//
// The host (esvit_amd/jpeg.py, a DataLoader worker) has parsed the markers, built the canonical Huffman lookup records (T.81
// Annex C), removed the FF 00 stuffing and split every scan at its restart markers into SEGMENTS (each starts byte-aligned with a
// fresh decoder state and DC predictors of zero).  Every segment is cut into LANES of ESVIT_JPEG_LANE_BITS bits.
//
// Entropy decode, mode 0 (self-synchronising parallel decode, Weissenberger & Schmidt, ICPP 2018 / HiPC 2021):
//   jpeg_sync_pass  x P  a lane decodes the symbols that START inside its bit range from an entry state (bit position,
//                        block-in-MCU u, zig-zag index k) and records the exit state, the blocks it began and the per-component
//                        sum of its DC differences.  Pass 0 guesses the entry (own start bit, u = 0, k = 0); pass p >= 1 takes the
//                        exit of the lane before it in pass p - 1 (the first lane of a segment: the true start state).  A lane
//                        whose entry did not change since the last pass copies its record (cheap).  No lane waits for another
//                        workgroup: every pass is a whole launch.
//   jpeg_scan            one workgroup per segment: converged iff no lane's entry changed in the last pass (then, by induction over
//                        the lanes, every entry IS the state the serial decoder reaches at that lane's start); exclusive prefixes
//                        of the block counts and DC sums give each lane its first block and its DC predictors; a real decode
//                        error or a segment that ends before its last block marks the segment corrupt.
//   jpeg_write           each lane of a converged segment decodes again from its true entry and writes int16 coefficients in
//                        natural order into the block slots fixed by the header (absolute DC = predictor + running sum).
//   jpeg_serial          one lane per segment that did not converge within P passes (mode 1: every segment) decodes it from the
//                        start, serially: the A/B reference and the bound of mode 0.
// Reconstruction: jpeg_idct (one thread per 8 x 8 block: dequantise + islow IDCT -> uint8 component planes) and jpeg_color
// (one thread per pixel: fancy upsampling of the chroma planes, YCbCr -> RGB, packed HWC out).
//
// Robustness: every decode loop is bounded by its segment's bit count (a symbol is decoded only if it starts before the end), a
// read past the end sees the >= 8 zero bytes the host appends to every segment, every coefficient write is bounded by the block
// count of the header, and the per-image status records corrupt entropy data (the caller re-decodes such an image on the host).
#include "common.h"
#include "esvit_hip.h"
#include "jpeg_math.h"

namespace {

constexpr int LB = ESVIT_JPEG_LANE_BITS;
constexpr int LANE_INTS = 12;  // entry pos, u, k | exit pos, u, k | blocks begun | dc sum 0..2 | error block (rel) | changed
constexpr int NO_ERR = 0x7fffffff;
constexpr int ERR_POS = 0x7fffffff;  // the position a decode loop leaves at when it meets an error
constexpr int DEFAULT_PASSES = 8;

// image record (include/esvit_hip.h, ESVIT_JPEG_IMG_INTS)
enum { I_H = 0, I_W, I_NCOMP, I_HMAX, I_VMAX, I_MCUX, I_MCUY, I_BPM, I_RESTART, I_SEG0, I_NSEG, I_BLOCK0, I_PLANE0, I_NBLOCKS, I_PLANEB,
       I_HOST, I_COMP };
enum { C_H = 0, C_V, C_Q, C_DC, C_AC, C_BW, C_BH, C_BOFF, C_POFF, C_CW, C_CH, C_INTS = 12 };
// segment record
enum { S_IMG = 0, S_BITS, S_BYTE, S_MCU0, S_NMCU, S_LANE0, S_NLANES };

// per-image constants of the decode loop; per-component fields are read from the record when a block starts (a select between
// register copies of them is turned into an indexed private array, i.e. scratch)
struct Img {
    const int32_t* rec;
    const int32_t* huff;
    int bpm, n0, h0, v0, mcux, block0;
};

__device__ __forceinline__ Img load_img(const int32_t* rec, const int32_t* huff) {
    Img m;
    m.rec = rec;
    m.huff = huff;
    m.bpm = rec[I_BPM];
    m.mcux = rec[I_MCUX];
    m.block0 = rec[I_BLOCK0];
    m.h0 = rec[I_COMP + C_H];
    m.v0 = rec[I_COMP + C_V];
    m.n0 = m.h0 * m.v0;
    return m;
}

__device__ __forceinline__ int comp_of(const Img& m, int u) { return u < m.n0 ? 0 : u - m.n0 + 1; }

__device__ __forceinline__ const int32_t* table_of(const Img& m, int c, int which) {
    return m.huff + (long)ESVIT_JPEG_HUFF_INTS * m.rec[I_COMP + C_INTS * c + which];
}

// block slot (global, in blocks) of block n of a segment whose first MCU is mcu0
__device__ __forceinline__ long block_slot(const Img& m, int mcu0, int n) {
    const int mcu = mcu0 + n / m.bpm, u = n % m.bpm;
    const int c = comp_of(m, u);
    const int dy = c == 0 ? u / m.h0 : 0, dx = c == 0 ? u % m.h0 : 0;
    const int my = mcu / m.mcux, mx = mcu % m.mcux;
    const int hc = c == 0 ? m.h0 : 1, vc = c == 0 ? m.v0 : 1;
    const int32_t* cr = m.rec + I_COMP + C_INTS * c;
    return (long)m.block0 + cr[C_BOFF] + (long)(my * vc + dy) * cr[C_BW] + mx * hc + dx;
}

// 32 bits of the segment starting at bit `pos` (MSB first); the segment is 4-byte aligned and followed by >= 8 zero bytes
__device__ __forceinline__ uint32_t peek32(const uint32_t* w, int pos) {
    const int i = pos >> 5, sh = pos & 31;
    const uint32_t a = __builtin_bswap32(w[i]), b = __builtin_bswap32(w[i + 1]);
    return sh ? (a << sh) | (b >> (32 - sh)) : a;
}

// one Huffman symbol from the top of `bits`; -1: no code of 16 bits or fewer matches
__device__ __forceinline__ int huff_decode(const int32_t* t, uint32_t bits, int& len) {
    const int e = t[bits >> 23];
    if (e) {
        len = e >> 8;
        return e & 255;
    }
    int l = 10;
    int code = (int)(bits >> 22);
    while (code > t[512 + l]) {  // maxcode[17] is INT_MAX
        ++l;
        code = (int)(bits >> (32 - l));
    }
    if (l > 16) return -1;
    len = l;
    return t[548 + ((t[530 + l] + code) & 255)];
}

__device__ __forceinline__ int extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

struct State {
    int pos, u, k;
};

struct Acc {
    int nblk, dc0, dc1, dc2, err;
};

// Decode the symbols that start before `end` from state `st`.  WRITE: coefficients of blocks g0 + i (i-th block begun here;
// g0 - 1 for the block in progress at entry) go to their slots when below `nblk_seg`; the DC predictors start at pred[].
// `stop`: end once all nblk_seg blocks are complete (the caller knows g0).
template <bool WRITE>
__device__ __forceinline__ void run(const Img& m, const uint32_t* w, int nbits, int end, State& st, Acc& a, int mcu0, int nblk_seg, int g0, int p0, int p1,
                    int p2, int16_t* __restrict__ coef, bool stop) {
    int pos = st.pos, u = st.u, k = st.k;
    int nblk = 0, d0 = 0, d1 = 0, d2 = 0, err = NO_ERR;
    int16_t* blk = nullptr;
    int c = comp_of(m, u);
    const int32_t* tdc = table_of(m, c, C_DC);
    const int32_t* tac = table_of(m, c, C_AC);
    if (WRITE && k > 0 && g0 >= 1 && g0 - 1 < nblk_seg) blk = coef + 64 * block_slot(m, mcu0, g0 - 1);
    while (pos < end) {
        if (stop && k == 0 && g0 + nblk >= nblk_seg) break;
        const uint32_t bits = peek32(w, pos);
        int len;
        if (k == 0) {
            const int sym = huff_decode(tdc, bits, len);
            if (sym < 0) {
                err = nblk;
                pos = ERR_POS;
                break;
            }
            const int s = sym & 15;
            const int diff = s ? extend((bits << len) >> (32 - s), s) : 0;
            pos += len + s;
            if (pos > nbits) {
                err = nblk;
                pos = ERR_POS;
                break;
            }
            d0 += c == 0 ? diff : 0;
            d1 += c == 1 ? diff : 0;
            d2 += c == 2 ? diff : 0;
            if (WRITE) {
                const int b = g0 + nblk;
                blk = b < nblk_seg ? coef + 64 * block_slot(m, mcu0, b) : nullptr;
                if (blk) blk[0] = (int16_t)(c == 0 ? p0 + d0 : (c == 1 ? p1 + d1 : p2 + d2));
            }
            ++nblk;
            k = 1;
        } else {
            const int sym = huff_decode(tac, bits, len);
            if (sym < 0) {
                err = nblk - 1;
                pos = ERR_POS;
                break;
            }
            const int r = sym >> 4, s = sym & 15;
            if (s) {
                k += r;
                const int val = extend((bits << len) >> (32 - s), s);
                pos += len + s;
                if (pos > nbits) {
                    err = nblk - 1;
                    pos = ERR_POS;
                    break;
                }
                if (WRITE && blk) blk[jpg::kNatural[k < 63 ? k : 63]] = (int16_t)val;  // jdhuff.c: a run past 63 lands on 63
                ++k;
            } else {
                pos += len;
                if (pos > nbits) {
                    err = nblk - 1;
                    pos = ERR_POS;
                    break;
                }
                k = r == 15 ? k + 16 : 64;  // ZRL / EOB
            }
        }
        if (k >= 64) {
            k = 0;
            u = u + 1 == m.bpm ? 0 : u + 1;
            const int c2 = comp_of(m, u);
            if (c2 != c) {
                c = c2;
                tdc = table_of(m, c, C_DC);
                tac = table_of(m, c, C_AC);
            }
        }
    }
    st.pos = pos;
    st.u = u;
    st.k = k;
    a.nblk = nblk;
    a.dc0 = d0;
    a.dc1 = d1;
    a.dc2 = d2;
    a.err = err;
}

struct Args {
    const int32_t* images;
    const int32_t* segments;
    const int32_t* lane_seg;
    const int32_t* huff;
    const int32_t* quant;
    const uint8_t* scan;
    const int64_t* table;
    uint8_t* out;
    int32_t* status;
    int n_images, n_segments, n_lanes;
};

__global__ __launch_bounds__(256) void jpeg_sync_pass(Args A, int pass, const int32_t* __restrict__ prev, int32_t* __restrict__ cur) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= A.n_lanes) return;
    const int s = A.lane_seg[j];
    const int32_t* sr = A.segments + (long)s * ESVIT_JPEG_SEG_INTS;
    const int local = j - sr[S_LANE0];
    State st;
    if (local == 0) st = {0, 0, 0};
    else if (pass == 0) st = {local * LB, 0, 0};
    else st = {prev[(long)(j - 1) * LANE_INTS + 3], prev[(long)(j - 1) * LANE_INTS + 4], prev[(long)(j - 1) * LANE_INTS + 5]};
    int32_t* o = cur + (long)j * LANE_INTS;
    if (pass > 0) {
        const int32_t* p = prev + (long)j * LANE_INTS;
        if (p[0] == st.pos && p[1] == st.u && p[2] == st.k) {
#pragma unroll
            for (int i = 0; i < LANE_INTS - 1; ++i) o[i] = p[i];
            o[LANE_INTS - 1] = 0;
            return;
        }
    }
    o[0] = st.pos;
    o[1] = st.u;
    o[2] = st.k;
    const int nbits = sr[S_BITS];
    const int end = min((local + 1) * LB, nbits);
    const Img m = load_img(A.images + (long)sr[S_IMG] * ESVIT_JPEG_IMG_INTS, A.huff);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(A.scan + sr[S_BYTE]);
    Acc a;
    run<false>(m, w, nbits, end, st, a, 0, 0, 0, 0, 0, 0, nullptr, false);
    // an error (on a guessed path, almost always) hands the next lane the same guess pass 0 makes: a sentinel state here would
    // travel one lane per pass behind the correct states and keep the segment from converging
    if (a.err != NO_ERR) st = {(local + 1) * LB, 0, 0};
    o[3] = st.pos;
    o[4] = st.u;
    o[5] = st.k;
    o[6] = a.nblk;
    o[7] = a.dc0;
    o[8] = a.dc1;
    o[9] = a.dc2;
    o[10] = a.err;
    o[11] = 1;
}

// one workgroup per segment: convergence, prefixes over the lanes, segment status
__global__ __launch_bounds__(256) void jpeg_scan(Args A, const int32_t* __restrict__ lanes, int32_t* __restrict__ lscan, int32_t* __restrict__ segflag) {
    __shared__ int sh[4][256];
    __shared__ int flags;
    const int s = blockIdx.x, t = threadIdx.x;
    const int32_t* sr = A.segments + (long)s * ESVIT_JPEG_SEG_INTS;
    const int lane0 = sr[S_LANE0], nl = sr[S_NLANES];
    const int bpm = A.images[(long)sr[S_IMG] * ESVIT_JPEG_IMG_INTS + I_BPM];
    const int nblk_seg = sr[S_NMCU] * bpm;
    if (t == 0) flags = 0;
    __syncthreads();
    int carry[4] = {0, 0, 0, 0};
    int fl = 0;
    for (int base = 0; base < nl; base += 256) {
        const int j = base + t;
        const int32_t* L = lanes + (long)(lane0 + j) * LANE_INTS;
        int v[4] = {0, 0, 0, 0};
        if (j < nl) {
            v[0] = L[6];
            v[1] = L[7];
            v[2] = L[8];
            v[3] = L[9];
            fl |= L[11] ? 2 : 0;
        }
        int x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = v[q];
            sh[q][t] = x[q];
        }
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {  // inclusive Hillis-Steele scan
            int y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = t >= off ? sh[q][t - off] : 0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] += y[q];
                sh[q][t] = x[q];
            }
            __syncthreads();
        }
        if (j < nl) {
            const int g0 = carry[0] + x[0] - v[0];
            int32_t* o = lscan + (long)(lane0 + j) * 4;
            o[0] = g0;
            o[1] = carry[1] + x[1] - v[1];
            o[2] = carry[2] + x[2] - v[2];
            o[3] = carry[3] + x[3] - v[3];
            if (L[10] != NO_ERR && g0 + L[10] < nblk_seg) fl |= 1;  // a decode error inside a real block
            if (j == nl - 1) {
                const int total = g0 + v[0];
                if (total < nblk_seg || (total == nblk_seg && L[5] != 0)) fl |= 1;  // the segment ends before its last block does
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) carry[q] += sh[q][255];
        __syncthreads();
    }
    if (fl) atomicOr(&flags, fl);
    __syncthreads();
    if (t == 0) segflag[s] = flags;
}

__global__ __launch_bounds__(256) void jpeg_write(Args A, const int32_t* __restrict__ lanes, const int32_t* __restrict__ lscan,
                                                  const int32_t* __restrict__ segflag, int16_t* __restrict__ coef) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= A.n_lanes) return;
    const int s = A.lane_seg[j];
    if (segflag[s] & 2) return;  // not converged: jpeg_serial decodes this segment
    const int32_t* sr = A.segments + (long)s * ESVIT_JPEG_SEG_INTS;
    const int local = j - sr[S_LANE0];
    const int32_t* L = lanes + (long)j * LANE_INTS;
    const int32_t* P = lscan + (long)j * 4;
    State st = {L[0], L[1], L[2]};
    const int nbits = sr[S_BITS];
    const int end = min((local + 1) * LB, nbits);
    const Img m = load_img(A.images + (long)sr[S_IMG] * ESVIT_JPEG_IMG_INTS, A.huff);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(A.scan + sr[S_BYTE]);
    Acc a;
    run<true>(m, w, nbits, end, st, a, sr[S_MCU0], sr[S_NMCU] * m.bpm, P[0], P[1], P[2], P[3], coef, true);
}

__global__ __launch_bounds__(64) void jpeg_serial(Args A, int all, int32_t* __restrict__ segflag, int16_t* __restrict__ coef) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= A.n_segments) return;
    if (!all && !(segflag[s] & 2)) return;
    const int32_t* sr = A.segments + (long)s * ESVIT_JPEG_SEG_INTS;
    const int nbits = sr[S_BITS];
    const Img m = load_img(A.images + (long)sr[S_IMG] * ESVIT_JPEG_IMG_INTS, A.huff);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(A.scan + sr[S_BYTE]);
    const int nblk_seg = sr[S_NMCU] * m.bpm;
    State st = {0, 0, 0};
    Acc a;
    run<true>(m, w, nbits, nbits, st, a, sr[S_MCU0], nblk_seg, 0, 0, 0, 0, coef, true);
    const bool bad = (a.err != NO_ERR && a.err < nblk_seg) || a.nblk < nblk_seg || (a.nblk == nblk_seg && st.k != 0);
    segflag[s] = bad ? 1 : 0;
}

__global__ __launch_bounds__(256) void jpeg_status(Args A, const int32_t* __restrict__ segflag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_images) return;
    const int32_t* rec = A.images + (long)i * ESVIT_JPEG_IMG_INTS;
    int st = rec[I_HOST];
    if (rec[I_NCOMP] > 0)
        for (int s = rec[I_SEG0]; s < rec[I_SEG0] + rec[I_NSEG]; ++s) st |= segflag[s] & 1;
    A.status[i] = st;
}

// one thread per 8 x 8 block of image blockIdx.y: dequantise + islow IDCT -> its component plane (row pitch bw * 8)
__global__ __launch_bounds__(128) void jpeg_idct(Args A, const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
    const int32_t* rec = A.images + (long)blockIdx.y * ESVIT_JPEG_IMG_INTS;
    const int ncomp = rec[I_NCOMP];
    if (ncomp == 0) return;
    const int nblocks = rec[I_NBLOCKS];
    for (int b = blockIdx.x * 128 + threadIdx.x; b < nblocks; b += gridDim.x * 128) {
        int c = 0;
        if (ncomp == 3) c = b >= rec[I_COMP + C_INTS * 2 + C_BOFF] ? 2 : (b >= rec[I_COMP + C_INTS + C_BOFF] ? 1 : 0);
        const int32_t* cr = rec + I_COMP + C_INTS * c;
        const int local = b - cr[C_BOFF], bw = cr[C_BW];
        const int by = local / bw, bx = local - by * bw;
        const int16_t* src = coef + 64 * ((long)rec[I_BLOCK0] + b);
        int16_t cf[64];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int4 v = reinterpret_cast<const int4*>(src)[i];
            cf[8 * i + 0] = (int16_t)(v.x & 0xffff);
            cf[8 * i + 1] = (int16_t)((uint32_t)v.x >> 16);
            cf[8 * i + 2] = (int16_t)(v.y & 0xffff);
            cf[8 * i + 3] = (int16_t)((uint32_t)v.y >> 16);
            cf[8 * i + 4] = (int16_t)(v.z & 0xffff);
            cf[8 * i + 5] = (int16_t)((uint32_t)v.z >> 16);
            cf[8 * i + 6] = (int16_t)(v.w & 0xffff);
            cf[8 * i + 7] = (int16_t)((uint32_t)v.w >> 16);
        }
        int32_t q[64];
        const int32_t* qt = A.quant + 64 * (long)cr[C_Q];
#pragma unroll
        for (int i = 0; i < 64; ++i) q[i] = qt[i];
        uint8_t px[64];
        jpg::idct_islow(cf, q, px, 8);
        const int pitch = bw * 8;
        uint8_t* dst = planes + (long)rec[I_PLANE0] + cr[C_POFF] + (long)by * 8 * pitch + bx * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint2 v;
            v.x = px[8 * r] | (px[8 * r + 1] << 8) | (px[8 * r + 2] << 16) | ((uint32_t)px[8 * r + 3] << 24);
            v.y = px[8 * r + 4] | (px[8 * r + 5] << 8) | (px[8 * r + 6] << 16) | ((uint32_t)px[8 * r + 7] << 24);
            *reinterpret_cast<uint2*>(dst + (long)r * pitch) = v;
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_color(Args A, const uint8_t* __restrict__ planes) {
    const int i = blockIdx.y;
    const int32_t* rec = A.images + (long)i * ESVIT_JPEG_IMG_INTS;
    const int ncomp = rec[I_NCOMP];
    if (ncomp == 0) return;
    const int H = rec[I_H], W = rec[I_W], hmax = rec[I_HMAX], vmax = rec[I_VMAX];
    const uint8_t* base = planes + (long)rec[I_PLANE0];
    const int32_t* c0 = rec + I_COMP;
    const uint8_t* py = base + c0[C_POFF];
    const int pitch0 = c0[C_BW] * 8;
    uint8_t* out = A.out + A.table[3 * i];
    const long npx = (long)H * W;
    for (long p = blockIdx.x * 256 + threadIdx.x; p < npx; p += (long)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const int Y = py[(long)y * pitch0 + x];
        uint8_t rgb[3];
        if (ncomp == 1) {
            rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;  // Pillow's L -> RGB
        } else {
            const int32_t* c1 = rec + I_COMP + C_INTS;
            const int32_t* c2 = rec + I_COMP + 2 * C_INTS;
            const int rh = hmax / c1[C_H], rv = vmax / c1[C_V];
            const int cb = jpg::chroma(base + c1[C_POFF], c1[C_BW] * 8, c1[C_CW], c1[C_CH], rh, rv, x, y);
            const int cr = jpg::chroma(base + c2[C_POFF], c2[C_BW] * 8, c2[C_CW], c2[C_CH], rh, rv, x, y);
            jpg::ycc_to_rgb(Y, cb, cr, rgb);
        }
        uint8_t* o = out + 3 * p;
        o[0] = rgb[0];
        o[1] = rgb[1];
        o[2] = rgb[2];
    }
}

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Ws {
    int16_t* coef;
    uint8_t* planes;
    int32_t* lanes[2];
    int32_t* lscan;
    int32_t* segflag;
    size_t bytes;
};

Ws carve(void* base, int64_t blocks, int64_t plane_bytes, int64_t lanes, int64_t segs) {
    Ws w;
    size_t at = 0;
    char* b = static_cast<char*>(base);
    w.coef = reinterpret_cast<int16_t*>(b + at);
    at += align256((size_t)blocks * 128);
    w.planes = reinterpret_cast<uint8_t*>(b + at);
    at += align256((size_t)plane_bytes);
    for (int i = 0; i < 2; ++i) {
        w.lanes[i] = reinterpret_cast<int32_t*>(b + at);
        at += align256((size_t)lanes * LANE_INTS * 4);
    }
    w.lscan = reinterpret_cast<int32_t*>(b + at);
    at += align256((size_t)lanes * 16);
    w.segflag = reinterpret_cast<int32_t*>(b + at);
    at += align256((size_t)segs * 4 + 4);
    w.bytes = at;
    return w;
}

}  // namespace

int64_t esvit_i_jpeg_workspace(int64_t blocks, int64_t plane_bytes, int64_t lanes_segs) {
    const int64_t lanes = lanes_segs & 0xffffffff, segs = lanes_segs >> 32;
    if (blocks < 0 || plane_bytes < 0) return ESVIT_ERR_ARG;
    return (int64_t)carve(nullptr, blocks, plane_bytes, lanes, segs).bytes;
}

extern "C" int esvit_jpeg_decode(const esvit_jpeg_desc* d, void* workspace, size_t ws_bytes, esvit_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ESVIT_CHECK_ARG(d, "esvit_jpeg_decode: null descriptor");
    ESVIT_CHECK_ARG(d->n_images > 0 && d->n_images <= 65535 && d->n_segments >= 0 && d->n_lanes >= 0 && d->n_blocks >= 0 && d->plane_bytes >= 0,
                    "esvit_jpeg_decode: bad counts (%d images, %d segments, %d lanes, %d blocks)", d->n_images, d->n_segments, d->n_lanes,
                    d->n_blocks);
    ESVIT_CHECK_ARG(d->images && d->table && d->out && d->status, "esvit_jpeg_decode: null pointer");
    ESVIT_CHECK_ARG(d->n_segments == 0 || (d->segments && d->lane_seg && d->huff && d->quant && d->scan),
                    "esvit_jpeg_decode: null pointer");
    ESVIT_CHECK_ARG(d->mode == ESVIT_JPEG_PARALLEL || d->mode == ESVIT_JPEG_SERIAL, "esvit_jpeg_decode: mode %d", d->mode);
    ESVIT_CHECK_ARG(d->max_passes >= 0 && d->max_passes <= 64, "esvit_jpeg_decode: max_passes %d (0 = default, at most 64)", d->max_passes);
    ESVIT_CHECK_ARG(d->n_segments == 0 || d->n_lanes >= d->n_segments, "esvit_jpeg_decode: fewer lanes than segments");
    ESVIT_CHECK_ARG(((uintptr_t)d->scan & 3) == 0, "esvit_jpeg_decode: the scan data must be 4-byte aligned");
    const Ws w = carve(workspace, d->n_blocks, d->plane_bytes, d->n_lanes, d->n_segments);
    ESVIT_CHECK_ARG(workspace && ws_bytes >= w.bytes, "esvit_jpeg_decode: workspace of %zu bytes, %zu needed (ESVIT_Q_JPEG_WORKSPACE)", ws_bytes,
                    w.bytes);
    const int passes = d->max_passes > 0 ? d->max_passes : DEFAULT_PASSES;
    Args A = {d->images, d->segments, d->lane_seg, d->huff, d->quant, d->scan, d->table, d->out, d->status, d->n_images, d->n_segments, d->n_lanes};
    if (d->n_segments > 0) {
        if (hipMemsetAsync(w.coef, 0, (size_t)d->n_blocks * 128, stream) != hipSuccess) {
            esvit_set_error("esvit_jpeg_decode: hipMemsetAsync failed");
            return ESVIT_ERR_HIP;
        }
        const int lane_blocks = (d->n_lanes + 255) / 256;
        if (d->mode == ESVIT_JPEG_PARALLEL) {
            for (int p = 0; p < passes; ++p) {
                hipLaunchKernelGGL(jpeg_sync_pass, dim3(lane_blocks), dim3(256), 0, stream, A, p, w.lanes[(p + 1) & 1], w.lanes[p & 1]);
                ESVIT_CHECK_LAUNCH("jpeg_decode(sync)");
            }
            const int32_t* fin = w.lanes[(passes - 1) & 1];
            hipLaunchKernelGGL(jpeg_scan, dim3(d->n_segments), dim3(256), 0, stream, A, fin, w.lscan, w.segflag);
            ESVIT_CHECK_LAUNCH("jpeg_decode(scan)");
            hipLaunchKernelGGL(jpeg_write, dim3(lane_blocks), dim3(256), 0, stream, A, fin, w.lscan, w.segflag, w.coef);
            ESVIT_CHECK_LAUNCH("jpeg_decode(write)");
        }
        hipLaunchKernelGGL(jpeg_serial, dim3((d->n_segments + 63) / 64), dim3(64), 0, stream, A, d->mode == ESVIT_JPEG_SERIAL ? 1 : 0, w.segflag,
                           w.coef);
        ESVIT_CHECK_LAUNCH("jpeg_decode(serial)");
        hipLaunchKernelGGL(jpeg_idct, dim3(32, d->n_images), dim3(128), 0, stream, A, w.coef, w.planes);
        ESVIT_CHECK_LAUNCH("jpeg_decode(idct)");
        hipLaunchKernelGGL(jpeg_color, dim3(64, d->n_images), dim3(256), 0, stream, A, w.planes);
        ESVIT_CHECK_LAUNCH("jpeg_decode(color)");
    }
    hipLaunchKernelGGL(jpeg_status, dim3((d->n_images + 255) / 256), dim3(256), 0, stream, A, w.segflag);
    ESVIT_CHECK_LAUNCH("jpeg_decode(status)");
    return ESVIT_OK;
}
