// Scalar arithmetic of the JPEG decoder (jpeg.hip), restated from ITU-T T.81 and from the well-known algorithms of the
// Independent JPEG Group's 6b release that libjpeg(-turbo), and hence Pillow's default decode, still use:
//   - the accurate integer inverse DCT (jidctint.c, "islow": 13-bit constants, 2 pass-1 fraction bits) with the output
//     range limit of the post-IDCT table (a 10-bit wrap around the clamp, see idct_limit);
//   - "fancy" triangle-filter chroma upsampling (jdsample.c h2v1 / h2v2) with edge replication, and the plain replication
//     libjpeg falls back to when a downsampled row holds two samples or fewer;
//   - the fixed-point YCbCr -> RGB tables of jdcolor.c (16 fraction bits, rounding folded into the Cr/Cb terms).
// Plain C++ (JPG_HD expands to __host__ __device__ under hipcc and to nothing under a host compiler), so
// tests/test_jpeg_cpu.py compiles this header with g++ and checks it against the restatement in tests/jpeg_ref.py.
#pragma once
#include <stdint.h>

#ifndef JPG_HD
#define JPG_HD __host__ __device__ __forceinline__
#endif

namespace jpg {

// zig-zag index -> natural (row-major) index, T.81 Figure A.6
#ifdef __HIPCC__
__constant__
#endif
static const uint8_t kNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the post-IDCT range limit: index (v & 1023) of a table that is v + 128 on [-128, 127], 255 on [128, 511], 0 on [-512, -129],
// and repeats with period 1024 (a corrupt block wraps instead of saturating, as libjpeg's does)
JPG_HD int idct_limit(int v) {
    const int j = v & 1023;
    if (j < 128) return j + 128;
    if (j < 512) return 255;
    if (j < 896) return 0;
    return j - 896;
}

JPG_HD int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
              F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;

// one 8-point islow butterfly: in[0..7] (stride `is`) -> out[0..7] (stride `os`), descaled by `shift` with rounding
template <typename TIn, typename TOut, typename F>
JPG_HD void islow_1d(const TIn* in, int is, TOut* out, int os, int shift, F store) {
    int z2 = in[2 * is], z3 = in[6 * is];
    int z1 = (z2 + z3) * F0_541;
    const int tmp2 = z1 + z3 * (-F1_847);
    const int tmp3 = z1 + z2 * F0_765;
    z2 = in[0];
    z3 = in[4 * is];
    const int t0 = (z2 + z3) * (1 << CONST_BITS);
    const int t1 = (z2 - z3) * (1 << CONST_BITS);
    const int tmp10 = t0 + tmp3, tmp13 = t0 - tmp3, tmp11 = t1 + tmp2, tmp12 = t1 - tmp2;
    int o0 = in[7 * is], o1 = in[5 * is], o2 = in[3 * is], o3 = in[1 * is];
    z1 = o0 + o3;
    z2 = o1 + o2;
    z3 = o0 + o2;
    int z4 = o1 + o3;
    const int z5 = (z3 + z4) * F1_175;
    o0 *= F0_298;
    o1 *= F2_053;
    o2 *= F3_072;
    o3 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 *= -F1_961;
    z4 *= -F0_390;
    z3 += z5;
    z4 += z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    const int r = 1 << (shift - 1);
    out[0 * os] = store((tmp10 + o3 + r) >> shift);
    out[7 * os] = store((tmp10 - o3 + r) >> shift);
    out[1 * os] = store((tmp11 + o2 + r) >> shift);
    out[6 * os] = store((tmp11 - o2 + r) >> shift);
    out[2 * os] = store((tmp12 + o1 + r) >> shift);
    out[5 * os] = store((tmp12 - o1 + r) >> shift);
    out[3 * os] = store((tmp13 + o0 + r) >> shift);
    out[4 * os] = store((tmp13 - o0 + r) >> shift);
}

struct Ident {
    JPG_HD int operator()(int v) const { return v; }
};
struct Limit {
    JPG_HD uint8_t operator()(int v) const { return (uint8_t)idct_limit(v); }
};

// jidctint.c jpeg_idct_islow: coef int16 [64] natural order, q [64] natural order -> out 8 x 8 samples (row stride `stride`).
// 32-bit intermediates: exact for every block whose dequantised coefficients stay within what an encoder of 8-bit samples emits.
// (The zero-AC shortcuts of jidctint.c give the same values as the full butterflies, so they are not restated.)
JPG_HD void idct_islow(const int16_t* coef, const int32_t* q, uint8_t* out, int stride) {
    int deq[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) deq[i] = (int)coef[i] * q[i];
    int ws[64];
#pragma unroll
    for (int c = 0; c < 8; ++c) islow_1d(deq + c, 8, ws + c, 8, CONST_BITS - PASS1_BITS, Ident());
#pragma unroll
    for (int r = 0; r < 8; ++r) islow_1d(ws + 8 * r, 1, out + r * stride, 1, CONST_BITS + PASS1_BITS + 3, Limit());
}

// jdcolor.c ycc_rgb_convert (SCALEBITS = 16; FIX(x) = x * 65536 + 0.5)
JPG_HD void ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
    const int x = cr - 128, z = cb - 128;
    const int cr_r = (91881 * x + 32768) >> 16;                // FIX(1.40200)
    const int cb_b = (116130 * z + 32768) >> 16;               // FIX(1.77200)
    const int g = ((-22554) * z + 32768 + (-46802) * x) >> 16;  // FIX(0.34414), FIX(0.71414)
    rgb[0] = (uint8_t)clamp255(y + cr_r);
    rgb[1] = (uint8_t)clamp255(y + g);
    rgb[2] = (uint8_t)clamp255(y + cb_b);
}

// neighbour index for the triangle filter: output sample o of a 2x upsampled axis of n input samples takes input o / 2 and its
// neighbour on o's side, replicated at the edges
JPG_HD int up_near(int o) { return o >> 1; }
JPG_HD int up_far(int o, int n) {
    const int i = o >> 1;
    if (o & 1) return i + 1 < n ? i + 1 : i;
    return i > 0 ? i - 1 : 0;
}

// jdsample.c h2v1_fancy_upsample, output sample o of a row of n inputs (n > 2): (3 near + far + 1 or 2) >> 2
JPG_HD int fancy_h2v1(int near, int far, int o) { return (3 * near + far + 1 + (o & 1)) >> 2; }

// jdsample.c h2v2_fancy_upsample: column sums s = 3 * near row + far row; output (3 s_near + s_far + 8 or 7) >> 4
JPG_HD int fancy_h2v2(int s_near, int s_far, int o) { return (3 * s_near + s_far + 8 - (o & 1)) >> 4; }

// libjpeg's upsampled chroma sample at output pixel (x, y) from a component plane `p` (row pitch `pitch`; the downsampled image is
// cw x ch samples) upsampled by (rh, rv) in {(1, 1), (2, 1), (2, 2)}: jdsample.c fullsize / h2v1 / h2v2, fancy when the rows hold
// more than two samples, plain replication otherwise; the rows above the first and below the last are replications of them
JPG_HD int chroma(const uint8_t* p, int pitch, int cw, int ch, int rh, int rv, int x, int y) {
    if (rh == 1) return p[(long)y * pitch + x];
    if (cw <= 2) return p[(long)(rv == 2 ? y >> 1 : y) * pitch + (x >> 1)];
    const int xn = up_near(x), xf = up_far(x, cw);
    if (rv == 1) {
        const uint8_t* row = p + (long)y * pitch;
        return fancy_h2v1(row[xn], row[xf], x);
    }
    const uint8_t* rn = p + (long)up_near(y) * pitch;
    const uint8_t* rf = p + (long)up_far(y, ch) * pitch;
    return fancy_h2v2(3 * rn[xn] + rf[xn], 3 * rn[xf] + rf[xf], x);
}

}  // namespace jpg
