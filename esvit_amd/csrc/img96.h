// The [rows][96] bf16 LDS image of the persistent stage-0 backward kernels (mlp_fused_dw.hip, attn_tail_bwd.hip): 192-byte rows whose
// 16-byte units are XOR-ed with (row >> 2) inside aligned groups of four (fused16.h's image A), so that 16-byte fragment reads of 16
// consecutive rows and the transpose reads of 4-row blocks both spread over all banks.
#pragma once
#include "common.h"

// byte offset of channel ch of row `row`
__host__ __device__ constexpr int img_off(int row, int ch) {
    const int u = ch >> 3;
    return row * 192 + (((u & ~3) | ((u ^ (row >> 2)) & 3)) << 4) + ((ch & 7) << 1);
}

// The XOR sees (row >> 2) & 3 and the low two bits of the 16-byte unit only, hence: 16 rows further is +3072 bytes; 32 channels
// further is +64 bytes; of a 16-channel step only its parity reaches the XOR (two bases, 32 bytes apart under XOR).
constexpr int IMG_ROWS16 = 16 * 192, IMG_CH32 = 64;

// two transpose reads: element j / 4 + j of the result is image[row0 + j][col + (lane & 15)] / image[row1 + j][..] when lo / hi
// are the addresses of (row0 / row1 + ((lane & 15) >> 2), col + 4 * (lane & 3)) (mfma.h: frag_ks, frag_v_perm)
__device__ __forceinline__ bf16x8 tr_pair(const char* lo_p, const char* hi_p) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    typedef short s16x8_ __attribute__((ext_vector_type(8)));
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo_p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi_p);
    const s16x8_ both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, both);
}
