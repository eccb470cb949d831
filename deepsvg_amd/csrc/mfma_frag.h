// The operand-layout rules of v_mfma_f32_32x32x16_bf16 as this library uses it, stated once: the register unions, the
// accumulator row map, and the accessors between row-major bf16 images (LDS or global) and MFMA operands / results.
// Shared by the host-side weight packers (pack_images.h) and by every kernel that reads their images or hands an
// accumulator on as the next operand.
//
//   A / B operand: lane l supplies row (l & 31) of its matrix, K slots 8 (l >> 5) .. + 7 of the 16-wide K step (8 x bf16)
//   C / D result:  lane l holds column (l & 31), register r the row rowmap(r, l >> 5)
// Kernels compute TRANSPOSED tiles (weights or keys as A, tokens or queries as B), so a lane owns one token row and its
// 16 registers are that row's columns rowmap(r, h2).
#pragma once
#include "dsvg_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short shortx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

// address-space casts: an LDS pointer as a 32-bit LDS byte address / for the LDS builtins, a global pointer for LDS-DMA
#define DSVG_LDS_PTR(p) ((void __attribute__((address_space(3)))*)(p))
#define DSVG_GLB_PTR(p) ((const void __attribute__((address_space(1)))*)(p))

namespace {

// 8 x bf16 = one lane's share of an MFMA operand: as the operand, as two transposed-read halves, as a 16-byte word
union Frag8 {
    bf16x8 v;
    shortx4 h[2];
    uint4 u;
};

// the register order of a transposed 32 x 32 MFMA tile: value r of lane half h2 belongs to row / column rowmap(r, h2)
__host__ __device__ __forceinline__ int rowmap(int r, int h2) { return (r & 3) + 8 * (r >> 2) + 4 * h2; }

// bf16 <-> fp32 of one 16-byte piece
__device__ __forceinline__ void unpack8(const uint4& t, float (&v)[8]) {
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = __uint_as_float(w[e] << 16);
        v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
    }
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    return make_uint4(f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3]), f2bf_pk(v[4], v[5]), f2bf_pk(v[6], v[7]));
}

// B (or A) operand from a row-major image: row `row`, columns col0 + 16 step + 8 h2 .. + 7 - one 16-byte read, free of
// bank conflicts when the row stride is an odd number of 16-byte units
__device__ __forceinline__ bf16x8 row_frag(const bf16_t* img, int ld, int row, int col0, int step, int h2) {
    Frag8 f;
    f.u = *reinterpret_cast<const uint4*>(&img[row * ld + col0 + 16 * step + 8 * h2]);
    return f.v;
}
// A operand down the columns of an LDS image: A[i = column col0 + (lane & 31)][K slot e] = img[row rowmap(8 ks + e,
// lane >> 5)][that column] - two hardware-transposed 4 x 16 reads (ds_read_b64_tr_b16).  The K order is that of an
// accumulator's registers, so the other operand can be a pack_regs of the lane's own results.
__device__ __forceinline__ bf16x8 col_frag(const bf16_t* img, int ld, int col0, int ks, int lane) {
    const int g = lane >> 4, q16 = lane & 15;
    const int row = 16 * ks + 4 * (g >> 1) + (q16 >> 2);
    const int col = col0 + 16 * (g & 1) + 4 * (q16 & 3);
    Frag8 f;
    f.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(&img[row * ld + col]));
    f.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(&img[(row + 8) * ld + col]));
    return f.v;
}
// the accumulator as the next operand: registers 8 ks .. + 7 of a transposed tile = K slots rowmap(8 ks + e, h2)
__device__ __forceinline__ bf16x8 pack_regs(const float (&p)[16], int ks) {
    Frag8 f;
    f.u = make_uint4(f2bf_pk(p[8 * ks + 0], p[8 * ks + 1]), f2bf_pk(p[8 * ks + 2], p[8 * ks + 3]),
                     f2bf_pk(p[8 * ks + 4], p[8 * ks + 5]), f2bf_pk(p[8 * ks + 6], p[8 * ks + 7]));
    return f.v;
}
// a transposed 32 x 32 result tile (lane: row `row`, v[r] = column col0 + rowmap(r, h2)) -> four 8-byte pieces per lane;
// V is floatx16 or float[16]
template <typename V>
__device__ __forceinline__ void stage_rows(bf16_t* img, int ld, int row, int col0, int h2, const V& v) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint2 t;
        t.x = f2bf_pk(v[4 * c + 0], v[4 * c + 1]);
        t.y = f2bf_pk(v[4 * c + 2], v[4 * c + 3]);
        *reinterpret_cast<uint2*>(&img[row * ld + col0 + 8 * c + 4 * h2]) = t;
    }
}
// the lane's 16 values of such a tile, read back (bf16 -> fp32)
__device__ __forceinline__ void load_rows(const bf16_t* img, int ld, int row, int col0, int h2, float (&v)[16]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint2 t = *reinterpret_cast<const uint2*>(&img[row * ld + col0 + 8 * c + 4 * h2]);
        v[4 * c + 0] = __uint_as_float(t.x << 16); v[4 * c + 1] = __uint_as_float(t.x & 0xffff0000u);
        v[4 * c + 2] = __uint_as_float(t.y << 16); v[4 * c + 3] = __uint_as_float(t.y & 0xffff0000u);
    }
}
// rows [0, S) x `cols` columns of an LDS image -> global rows, 16 bytes per lane, by a whole 512-thread workgroup
__device__ __forceinline__ void store_image(bf16_t* dst, long long ld_dst, const bf16_t* img, int ld, int col0, int S, int cols) {
    const int cpr = cols / 8;
    for (int idx = threadIdx.x; idx < S * cpr; idx += 512) {
        const int r = idx / cpr, c = idx % cpr;
        *reinterpret_cast<uint4*>(dst + (long long)r * ld_dst + 8 * c) = *reinterpret_cast<const uint4*>(img + r * ld + col0 + 8 * c);
    }
}

}  // namespace
