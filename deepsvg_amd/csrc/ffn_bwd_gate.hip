// Fused-FFN backward: the gated input-gradient GEMM and the linear2 weight-gradient GEMM from ONE staging of their common
// operands.  For a 64-column block c of the 512 hidden units (fragment order) both products read the same two tiles:
//     dpre[rows, c] = (dym[rows, 0:256] . W2p[:, c]) gated by hp[rows, c] > 0, x gate_scale          (K = 256)
//     G2p[:, c]    += dym[rows, 0:256]^T . hp[rows, c],   db2 += colsum(dym[rows, :])                 (K = rows)
// Until now they were two launches (gemm_bf16_glds.hip: the EPI_GATE GEMM and a split-K EPI_PARTIAL GEMM) that each pulled
// dym and hp through L2 -> LDS; these LDS-DMA GEMMs are bound by exactly those bytes per CU.
//
// One workgroup of 8 waves per (column block c, row slice z), 8 x nsplit workgroups, all column blocks of a slice on one
// XCD (workgroup b runs on XCD b % 8) so that the slice's dym rows are fetched into that XCD's L2 once.  The workgroup walks
// its slice in 64-row tiles; a tile = dym [64][256] (two [64][128] images, 256-byte rows) + hp[:, c] [64][64] (128-byte
// rows), 40 KiB, LDS-DMA'd by all 8 waves into a 4-slot ring (three tiles in flight beside the one consumed): 160 KiB, all
// of the CU's LDS, one workgroup per CU.  W2p[:, c] ([256][64], 32 KiB) is row-invariant and read by the dpre waves only: it
// is requested up front into the ring's last slot, each dpre wave takes its 16 fragments (64 registers per lane) out of it
// once, and the slot then joins the ring.
//   waves 0-3: dpre - one 32x32 tile each (K = 256: dym rows by ds_read_b128, W2p columns by ds_read_b64_tr_b16, once), the
//              same MFMA sequence, operand order and epilogue as the EPI_GATE GEMM (bit-identical dpre); the gate is read from
//              the staged hp image instead of global memory.
//   waves 4-7: G2p - 64 dym features x the 64 columns each, accumulated across all tiles of the slice (both operands by
//              ds_read_b64_tr_b16 from the same images), + db2's row sums; the slice is written like the split-K GEMM's
//              (same slices, same per-slice order: bit-identical partials) and reduced by the deferred funnel.
// Every wave issues 5 of a tile's 40 DMA pieces and counts them (vmcnt).  The dpre waves' stores sit in the same counter and
// do not return in order with the loads, so their wait can only be longer than needed, never shorter.  Letting the four G2p
// waves, which store nothing inside the loop, issue all 40 pieces behind an exact count was measured and is slower (35.9
// against 31.2 us at 41,216 rows, 58.8 against 58.0 at 63,488: profiles/ffn_gate_dw2_ring_ab.log).
// Images: 256-byte rows: 16-byte chunk ch of row r at ch ^ (((r & 3) << 2) | ((r >> 2) & 3)) - conflict-free for the row
// reads and the transposed reads alike; 128-byte rows (read transposed only): ch ^ (((r >> 1) & 1) << 2).
// Rows past the slice's end (ragged row count, clamped on the load side) are zeroed in the G2p operand and not stored.
#include <stdlib.h>
#include "mfma_frag.h"
#include "../../include/dsvg.h"

namespace {

constexpr int GT = 64;                       // token rows per tile
constexpr int W2_BYTES = 256 * 64 * 2;       // W2p[:, c] image
constexpr int SLOT = (2 * 64 * 128 + 64 * 64) * 2;     // dym images + hp image of one tile (40 KiB)
constexpr int HP_OFF = 2 * 64 * 128 * 2;     // hp image inside a slot
constexpr int NSLOT = 4;
constexpr int W2_AT = (NSLOT - 1) * SLOT;    // the W2p image lands in the last slot, which tile NSLOT - 1 overwrites
constexpr int LDS_BYTES = NSLOT * SLOT;
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget of a CU");
static_assert(W2_BYTES <= SLOT, "the W2p image fits a slot");

__device__ __forceinline__ int sw256(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int sw128(int r) { return ((r >> 1) & 1) << 2; }

// LDS-DMA of consecutive 1 KiB pieces from inline asm (the waits are ours: counted vmcnt, see gemm_bf16_glds.hip dma_step8)
__device__ __forceinline__ void dma5(const char* s0, const char* s1, const char* s2, const char* s3, const char* s4,
                                     uint32_t lds) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %6\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, off\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %3, off\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, off\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %5, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "s"(lds)
        : "memory", "scc");
}
__device__ __forceinline__ void dma4(const char* s0, const char* s1, const char* s2, const char* s3, uint32_t lds) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %5\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, off\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %3, off\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(s0), "v"(s1), "v"(s2), "v"(s3), "s"(lds)
        : "memory", "scc");
}

__device__ __forceinline__ bf16x8 ld_tr(const char* img, uint32_t off0, uint32_t off1) {
    Frag8 f;
    f.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(img + off0));
    f.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(img + off1));
    return f.v;
}

// the lane's 8 k values are rows 8 h + e of a 16-row step: zero those at or past `lim`
__device__ __forceinline__ bf16x8 zero_from(const bf16x8& v, int lim) {
    Frag8 f;
    f.v = v;
    uint32_t w[4] = {f.u.x, f.u.y, f.u.z, f.u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = 2 * e >= lim ? 0u : (2 * e + 1 >= lim ? (w[e] & 0xffffu) : w[e]);
    f.u = make_uint4(w[0], w[1], w[2], w[3]);
    return f.v;
}

__device__ __forceinline__ float rowsum8(const bf16x8& f, float s) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    Frag8 t;
    t.v = f;
    const uint32_t w[4] = {t.u.x, t.u.y, t.u.z, t.u.w};
    const bf16x2 one = __builtin_bit_cast(bf16x2, 0x3f803f80u);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w[e]), one, s, false);
    return s;
}

__global__ __launch_bounds__(512, 1) void ffn_gate_dw2_kernel(const bf16_t* __restrict__ dym, const bf16_t* __restrict__ hp,
                                                               const bf16_t* __restrict__ w2p, float gate_scale,
                                                               bf16_t* __restrict__ dpre, int T, int k_chunk, int xcd_map,
                                                               float* __restrict__ part, int part_bf16) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int bid = (int)blockIdx.x;
    int c, z;
    if (xcd_map) { const int local = bid >> 3; c = local & 7; z = (local >> 3) * 8 + (bid & 7); }
    else { c = bid & 7; z = bid >> 3; }
    const int row_begin = z * k_chunk;
    const int row_end = min(T, row_begin + k_chunk);
    const int n_tiles = row_end > row_begin ? (row_end - row_begin + GT - 1) / GT : 0;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)DSVG_LDS_PTR(lds);

    // ---- LDS-DMA sources: wave w fills pieces 5 w .. 5 w + 4 of a slot (0-31: dym images, 32-39: hp image) -------------
    const char* src[5];
    int srow[5];
    long long sld[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int P = wave * 5 + i;
        if (P < 32) {
            const int r = 4 * (P & 15) + (lane >> 4);
            const int ch = (lane & 15) ^ sw256(r);
            src[i] = (const char*)dym + (size_t)(128 * (P >> 4) + 8 * ch) * 2;
            srow[i] = r;
            sld[i] = 256 * 2;
        } else {
            const int r = 8 * (P - 32) + (lane >> 3);
            const int ch = (lane & 7) ^ sw128(r);
            src[i] = (const char*)hp + (size_t)(64 * c + 8 * ch) * 2;
            srow[i] = r;
            sld[i] = 512 * 2;
        }
    }
    auto issue = [&](int s) {
        const int r0 = row_begin + s * GT;
        const char* a[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) a[i] = src[i] + (size_t)min(r0 + srow[i], T - 1) * sld[i];
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(s % NSLOT) * SLOT + (uint32_t)wave * 5 * 1024);
        dma5(a[0], a[1], a[2], a[3], a[4], dst);
    };
    // the wave's pieces of tile s landed: the tiles issued after it (up to NSLOT - 2 at this point) may stay in flight, 5
    // DMAs each (the dpre stores issued since only make this wait longer)
    auto wait_tile = [&](int s) {
        const int ahead = min(NSLOT - 2, n_tiles - 1 - s);
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    static_assert(NSLOT == 4, "wait_tile counts for a 4-slot ring");

    // ---- fragment offsets --------------------------------------------------------------------------------------------
    const int g = lane >> 4, q = lane & 15, qq = q >> 2, pp = q & 3;
    const bool p1 = wave < 4;               // wave-uniform role
    const int wm = (wave >> 1) & 1, wn = wave & 1;       // dpre waves: 32 x 32 tile (rows 32 wm, columns 32 wn)
    const int ww = wave & 3;                              // G2p waves: dym features 64 ww .. 64 ww + 63
    const int trow = 8 * (g >> 1) + qq;                   // row of a transposed read inside its 16-row step (+4: second)
    // dpre: dym row read (row r, chunk 2 (kk & 7) + h of image kk >> 3) and W2p transposed read (columns 32 wn ..)
    const int pr = 32 * wm + (lane & 31);
    const uint32_t w2_off = (uint32_t)(trow * 128 + 16 * ((4 * wn + 2 * (g & 1) + (pp >> 1)) ^ sw128(trow)) + 8 * (pp & 1));
    // G2p: dym transposed reads (features 32 it of the wave's 64) and hp transposed reads (columns 32 jn)
    uint32_t da_off[2][2], hb_off[2];
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int sc = 0; sc < 2; ++sc) {
            const int r = trow + 4 * sc;
            const int ch = 8 * (ww & 1) + 4 * it + 2 * (g & 1) + (pp >> 1);
            da_off[it][sc] = (uint32_t)((ww >> 1) * 16384 + r * 256 + 16 * (ch ^ sw256(r)) + 8 * (pp & 1));
        }
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
        hb_off[jn] = (uint32_t)(HP_OFF + trow * 128 + 16 * ((4 * jn + 2 * (g & 1) + (pp >> 1)) ^ sw128(trow)) + 8 * (pp & 1));

    floatx16 acc00, acc01, acc10, acc11;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc00[r] = 0.f; acc01[r] = 0.f; acc10[r] = 0.f; acc11[r] = 0.f; }
    // db2 (column block 0 only): the lane's k values of dym features (lane & 31) + 32 it; steps kk 0-1 and 2-3 in two chains
    // (the split-K GEMM's two waves per row block), added at the end in its order
    const bool do_rs = !p1 && c == 0;
    float rsa0 = 0.f, rsa1 = 0.f, rsb0 = 0.f, rsb1 = 0.f;

    // dpre waves: the wave's 16 W2p fragments (columns 32 wn .., k steps kk), read once from the image in the last slot
    Frag8 w2f[16];

    auto dpre_tile = [&](int s) {
        const char* slot = lds + (s % NSLOT) * SLOT;
        const int r0 = row_begin + s * GT;
        // dpre tile: acc = sum over kk of mfma(W2p columns, dym rows) - EPI_GATE's operand order and k order
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            Frag8 a;
            a.u = *reinterpret_cast<const uint4*>(slot + (kk >> 3) * 16384 + pr * 256 +
                                                  16 * ((2 * (kk & 7) + h) ^ sw256(pr)));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[kk].v, a.v, acc, 0, 0, 0);
        }
        // epilogue (gemm_bf16_glds.hip tile16, EPI_GATE): 16 consecutive columns of token row m per lane
        uint32_t x[4][4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int e = 0; e < 4; ++e) x[gq][e] = __float_as_uint(acc[4 * gq + e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            auto s01 = __builtin_amdgcn_permlane32_swap(x[0][e], x[1][e], false, false);
            auto s23 = __builtin_amdgcn_permlane32_swap(x[2][e], x[3][e], false, false);
            x[0][e] = s01[0]; x[1][e] = s01[1]; x[2][e] = s23[0]; x[3][e] = s23[1];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            auto s02 = __builtin_amdgcn_permlane32_swap(x[0][e], x[2][e], false, false);
            auto s13 = __builtin_amdgcn_permlane32_swap(x[1][e], x[3][e], false, false);
            x[0][e] = s02[0]; x[2][e] = s02[1]; x[1][e] = s13[0]; x[3][e] = s13[1];
        }
        uint4 pk[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = __uint_as_float(x[2 * cb][e]); v[4 + e] = __uint_as_float(x[2 * cb + 1][e]); }
            const uint4 gt = *reinterpret_cast<const uint4*>(slot + HP_OFF + pr * 128 +
                                                             16 * ((4 * wn + 2 * h + cb) ^ sw128(pr)));
            const uint32_t gw[4] = {gt.x, gt.y, gt.z, gt.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g0 = __uint_as_float(gw[e] << 16), g1 = __uint_as_float(gw[e] & 0xffff0000u);
                v[2 * e] = g0 > 0.f ? v[2 * e] * gate_scale : 0.f;
                v[2 * e + 1] = g1 > 0.f ? v[2 * e + 1] * gate_scale : 0.f;
            }
            pk[cb] = make_uint4(f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3]), f2bf_pk(v[4], v[5]), f2bf_pk(v[6], v[7]));
        }
        const int m = r0 + pr;
        if (m < row_end) {
            bf16_t* cp = dpre + (size_t)m * 512 + 64 * c + 32 * wn + 16 * h;
            *reinterpret_cast<uint4*>(cp) = pk[0];
            *reinterpret_cast<uint4*>(cp + 8) = pk[1];
        }
    };
    auto g2p_tile = [&](int s) {
        const char* slot = lds + (s % NSLOT) * SLOT;
        const int r0 = row_begin + s * GT;
        const bool ragged = r0 + GT > row_end;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            bf16x8 a0 = ld_tr(slot, da_off[0][0] + kk * 4096, da_off[0][1] + kk * 4096);
            bf16x8 a1 = ld_tr(slot, da_off[1][0] + kk * 4096, da_off[1][1] + kk * 4096);
            const bf16x8 b0 = ld_tr(slot, hb_off[0] + kk * 2048, hb_off[0] + kk * 2048 + 512);
            const bf16x8 b1 = ld_tr(slot, hb_off[1] + kk * 2048, hb_off[1] + kk * 2048 + 512);
            if (ragged) {
                const int lim = row_end - (r0 + 16 * kk + 8 * h);
                a0 = zero_from(a0, lim);
                a1 = zero_from(a1, lim);
            }
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b0, a0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b0, a1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b1, a0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b1, a1, acc11, 0, 0, 0);
            if (do_rs) {
                if (kk < 2) { rsa0 = rowsum8(a0, rsa0); rsa1 = rowsum8(a1, rsa1); }
                else { rsb0 = rowsum8(a0, rsb0); rsb1 = rowsum8(a1, rsb1); }
            }
        }
    };

    // DMA order of every wave: tile 0, the W2p image, tiles 1 .. NSLOT - 2, then one tile per iteration
    if (n_tiles > 0) {
        issue(0);
        // W2p[:, c] into the last slot: wave w fills pieces 4 w .. 4 w + 3 of the [256][64] image
        const char* a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 8 * (wave * 4 + i) + (lane >> 3);
            const int ch = (lane & 7) ^ sw128(r);
            a[i] = (const char*)w2p + ((size_t)r * 512 + 64 * c + 8 * ch) * 2;
        }
        dma4(a[0], a[1], a[2], a[3], __builtin_amdgcn_readfirstlane(lds0 + W2_AT + (uint32_t)wave * 4 * 1024));
        for (int s = 1; s < NSLOT - 1 && s < n_tiles; ++s) issue(s);
        wait_tile(0);                       // tile 0 and, issued before tile 1, the W2p image
        __builtin_amdgcn_s_barrier();       // the W2p image landed everywhere
    }
    // One loop per role: in a common loop the dpre waves' 64 fragment registers and the G2p waves' 64 accumulators are live
    // together and the kernel spills inside the loop.  Both loops pass the same barriers.
    if (p1) {
        if (n_tiles > 0) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) w2f[kk].v = ld_tr(lds + W2_AT, w2_off + kk * 2048, w2_off + kk * 2048 + 512);
            // in registers before the loop's first barrier hands the slot to tile NSLOT - 1
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        for (int s = 0; s < n_tiles; ++s) {
            wait_tile(s);
            __builtin_amdgcn_s_barrier();   // (as in the G2p waves' loop below)
            if (s + NSLOT - 1 < n_tiles) issue(s + NSLOT - 1);
            dpre_tile(s);
        }
        return;
    }
    for (int s = 0; s < n_tiles; ++s) {
        wait_tile(s);
        __builtin_amdgcn_s_barrier();       // tile s landed everywhere; everybody is done with tile s - 1's slot
        if (s + NSLOT - 1 < n_tiles) issue(s + NSLOT - 1);
        g2p_tile(s);
    }

    // ---- G2p slice z: rows = dym features (64 ww + 32 it + (lane & 31)), columns 64 c + 32 jn + ... -------------------
    const size_t slice = dsvg_splitk_slice(256, 512, true);
    float* my_part = part + (size_t)z * slice;
    const int mrow = 64 * ww + (lane & 31);
    const int ncol = 64 * c;
    auto put = [&](const floatx16& v, int jn, int im) {
        const int m = mrow + 32 * im;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int n = ncol + 32 * jn + 8 * gq + 4 * h;
            *reinterpret_cast<float4*>(my_part + (size_t)m * 512 + n) = make_float4(v[4 * gq], v[4 * gq + 1], v[4 * gq + 2], v[4 * gq + 3]);
        }
    };
    auto put_bf16 = [&](const floatx16& v, int jn, int im) {
        const int m = mrow + 32 * im;
        bf16_t* base = reinterpret_cast<bf16_t*>(my_part);
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            const uint32_t a0 = f2bf_pk(v[8 * gp + 0], v[8 * gp + 1]), a1 = f2bf_pk(v[8 * gp + 2], v[8 * gp + 3]);
            const uint32_t b0 = f2bf_pk(v[8 * gp + 4], v[8 * gp + 5]), b1 = f2bf_pk(v[8 * gp + 6], v[8 * gp + 7]);
            auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
            auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
            const int n = ncol + 32 * jn + 16 * gp + 8 * h;
            *reinterpret_cast<uint4*>(base + (size_t)m * 512 + n) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
        }
    };
    if (part_bf16) { put_bf16(acc00, 0, 0); put_bf16(acc01, 0, 1); put_bf16(acc10, 1, 0); put_bf16(acc11, 1, 1); }
    else { put(acc00, 0, 0); put(acc01, 0, 1); put(acc10, 1, 0); put(acc11, 1, 1); }
    if (do_rs) {
        rsa0 += __shfl_xor(rsa0, 32, 64);
        rsa1 += __shfl_xor(rsa1, 32, 64);
        rsb0 += __shfl_xor(rsb0, 32, 64);
        rsb1 += __shfl_xor(rsb1, 32, 64);
        if (h == 0) {
            float* rs = my_part + 256 * 512;
            rs[mrow] = rsa0 + rsb0;
            rs[mrow + 32] = rsa1 + rsb1;
        }
    }
}

}  // namespace

extern "C" int dsvg_ffn_gate_dw2(const void* dym, const void* hp, const void* w2p, float gate_scale, void* dpre,
                                 int64_t rows, int32_t split_k, float* g2p, float* db2, float* workspace,
                                 int64_t workspace_bytes, void* stream) {
    DSVG_CHECK_ARG(dym && hp && w2p && dpre && g2p && db2 && workspace, "ffn_gate_dw2: null operand");
    DSVG_CHECK_ARG(rows > 0 && rows < (1ll << 30) && split_k > 1, "ffn_gate_dw2: bad rows %lld / split_k %d",
                   (long long)rows, split_k);
    DSVG_CHECK_ARG(workspace_bytes >= dsvg_gemm_workspace_bytes(256, 512, split_k), "ffn_gate_dw2: workspace too small");
    DSVG_CHECK_ARG(!(((uintptr_t)dym | (uintptr_t)hp | (uintptr_t)w2p | (uintptr_t)dpre | (uintptr_t)workspace) & 15),
                   "ffn_gate_dw2: operands must be 16-byte aligned");
    static const bool pbf_on = !(getenv("DSVG_SPLITK_BF16") && atoi(getenv("DSVG_SPLITK_BF16")) == 0);   // as dsvg_gemm
    hipStream_t st = (hipStream_t)stream;
    const int T = (int)rows;
    // the split-K GEMM's slicing (dsvg_gemm): same row slices, same slice count, same slice format
    const int k_chunk = ((T + split_k - 1) / split_k + 63) / 64 * 64;
    int nsplit = (T + k_chunk - 1) / k_chunk;
    if ((split_k % 8) == 0) nsplit = split_k;       // trailing slices may be empty (they write zero partials)
    // bf16 slices where dsvg_gemm takes the LDS-DMA kernel (row count a multiple of 64), fp32 where it does not
    const int pbf = (pbf_on && (T % 64) == 0) ? 1 : 0;
    static bool once = false;
    if (!once) {
        (void)hipFuncSetAttribute((const void*)ffn_gate_dw2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        once = true;
    }
    hipLaunchKernelGGL(ffn_gate_dw2_kernel, dim3(8 * nsplit), dim3(512), LDS_BYTES, st, (const bf16_t*)dym,
                       (const bf16_t*)hp, (const bf16_t*)w2p, gate_scale, (bf16_t*)dpre, T, k_chunk,
                       (nsplit % 8) == 0 ? 1 : 0, workspace, pbf);
    DSVG_LAUNCH_CHECK("ffn_gate_dw2");
    const int64_t mn = 256 * 512;
    const int64_t slice = (int64_t)dsvg_splitk_slice(256, 512, true);
    int rc = pbf ? dsvg_reduce_partials_mixed(workspace, nsplit, slice, mn, mn, g2p, 0, st)
                 : dsvg_reduce_partials_strided(workspace, nsplit, slice, mn, g2p, 0, st);
    if (rc) return rc;
    return dsvg_reduce_partials_strided(workspace + mn, nsplit, slice, 256, db2, 0, st);
}
