// MFMA attention core for the path-level stages of two-stage configs with paths of 65..256 tokens (bf16, head_dim 32,
// non-causal): the first encoder stage (keys masked past the first EOS; padded with a length per sequence, or packed with
// seq_off) and the second decoder stage (padded, no key mask).  The 17..32-token kernel of attention_mfma.hip extended
// to tiles: one 256-thread workgroup per (sequence, head), its K / V slabs staged once in LDS as 32-key tiles (rows past
// the length zero-filled: 0 * garbage would be NaN in an MFMA), each wave owning 32-row query tiles (forward, backward
// pass A) or 32-row key tiles (backward pass B).  Every product is 2 x v_mfma_f32_32x32x16_bf16 per 32 x 32 tile:
//
//   forward   St = K Q^T -> lane (q = l&31, h2 = l>>5) holds S[q][key(r,h2)]; online softmax in fp32 over the key tiles,
//             O^T += V^T P~^T with P~ straight from the lane's own registers (the accumulator as the next B operand)
//   backward  pass A (query-stationary): sweep 1 recomputes m, l and D = rowsum(dO o O) = sum_j P dP~ online; sweep 2 forms
//             dS = P (dP~ - D) and dQ^T += K^T dS^T.  lse and D go to LDS for
//             pass B (key-stationary): S2 = Q K^T, dP2 = dO V^T -> lane (key, h2) holds [q(r,h2)][key];
//             dK^T += Q^T dS2, dV^T += dO^T P~2
//   with key(r,h2) = q(r,h2) = d(r,h2) = (r&3) + 8*(r>>2) + 4*h2  (the 32x32 MFMA C layout).
//
// lse and D are RECOMPUTED in the backward pass rather than kept from the forward one: the layer saves q|k|v and the head
// outputs only (functional.LayerFn, the same contract as every other attention route), the recomputation reads nothing
// from HBM that the backward pass does not stage anyway, and it costs 4 MFMAs per 32 x 32 tile.
// Dropout draws the element ids of every other attention kernel: row (b H + h) S + i with S the padded length in both
// layouts, key block j >> 5, attn_drop_key(.., j) (dsvg_common.h).
#include "mfma_frag.h"
#include "../../include/dsvg.h"

namespace {

constexpr int LT = 256;          // threads per workgroup
constexpr int NW = LT / 64;      // waves
constexpr int TLD = 40;          // LDS row stride (elements) of a 32-column slab: 80 bytes, 16-byte aligned rows
constexpr int MAX_S = 256;

// row_frag / col_frag (on a [..][TLD] slab: ld = TLD, col0 = 0) / pack_regs: mfma_frag.h
// lane holds v[r] = X[row][d = rowmap(r, h2)]: four 8-byte pieces of the row's 32 columns.  (Not stage_rows of mfma_frag.h on
// the row pointer: the compiler schedules the address of that form differently.)
__device__ __forceinline__ void store_rowmap(bf16_t* dst_row, int h2, const floatx16& v) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
        *reinterpret_cast<uint2*>(dst_row + 8 * c + 4 * h2) =
            make_uint2(f2bf_pk(v[4 * c + 0], v[4 * c + 1]), f2bf_pk(v[4 * c + 2], v[4 * c + 3]));
}
__device__ __forceinline__ void zero16(floatx16& v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
}

// rows [0, rows_pad) of one head's 32 columns -> LDS slab; rows >= n zero
__device__ __forceinline__ void stage32(bf16_t* dst, const bf16_t* __restrict__ src, long long ld, int n, int rows_pad) {
    for (int idx = threadIdx.x; idx < rows_pad * 4; idx += LT) {
        const int r = idx >> 2, c = idx & 3;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r < n) v = *reinterpret_cast<const uint4*>(src + (long long)r * ld + 8 * c);
        *reinterpret_cast<uint4*>(dst + r * TLD + 8 * c) = v;
    }
}
// packed layout: rows [first, total_rows) of one head's 32 columns <- 0
__device__ __forceinline__ void zero_rows(bf16_t* dst, long long ld, long long first, long long total_rows) {
    for (long long idx = threadIdx.x; idx < (total_rows - first) * 4; idx += LT)
        *reinterpret_cast<uint4*>(dst + (first + (idx >> 2)) * ld + 8 * (int)(idx & 3)) = make_uint4(0u, 0u, 0u, 0u);
}

// sequence b: first row, query rows, valid keys
template <bool PACKED>
__device__ __forceinline__ void seq_extent(int b, int S, const int32_t* lens, const int32_t* seq_off, long long& row0,
                                           int& nq, int& len) {
    if (PACKED) {
        row0 = seq_off[b];
        nq = len = min(seq_off[b + 1] - seq_off[b], S);      // (<= S by construction: LDS holds S32 rows)
    } else {
        row0 = (long long)b * S;
        nq = S;
        len = lens ? min(max(lens[b], 0), S) : S;
    }
}

template <bool PACKED>
__global__ __launch_bounds__(LT) void attn_long_mfma_fwd_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens,
                                                                const int32_t* __restrict__ seq_off, long long total_rows,
                                                                bf16_t* __restrict__ out, int S, int H, float scale,
                                                                float drop_p, uint32_t drop_site, const uint64_t* seed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int S32 = (S + 31) & ~31;
    bf16_t* Ks = reinterpret_cast<bf16_t*>(smem_raw);     // [S32][TLD]
    bf16_t* Vs = Ks + S32 * TLD;                          // [S32][TLD]
    const int b = blockIdx.x, h = blockIdx.y, d = H * 32;
    if (PACKED && b == (int)gridDim.x - 1) {
        zero_rows(out + h * 32, d, seq_off[b], total_rows);
        return;
    }
    long long row0;
    int nq, len;
    seq_extent<PACKED>(b, S, lens, seq_off, row0, nq, len);
    const int nkt = (len + 31) >> 5, nqt = (nq + 31) >> 5;
    const bf16_t* src = qkv + (size_t)row0 * 3 * d + h * 32;
    stage32(Ks, src + d, 3LL * d, len, nkt * 32);
    stage32(Vs, src + 2 * d, 3LL * d, len, nkt * 32);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, h2 = lane >> 5;
    const DropCtx dc = drop_make(drop_p, seed, drop_site);
    for (int qt = wave; qt < nqt; qt += NW) {
        const int qi = 32 * qt + li;
        const bf16_t* qrow = src + (size_t)min(qi, nq - 1) * 3 * d;
        Frag8 qf[2];
#pragma unroll
        for (int step = 0; step < 2; ++step) qf[step].u = *reinterpret_cast<const uint4*>(qrow + 16 * step + 8 * h2);
        const uint64_t drow = ((uint64_t)b * H + h) * S + qi;
        float m = -INFINITY, l = 0.f;
        floatx16 ot;
        zero16(ot);
        for (int kt = 0; kt < nkt; ++kt) {
            const bf16_t* kimg = Ks + kt * 32 * TLD;
            floatx16 st;
            zero16(st);
#pragma unroll
            for (int step = 0; step < 2; ++step)
                st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(kimg, TLD, li, 0, step, h2), qf[step].v, st, 0, 0, 0);
            // st[r] = q_qi . k_(32 kt + rowmap(r, h2))
            float p[16];
            float mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = (32 * kt + rowmap(r, h2) < len) ? st[r] * scale : -INFINITY;
                mt = fmaxf(mt, p[r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float mn = fmaxf(m, mt);          // finite: key 32 kt is valid
            const float corr = __expf(m - mn);
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = (p[r] == -INFINITY) ? 0.f : __expf(p[r] - mn);
                ls += p[r];
            }
            ls += __shfl_xor(ls, 32, 64);
            l = l * corr + ls;
            m = mn;
            if (dc.on) {
                const uint32_t hrow = attn_drop_row(dc, drow, (uint32_t)kt);
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r] *= attn_drop_key(dc, hrow, (uint32_t)(32 * kt + rowmap(r, h2)));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[r] *= corr;
            const bf16_t* vimg = Vs + kt * 32 * TLD;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(col_frag(vimg, TLD, 0, ks, lane), pack_regs(p, ks), ot, 0, 0, 0);
        }
        // ot[r] = O[q = qi][d = rowmap(r, h2)] (unnormalised)
        const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[r] *= inv;
        if (qi < nq) store_rowmap(out + ((size_t)row0 + qi) * d + h * 32, h2, ot);
    }
}

template <bool PACKED>
__global__ __launch_bounds__(LT) void attn_long_mfma_bwd_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens,
                                                                const int32_t* __restrict__ seq_off, long long total_rows,
                                                                const bf16_t* __restrict__ dout, bf16_t* __restrict__ dqkv,
                                                                int S, int H, float scale, float drop_p, uint32_t drop_site,
                                                                const uint64_t* seed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int S32 = (S + 31) & ~31;
    bf16_t* Qs = reinterpret_cast<bf16_t*>(smem_raw);     // [S32][TLD] each
    bf16_t* Ks = Qs + S32 * TLD;
    bf16_t* Vs = Ks + S32 * TLD;
    bf16_t* Gs = Vs + S32 * TLD;                          // dO
    float* lse_s = reinterpret_cast<float*>(Gs + S32 * TLD);
    float* D_s = lse_s + S32;
    const int b = blockIdx.x, h = blockIdx.y, d = H * 32;
    if (PACKED && b == (int)gridDim.x - 1) {
        for (int k = 0; k < 3; ++k) zero_rows(dqkv + k * d + h * 32, 3LL * d, seq_off[b], total_rows);
        return;
    }
    long long row0;
    int nq, len;
    seq_extent<PACKED>(b, S, lens, seq_off, row0, nq, len);
    const int nkt = (len + 31) >> 5, nqt = (nq + 31) >> 5;
    const bf16_t* src = qkv + (size_t)row0 * 3 * d + h * 32;
    stage32(Qs, src, 3LL * d, nq, nqt * 32);
    stage32(Ks, src + d, 3LL * d, len, nkt * 32);
    stage32(Vs, src + 2 * d, 3LL * d, len, nkt * 32);
    stage32(Gs, dout + (size_t)row0 * d + h * 32, (long long)d, nq, nqt * 32);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, h2 = lane >> 5;
    const DropCtx dc = drop_make(drop_p, seed, drop_site);
    const uint64_t hbase = ((uint64_t)b * H + h) * S;      // dropout row of query i = hbase + i
    bf16_t* dst = dqkv + (size_t)row0 * 3 * d + h * 32;

    // ---------------- pass A: lane = (query 32 qt + li, half h2), registers over keys ----------------------------
    for (int qt = wave; qt < nqt; qt += NW) {
        const int qi = 32 * qt + li;
        const bf16_t* qimg = Qs + qt * 32 * TLD;
        const bf16_t* gimg = Gs + qt * 32 * TLD;
        // sweep 1: m, l and D = sum_j P dP~ (online, rescaled with l)
        float m = -INFINITY, l = 0.f, dacc = 0.f;
        for (int kt = 0; kt < nkt; ++kt) {
            const bf16_t* kimg = Ks + kt * 32 * TLD;
            const bf16_t* vimg = Vs + kt * 32 * TLD;
            floatx16 st, dp;
            zero16(st);
            zero16(dp);
#pragma unroll
            for (int step = 0; step < 2; ++step) {
                st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(kimg, TLD, li, 0, step, h2), row_frag(qimg, TLD, li, 0, step, h2), st, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(vimg, TLD, li, 0, step, h2), row_frag(gimg, TLD, li, 0, step, h2), dp, 0, 0, 0);
            }
            float mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                st[r] = (32 * kt + rowmap(r, h2) < len) ? st[r] * scale : -INFINITY;
                mt = fmaxf(mt, st[r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float mn = fmaxf(m, mt);
            const float corr = __expf(m - mn);
            const uint32_t hrow = dc.on ? attn_drop_row(dc, hbase + qi, (uint32_t)kt) : 0u;
            float ls = 0.f, ds = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = (st[r] == -INFINITY) ? 0.f : __expf(st[r] - mn);
                ls += e;
                ds = fmaf(e, dp[r] * attn_drop_key(dc, hrow, (uint32_t)(32 * kt + rowmap(r, h2))), ds);
            }
            ls += __shfl_xor(ls, 32, 64);
            ds += __shfl_xor(ds, 32, 64);
            l = l * corr + ls;
            dacc = dacc * corr + ds;
            m = mn;
        }
        const float lse = l > 0.f ? m + __logf(l) : INFINITY;
        const float D = l > 0.f ? dacc / l : 0.f;
        // sweep 2: dS = P (dP~ - D) scale, dQ^T += K^T dS^T
        floatx16 dq;
        zero16(dq);
        for (int kt = 0; kt < nkt; ++kt) {
            const bf16_t* kimg = Ks + kt * 32 * TLD;
            const bf16_t* vimg = Vs + kt * 32 * TLD;
            floatx16 st, dp;
            zero16(st);
            zero16(dp);
#pragma unroll
            for (int step = 0; step < 2; ++step) {
                st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(kimg, TLD, li, 0, step, h2), row_frag(qimg, TLD, li, 0, step, h2), st, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(vimg, TLD, li, 0, step, h2), row_frag(gimg, TLD, li, 0, step, h2), dp, 0, 0, 0);
            }
            const uint32_t hrow = dc.on ? attn_drop_row(dc, hbase + qi, (uint32_t)kt) : 0u;
            float g[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * kt + rowmap(r, h2);
                const bool ok = key < len && qi < nq;
                const float p = ok ? __expf(st[r] * scale - lse) : 0.f;
                g[r] = ok ? p * (dp[r] * attn_drop_key(dc, hrow, (uint32_t)key) - D) * scale : 0.f;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                dq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(col_frag(kimg, TLD, 0, ks, lane), pack_regs(g, ks), dq, 0, 0, 0);
        }
        if (h2 == 0) {
            lse_s[qi] = lse;
            D_s[qi] = D;
        }
        if (qi < nq) store_rowmap(dst + (size_t)qi * 3 * d, h2, dq);
    }
    __syncthreads();

    // ---------------- pass B: lane = (key 32 kt + li, half h2), registers over queries ----------------------------
    // (key tiles past the length: their rows of dK / dV are zeros)
    for (int kt = wave; kt < nqt; kt += NW) {
        const int kj = 32 * kt + li;
        floatx16 dk, dv;
        zero16(dk);
        zero16(dv);
        if (kt < nkt) {
            const bf16_t* kimg = Ks + kt * 32 * TLD;
            const bf16_t* vimg = Vs + kt * 32 * TLD;
            const bool kvalid = kj < len;
            for (int qt = 0; qt < nqt; ++qt) {
                const bf16_t* qimg = Qs + qt * 32 * TLD;
                const bf16_t* gimg = Gs + qt * 32 * TLD;
                floatx16 s2, dp2;
                zero16(s2);
                zero16(dp2);
#pragma unroll
                for (int step = 0; step < 2; ++step) {
                    s2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(qimg, TLD, li, 0, step, h2), row_frag(kimg, TLD, li, 0, step, h2), s2, 0, 0, 0);
                    dp2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(gimg, TLD, li, 0, step, h2), row_frag(vimg, TLD, li, 0, step, h2), dp2, 0, 0, 0);
                }
                // s2[r] = q_(32 qt + rowmap(r, h2)) . k_kj
                float pv[16], gv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int q = 32 * qt + rowmap(r, h2);
                    const bool ok = kvalid && q < nq;
                    const float pr = ok ? __expf(s2[r] * scale - lse_s[q]) : 0.f;
                    const float mult = attn_drop_mult(dc, hbase + q, (uint32_t)kj);
                    pv[r] = pr * mult;                                          // P~ (as used by O = P~ V)
                    gv[r] = ok ? pr * (dp2[r] * mult - D_s[q]) * scale : 0.f;   // scale * dS[q][key]
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    dk = __builtin_amdgcn_mfma_f32_32x32x16_bf16(col_frag(qimg, TLD, 0, ks, lane), pack_regs(gv, ks), dk, 0, 0, 0);
                    dv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(col_frag(gimg, TLD, 0, ks, lane), pack_regs(pv, ks), dv, 0, 0, 0);
                }
            }
        }
        if (kj < nq) {
            store_rowmap(dst + (size_t)kj * 3 * d + d, h2, dk);
            store_rowmap(dst + (size_t)kj * 3 * d + 2 * d, h2, dv);
        }
    }
}

bool long_mfma_args_ok(const void* qkv, const int32_t* lens, const int32_t* seq_off, int64_t total_rows, int64_t n_seq,
                       int32_t S, int32_t n_heads) {
    return qkv && n_seq > 0 && n_seq < (1ll << 31) && S > 0 && S <= MAX_S && n_heads > 0 &&
           ((uintptr_t)qkv & 15) == 0 && (!seq_off || (!lens && total_rows > 0));
}

}  // namespace

extern "C" int dsvg_attention_long_mfma_fwd(const void* qkv, const int32_t* lens, const int32_t* seq_off, int64_t total_rows,
                                            void* out, int64_t n_seq, int32_t S, int32_t n_heads, float scale, float drop_p,
                                            uint32_t drop_site, const uint64_t* seed, void* stream) {
    DSVG_CHECK_ARG(long_mfma_args_ok(qkv, lens, seq_off, total_rows, n_seq, S, n_heads) && out && ((uintptr_t)out & 15) == 0,
                   "attention_long_mfma_fwd: bad args (S=%d, at most %d; lens and seq_off exclusive)", S, MAX_S);
    DSVG_CHECK_ARG(drop_p <= 0.f || seed, "attention_long_mfma_fwd: dropout needs a seed pointer");
    const size_t lds = (size_t)2 * ((S + 31) & ~31) * TLD * sizeof(bf16_t);
    const dim3 grid((unsigned)n_seq + (seq_off ? 1u : 0u), (unsigned)n_heads);
    auto kern = seq_off ? attn_long_mfma_fwd_kernel<true> : attn_long_mfma_fwd_kernel<false>;
    DSVG_ENSURE_LDS(kern, lds);
    hipLaunchKernelGGL(kern, grid, dim3(LT), lds, (hipStream_t)stream, (const bf16_t*)qkv, lens, seq_off, (long long)total_rows,
                       (bf16_t*)out, S, n_heads, scale, drop_p, drop_site, seed);
    DSVG_LAUNCH_CHECK("attention_long_mfma_fwd");
    return 0;
}

extern "C" int dsvg_attention_long_mfma_bwd(const void* qkv, const int32_t* lens, const int32_t* seq_off, int64_t total_rows,
                                            const void* dout, void* dqkv, int64_t n_seq, int32_t S, int32_t n_heads,
                                            float scale, float drop_p, uint32_t drop_site, const uint64_t* seed,
                                            void* stream) {
    DSVG_CHECK_ARG(long_mfma_args_ok(qkv, lens, seq_off, total_rows, n_seq, S, n_heads) && dout && dqkv &&
                   (((uintptr_t)dout | (uintptr_t)dqkv) & 15) == 0,
                   "attention_long_mfma_bwd: bad args (S=%d, at most %d; lens and seq_off exclusive)", S, MAX_S);
    DSVG_CHECK_ARG(drop_p <= 0.f || seed, "attention_long_mfma_bwd: dropout needs a seed pointer");
    const int S32 = (S + 31) & ~31;
    const size_t lds = (size_t)4 * S32 * TLD * sizeof(bf16_t) + (size_t)2 * S32 * sizeof(float);
    const dim3 grid((unsigned)n_seq + (seq_off ? 1u : 0u), (unsigned)n_heads);
    auto kern = seq_off ? attn_long_mfma_bwd_kernel<true> : attn_long_mfma_bwd_kernel<false>;
    DSVG_ENSURE_LDS(kern, lds);
    hipLaunchKernelGGL(kern, grid, dim3(LT), lds, (hipStream_t)stream, (const bf16_t*)qkv, lens, seq_off,
                       (long long)total_rows, (const bf16_t*)dout, (bf16_t*)dqkv, S, n_heads, scale, drop_p, drop_site, seed);
    DSVG_LAUNCH_CHECK("attention_long_mfma_bwd");
    return 0;
}
