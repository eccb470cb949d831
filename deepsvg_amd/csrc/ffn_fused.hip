// Fused FFN sub-block of the pre-LN transformer layers, d_model = 256, dim_feedforward = 512, bf16 storage, fp32
// accumulation and statistics:
//     y = x + drop_r( W2 . drop_h( relu( W1 . LN(x) + b1 ) ) + b2 )
// (deepsvg/model/layers/improved_transformer.py:51-53,138-140; the LayerNorm is norm2 of the same layer, :51,:138).
// One launch replaces LayerNorm + linear1 GEMM + linear2 GEMM: the normalised rows and the 512-wide hidden activations
// never leave the chip, HBM sees 512 B in + 512 B out per token (AI 512 FLOP/B, MFMA-bound).
//
// Structure (gfx950, 64-lane waves, v_mfma_f32_32x32x16_bf16):
//   * token-stationary waves: a 512-thread workgroup owns 256 token rows, each of its 8 waves 32 of them.  A wave keeps
//     its LayerNorm-ed rows as the B operands of GEMM 1 in registers for the whole kernel (16 fragments = 64 VGPRs) and the
//     transposed output tile y^T[256 x 32 tokens] in 8 accumulators (128 registers).
//   * the weights stream: the hidden dimension is cut into 16 chunks of 32 units; per chunk the workgroup needs
//     W1[32 c .. 32 c + 31, :] (16 KiB) and W2[:, 32 c .. 32 c + 31] (16 KiB).  dsvg_ffn_pack stores them once per
//     optimiser step as ready-made MFMA A fragments (1 KiB each: lane l's 16 bytes at l * 16), so a chunk is ONE
//     contiguous 32 KiB block that goes L2 -> LDS by LDS-DMA (global_load_lds_dwordx4, 4 pieces per wave) into a ring of
//     NBUF chunk slots, issued NBUF - 1 chunks ahead behind counted s_waitcnt vmcnt + one s_barrier per chunk, and every
//     fragment read is a conflict-free ds_read_b128 at `slot + fragment * 1024 + lane * 16` (one address register).
//     The DMA is issued from inline asm: hipcc drains vmcnt(0) before the next ds_read after a *builtin* LDS-DMA
//     (it cannot tell the ring slots apart), which would serialise the prefetch.
//   * GEMM 1 is issued transposed (D = W1_frag x X_frag): a lane then holds, for its token row (lane & 31), the hidden
//     units 8 q + 4 (lane >> 5) + e of the chunk - exactly a B-operand register image for GEMM 2 once packed to bf16, if
//     the K index of GEMM 2 is taken in that order.  dsvg_ffn_pack lays the W2 fragments out in the same K order, so
//     the hidden tile goes accumulator -> bias / ReLU / dropout -> bf16 -> MFMA operand without touching LDS.
//   * epilogue: two v_permlane32_swap rounds turn each 32 x 32 accumulator tile into 16 consecutive output columns per
//     lane; bias, dropout, residual and the bf16 stores (32 contiguous bytes per lane and tile) run from registers.
//   * dropout draws of the hidden site ("v2", private to the fused kernels): ONE counter hash per 16 consecutive elements
//     and a one-multiply finaliser per pair of 16-bit draws (0.75 v_mul_lo_u32 per element instead of 1.5), still 16-bit
//     thresholds (p = 0.1 -> 6554 / 65536).  The ids are taken in the order the lane owns them (tok * 512 + 32 c + 16
//     (lane >> 5) + r); the backward pass never re-draws them, it reads the gate off the stored h (h > 0 <=> the unit
//     passed the ReLU and was kept).  The residual site uses the library's standard draws (dsvg_drop_apply replays it).
#include "fused_common.h"
#include "pack_images.h"
#include "../../include/dsvg.h"

namespace {

constexpr int FD = 256;                 // d_model
constexpr int FF = 512;                 // dim_feedforward
constexpr int CH = 32;                  // hidden units per chunk
constexpr int NCH = FF / CH;            // 16
constexpr int FWD_CHUNK = 32 * FRAG;    // [W1 chunk: 16 fragments | W2 chunk: 16 fragments]
constexpr int BWD_CHUNK = 48 * FRAG;    // [W1 chunk | W2^T chunk | W1^T chunk]
constexpr int TOK_PER_WG = 256;

using dsvg_pack::hidden_of;         // hidden unit (inside its chunk) that K slot (ks2, half, e) of GEMM 2 carries
using dsvg_pack::frag_pos;          // position of hidden unit j in the fragment-ordered h / dpre matrices (an involution)
static_assert(dsvg_pack::D == FD && dsvg_pack::F == FF && dsvg_pack::FFN_CH == CH && dsvg_pack::FFN_FWD_CHUNK == FWD_CHUNK &&
              dsvg_pack::FFN_BWD_CHUNK == BWD_CHUNK && dsvg_pack::FRAG_BYTES == FRAG, "pack_images.h restates these");

// ---------------------------------------------------------------------------------------------------------------------
// weight packing: fp32 master parameters -> bf16 fragment-major chunk images (one thread per lane slot of 8 elements),
// the LayerNorm affine folded into linear1 (W1' = W1 diag(gamma), b1' = b1 + W1 beta): bodies in pack_images.h, which the
// one-launch refresh of a training step (dsvg_pack_images) shares
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ffn_pack_kernel(const float* __restrict__ flat, const int64_t* __restrict__ offs,
                                                       int n_layers, bf16_t* __restrict__ fwd, bf16_t* __restrict__ bwd) {
    dsvg_pack::ffn_slot((long long)blockIdx.x * 256 + threadIdx.x, flat, offs, n_layers, fwd, bwd);
}
__global__ __launch_bounds__(256) void ffn_w2p_kernel(const float* __restrict__ flat, const int64_t* __restrict__ offs,
                                                      int n_layers, bf16_t* __restrict__ w2p) {
    dsvg_pack::ffn_w2p_slot((long long)blockIdx.x * 256 + threadIdx.x, flat, offs, n_layers, w2p);
}
__global__ __launch_bounds__(256) void ffn_fold_bias_kernel(const float* __restrict__ flat, const int64_t* __restrict__ offs,
                                                            int n_layers, float* __restrict__ b1f) {
    dsvg_pack::ffn_fold_bias_row(blockIdx.x * 4 + (threadIdx.x >> 6), threadIdx.x & 63, flat, offs, n_layers, b1f);
}

// ---------------------------------------------------------------------------------------------------------------------
// dropout draws, scheme v2 (see the header): group of 16 consecutive ids, word i = two 16-bit draws (slots 2 i, 2 i + 1)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t drop2_group(const DropCtx& c, uint64_t g16) {
    const uint32_t h = dsvg_hash32((uint32_t)g16 ^ c.s0);
    return (h ^ c.s1) + (uint32_t)(g16 >> 32) * 0x9e3779b1u;
}
__device__ __forceinline__ uint32_t drop2_word(uint32_t h, uint32_t i) { return drop_word(h, i); }   // (dsvg_common.h)
// multipliers of the 8 ids 16 g16 + 8 hi .. + 7 (hi = 0, 1) given the group hash
__device__ __forceinline__ void drop2_mult8(const DropCtx& c, uint32_t h, int hi, float (&m)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = drop2_word(h, 4 * hi + i);
        m[2 * i] = (w & 0xffffu) < c.thresh ? 0.f : c.scale;
        m[2 * i + 1] = (w >> 16) < c.thresh ? 0.f : c.scale;
    }
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));

// Activation of a hidden tile on PACKED pairs (round 5; 5.5 instructions per pair instead of 19): the 16 accumulator values
// of a lane -> the two B-operand fragments of G2.
//   scale (v_pk_mul_f32) -> bf16 pair (v_cvt_pk_bf16_f32) -> ReLU as a signed 16-bit maximum with 0 (v_pk_max_i16: a negative
//   bf16 is a negative int16) -> dropout: word k of the lane's group hash holds the draws of elements 2 k (low half) and
//   2 k + 1, drop when draw < thresh: r = sat(thresh - draw) is 0 for a kept element, else 0 - r >= 65536 - thresh >= 0x8000
//   exceeds every non-negative bf16 pattern (thresh <= 32768: dropout rates up to 0.5, checked by the host), so one more
//   saturating subtraction clears exactly the dropped halves (2 x v_pk_sub_u16 clamp + v_pk_sub_u16).
// The same draws as drop2_mult8 (ids in lane order); the scale is applied before instead of after the ReLU: results differ
// from the scalar form by fp32 rounding order only.
// bs: the lane's 16 bias values ALREADY MULTIPLIED BY THE SCALE, element 4 q + e at bs[8 q + e] (LDS): the
// token-stationary kernels start their hidden accumulator from zero (an initial value would be 16 more live registers under
// G2) and add the bias here, fused with the scale: v_pk_fma_f32.
__device__ __forceinline__ void ffn_act_packed(const float (&v)[16], const DropCtx& dh, uint32_t hh, uint32_t (&pk)[8],
                                               const float* bs) {
    const f2 sc2 = {dh.scale, dh.scale};
    const s16x2 zero = {0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 bb = *reinterpret_cast<const float4*>(bs + 8 * q);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = 2 * q + j;
            const f2 a = __builtin_elementwise_fma(f2{v[2 * k], v[2 * k + 1]}, sc2, j ? f2{bb.z, bb.w} : f2{bb.x, bb.y});
            pk[k] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, f2bf_pk(a[0], a[1])), zero));
        }
    }
    if (dh.on) {
        const u16x2 tpair = {(unsigned short)dh.thresh, (unsigned short)dh.thresh};
        const u16x2 z = {0, 0};
        // (stage by stage over the 8 words, not word by word: back-to-back dependent packed operations cost a wait state each)
        u16x2 r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = __builtin_bit_cast(u16x2, drop2_word(hh, k));
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = __builtin_elementwise_sub_sat(tpair, r[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = z - r[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) pk[k] = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, pk[k]), r[k]));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
// Schedule of the chunk loop (per workgroup; `sync(k)` = s_waitcnt vmcnt(0) + s_barrier + DMA issue of chunk k + 2):
//   * DMA runs two chunks ahead: after sync(k) chunks <= k + 1 are in LDS, chunk k + 2 is in flight into the slot chunk
//     k - 1 has left (NBUF = 3), so fragment reads may run ahead into the next chunk without waiting for anything.
//   * the two waves of a SIMD (w, w + 4) run the same three stages G1 (16 dependent MFMAs: hidden tile), E1 (VALU:
//     bias / ReLU / dropout / bf16) and G2 (16 MFMAs into the 8 output accumulators) one stage apart:
//        waves 0-3:  sync(c) | G1(c)   E1(c)     G2(c)
//        waves 4-7:  sync(c) | G2(c)   G1(c + 1) E1(c + 1)         (same code, their barrier sits before G2)
//     so every VALU stage of one wave sits beside an MFMA stage of its partner instead of beside the partner's VALU
//     stage (waves that leave a barrier together otherwise stay in lockstep and the matrix pipe idles during E1).
//     (tried in round 3, both without effect on the 52 us of a 65,536-row inference launch: the barrier of waves 4-7 between
//     the two halves of E1 - half a period apart instead of a stage - and two accumulator chains in G1, which cost 16
//     registers and with them in-loop spills: 60 us)
//   * A fragments go through a 4-deep register ring that is refilled right behind each MFMA (prefetch distance 4 MFMAs,
//     continuous across stages and chunks): ds_read latency is covered by the wave's own MFMAs, not only by its partner.
//   * TRAIN: the kernel also hands the unfused backward what it needs - h (bf16 [T, 512], hidden columns in FRAGMENT
//     ORDER: position 32 c + 16 s + 8 b + 4 a + e holds unit 32 c + 16 s + 8 a + 4 b + e, i.e. exactly the 8 values a
//     lane owns per K step: one aligned 16-byte store each), xh = (x - mean) * rstd (bf16) and rstd (fp32).  vmcnt
//     counts stores too, out of order with respect to loads, so the only safe DMA wait is vmcnt(0); the h stores of a
//     chunk are therefore held back in 8 registers and issued right BEHIND the next sync point, which gives them (and
//     the DMA) a whole iteration to drain before the next wait.
// development probe (dsvg_ffn_debug_clock): when set, wave `w` of every workgroup stores s_memtime at four points - kernel
// start, LayerNorm done (first chunk sync ahead), chunk loop done, last store issued - into dbg[(block * 8 + w) * 4 ..]
// (bit 0 of the buffer address set: s_memrealtime - the constant 100 MHz reference counter, ONE time base for the whole chip, so
// that start / end stamps of different workgroups can be compared: dispatch ramp and tail of a launch - instead of s_memtime,
// the shader clock (one counter per XCD: only differences inside a wave mean anything))
__device__ __forceinline__ void ffn_stamp(unsigned long long* d, int slot) {
    if (d && (threadIdx.x & 63) == 0) {
        const bool real = (reinterpret_cast<uintptr_t>(d) & 1) != 0;
        // (an explicit GLOBAL pointer: the integer round trip would make this a flat_store, and a flat operation pending in
        // vmcnt - these waves never wait on it - turns every LDS wait of the kernel into lgkmcnt(0), LLVM SIInsertWaitcnts)
        typedef unsigned long long __attribute__((address_space(1))) * gptr_t;
        gptr_t b = (gptr_t)(reinterpret_cast<uintptr_t>(d) & ~(uintptr_t)1);
        b[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 4 + slot] = real ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();
    }
}

// development probe of ffn_bwd_dx_kernel (dsvg_ffn_debug_clock with bit 1 of the buffer address set; scripts/ffn_bwd_dx_probe.py): 8
// stamps of the chip-wide 100 MHz counter per wave - start, first chunk ready, K loop done, x rows landed + statistics, LayerNorm
// math done, residual rows landed, stores issued, masked pass done
__device__ __forceinline__ void bwd_stamp(unsigned long long* d, int slot) {
    if (d && (threadIdx.x & 63) == 0) {
        typedef unsigned long long __attribute__((address_space(1))) * gptr_t;
        gptr_t b = (gptr_t)(reinterpret_cast<uintptr_t>(d) & ~(uintptr_t)3);
        b[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + slot] = __builtin_amdgcn_s_memrealtime();
    }
}

// The wave's 32 rows, one row per lane pair (lane half h owns the columns 16 ks + 8 h .. + 7 of every K step): LayerNorm
// without the affine part (folded into W1' / b1') -> the 16 B-operand fragments xf; TRAIN also stores xh and rstd.
// The statistics come from the packed words (ln_stats_packed, fused_common.h: the prologue is instruction-issue-bound).
// Called between the row loads and the first use of b1 / b2 (__syncthreads).
template <bool TRAIN>
__device__ __forceinline__ void ffn_ln_rows(const bf16_t* __restrict__ x, int my_row, int half, bool st,
                                            bf16_t* __restrict__ xh_out, float* __restrict__ rstd_out, float eps,
                                            bf16x8 (&xf)[16]) {
    const char* xr = reinterpret_cast<const char*>(x) + (size_t)my_row * (FD * 2) + half * 16;
    uint4 raw[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) raw[ks] = *reinterpret_cast<const uint4*>(xr + 32 * ks);
    __syncthreads();            // b1 / b2 staged (the row loads above are in flight meanwhile)
    float s, q, mean, rstd;
    ln_stats_packed(raw, s, q);
    ln_mean_rstd256(s, q, eps, mean, rstd);
    const float shift = -mean * rstd;
    char* xo = TRAIN ? reinterpret_cast<char*>(xh_out) + (size_t)my_row * (FD * 2) + half * 16 : nullptr;
    if (TRAIN && st && half == 0 && rstd_out) rstd_out[my_row] = rstd;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {       // (gamma / beta live in the packed W1' / b1', see ffn_pack_kernel)
        float v[8];
        unpack8(raw[ks], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], rstd, shift);
        Frag8 f;
        f.u = pack8(v);
        xf[ks] = f.v;
        if (TRAIN && st) *reinterpret_cast<uint4*>(xo + 32 * ks) = f.u;
    }
}

template <int NBUF, bool TRAIN, bool PK>
__global__ __launch_bounds__(512, 2) void ffn_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ img,
                                                         const float* __restrict__ b1, const float* __restrict__ b2,
                                                         bf16_t* __restrict__ y, bf16_t* __restrict__ h_out,
                                                         bf16_t* __restrict__ xh_out, float* __restrict__ rstd_out,
                                                         int M, float eps, float drop_p,
                                                         const uint64_t* __restrict__ seed, uint32_t site_h,
                                                         uint32_t site_r, int n_chunks, unsigned long long* dbg, int warm) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];      // [NBUF chunk slots | b1 (2 KiB) | b2 (1 KiB)]
    ffn_stamp(dbg, 0);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool late = wave >= 4;
    const int tok = lane & 31, half = lane >> 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)DSVG_LDS_PTR(smem);
    float* sb1 = reinterpret_cast<float*>(smem + NBUF * FWD_CHUNK);
    float* sb2 = sb1 + FF;

    // ---- weight stream: this wave moves pieces 4 wave .. 4 wave + 3 of every chunk -----------------------------------
    const char* my_src = reinterpret_cast<const char*>(img) + wave * 4096;         // (wave-uniform; + lane * 16 per lane)
    const uint32_t my_dst = __builtin_amdgcn_readfirstlane(lds0 + wave * 4096);
    auto issue = [&](int c) { dma4s(my_src + (size_t)c * FWD_CHUNK, (uint32_t)lane * 16u, my_dst + (uint32_t)(c % NBUF) * FWD_CHUNK); };
    // DMA distance: DIST = NBUF - 1 chunks ahead of the compute (NBUF = 3: 2, NBUF = 4: 3)
    constexpr int DIST = NBUF - 1;
    // Round 6: the layer's chunk image (512 KiB) is cold in this XCD's L2 when the launch starts (inside a training step every
    // layer's image is touched once per step) and the workgroups walk it in lockstep: every chunk would begin with one HBM miss
    // that all of them wait for.  So the workgroups of an XCD (block b runs on XCD b % 8) request the chunks behind the first
    // DIST up front, one each: an ordinary chunk DMA into the ring's last slot - this wave's own pieces of it, which its
    // own, later DMA of chunk DIST overwrites in order; nobody reads the slot before that one has landed.
    if (warm && NBUF == 4 && n_chunks > DIST) {
        const int wc = DIST + (int)((blockIdx.x >> 3) % (unsigned)(n_chunks - DIST));
        dma4s(my_src + (size_t)wc * FWD_CHUNK, (uint32_t)lane * 16u, my_dst + (uint32_t)DIST * FWD_CHUNK);
    }
#pragma unroll
    for (int c = 0; c < DIST; ++c)
        if (c < n_chunks) issue(c);

    // (PK: b1' is staged multiplied by the dropout scale, see ffn_act_packed)
    sb1[tid] = PK ? b1[tid] * drop_make(drop_p, seed, site_h).scale : b1[tid];
    if (tid < FD) sb2[tid] = b2[tid];

    // ---- the wave's 32 rows: LayerNorm in registers -> 16 B-operand fragments ------------------------------------------
    const int row0 = blockIdx.x * TOK_PER_WG + wave * 32;
    const int my_row = min(row0 + tok, M - 1);          // rows past M are computed on a clamped copy, never stored
    bf16x8 xf[16];
    ffn_ln_rows<TRAIN>(x, my_row, half, TRAIN && row0 + tok < M, xh_out, rstd_out, eps, xf);
    __builtin_amdgcn_sched_barrier(0);      // (the 128 accumulator zeroes below must not be hoisted above the LayerNorm)

    const DropCtx dh = drop_make(drop_p, seed, site_h);
    const DropCtx dr = drop_make(drop_p, seed, site_r);

    floatx16 yacc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) yacc[t][r] = 0.f;
    floatx16 hid;
    bf16x8 hf[2];
    uint4 ring[4];

    const char* lbase = smem + lane * 16;
    auto slot_of = [&](int c) -> const char* { return lbase + (c % NBUF) * FWD_CHUNK; };
    auto ld = [&](const char* p) -> uint4 { return *reinterpret_cast<const uint4*>(p); };

    // sync(k): afterwards chunks <= k + 1 are readable (this wave's pieces: counted vmcnt, the others': the barrier) and
    // chunk k + DIST is on its way into the slot chunk k - 1 has left; with NBUF = 4 chunk k + 2 stays in flight across
    // the barrier (4 pieces per wave and chunk)
    uint4 stash[2];                 // TRAIN: the packed h chunk waiting for its store slot
    int stash_c = -1;
    char* hrow = TRAIN ? reinterpret_cast<char*>(h_out) + (size_t)my_row * (FF * 2) + half * 16 : nullptr;
    const bool hst = TRAIN && row0 + tok < M;
    auto flush = [&]() {
        if (TRAIN && stash_c >= 0) {
            if (hst) {
                *reinterpret_cast<uint4*>(hrow + (CH * stash_c) * 2) = stash[0];
                *reinterpret_cast<uint4*>(hrow + (CH * stash_c + 16) * 2) = stash[1];
            }
            stash_c = -1;
        }
    };
    auto sync = [&](int k) {
        // (TRAIN: the h stores behind each sync are in flight too.  Loads return in order, so "at most 4 outstanding" still
        // means chunk k + 1 - older than the 4 DMA loads of chunk k + 2 - has landed; with the 3-slot ring there is no
        // younger load to count on and every sync has to drain the stores as well)
        if (DIST == 3 && k + 2 < n_chunks) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (k + DIST < n_chunks) issue(k + DIST);
        flush();
    };
    // G1: hid[unit][token] = sum_k W1[32 c + unit][k] xn[token][k]; the ring runs on into `cont` (4 more fragments)
    auto g2frag = [](int p) -> int { return 2 * (p & 7) + (p >> 3); };      // G2 position -> fragment of the W2 chunk
    auto G1 = [&](const char* w1, const char* cont) {
#pragma unroll
        for (int r = 0; r < 16; ++r) hid[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            Frag8 a;
            a.u = ring[ks & 3];
            hid = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, xf[ks], hid, 0, 0, 0);
            if (ks + 4 < 16) ring[ks & 3] = ld(w1 + (ks + 4) * FRAG);
            else if (cont) ring[ks & 3] = ld(cont + g2frag(ks + 4 - 16) * FRAG);
            __builtin_amdgcn_sched_barrier(0);      // keep "MFMA n, refill slot n" order: hipcc otherwise sinks every read
        }                                           // to just before its MFMA (prefetch distance 0)
    };
    // E1: bias, ReLU, dropout (ids tok * 512 + 32 c + 16 half + r), bf16 -> the two K steps of G2's B operand
    auto E1 = [&](int c) {
        const uint64_t id0 = (uint64_t)(row0 + tok) * FF + (uint32_t)(CH * c + 16 * half);
        const uint32_t hh = dh.on ? drop2_group(dh, id0 >> 4) : 0u;
        if (PK) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = hid[r];
            uint32_t pk[8];
            ffn_act_packed(v, dh, hh, pk, sb1 + CH * c + 4 * half);
            Frag8 f0, f1;
            f0.u = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            f1.u = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            hf[0] = f0.v; hf[1] = f1.v;
            if (TRAIN) { stash[0] = f0.u; stash[1] = f1.u; stash_c = c; }
            return;
        }
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
            float v[8];
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
                const int q = 2 * ks2 + qq;
                const float4 bb = *reinterpret_cast<const float4*>(sb1 + CH * c + 8 * q + 4 * half);
                v[4 * qq + 0] = fmaxf(hid[4 * q + 0] + bb.x, 0.f);
                v[4 * qq + 1] = fmaxf(hid[4 * q + 1] + bb.y, 0.f);
                v[4 * qq + 2] = fmaxf(hid[4 * q + 2] + bb.z, 0.f);
                v[4 * qq + 3] = fmaxf(hid[4 * q + 3] + bb.w, 0.f);
            }
            if (dh.on) {
                float m[8];
                drop2_mult8(dh, hh, ks2, m);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= m[e];
            }
            Frag8 f;
            f.u = pack8(v);
            hf[ks2] = f.v;
            if (TRAIN) stash[ks2] = f.u;
        }
        if (TRAIN) stash_c = c;
    };
    // G2: y[out][token] += sum_unit W2[out][32 c + unit] hid[unit][token]; the ring runs on into `cont`
    auto G2 = [&](const char* w2, const char* cont) {
        // position n: output tile n & 7, K step n >> 3 (fragment 2 (n & 7) + (n >> 3) of the packed chunk): the two MFMAs of
        // an accumulator are 8 apart instead of adjacent with a ring refill between them
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            Frag8 a;
            a.u = ring[n & 3];
            yacc[n & 7] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, hf[n >> 3], yacc[n & 7], 0, 0, 0);
            if (n + 4 < 16) ring[n & 3] = ld(w2 + g2frag(n + 4) * FRAG);
            else if (cont) ring[n & 3] = ld(cont + (n + 4 - 16) * FRAG);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // ---- the chunk loop ---------------------------------------------------------------------------------------------------
    // Both wave groups run the SAME straight-line code G1 E1 G2 per chunk; only the position of their one barrier per
    // chunk differs (before G1 for waves 0-3, before G2 for waves 4-7), which holds waves 4-7 one stage (G1 + E1) ahead.
    ffn_stamp(dbg, 1);
    if (n_chunks > 0) {
        if (DIST == 3 && n_chunks > 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();           // chunks 0 and 1 are in LDS
        {
            const char* s0 = slot_of(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) ring[i] = ld(s0 + i * FRAG);
        }
        for (int c = 0; c < n_chunks; ++c) {
            const char* sc = slot_of(c);
            const char* sn = (c + 1 < n_chunks) ? slot_of(c + 1) : nullptr;
            if (!late) sync(c);
            G1(sc, sc + 16 * FRAG);
            E1(c);
            if (late) sync(c);
            G2(sc + 16 * FRAG, sn);
        }
        flush();
    }
    ffn_stamp(dbg, 2);

    // ---- epilogue: + b2, dropout, + residual, bf16 rows ---------------------------------------------------------------
    const int m = row0 + tok;
    const bool live = m < M;
    const char* xres = reinterpret_cast<const char*>(x) + (size_t)my_row * (FD * 2);
    char* yrow = reinterpret_cast<char*>(y) + (size_t)my_row * (FD * 2);
    // the residual row (L2-hot: this workgroup read it in the prologue) in ONE batch of loads - the B-operand registers
    // are free by now - instead of one dependent round trip per tile
    uint4 res[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        res[2 * t] = *reinterpret_cast<const uint4*>(xres + (32 * t + 16 * half) * 2);
        res[2 * t + 1] = *reinterpret_cast<const uint4*>(xres + (32 * t + 16 * half + 8) * 2);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        uint32_t xc[4][4];
        tile_to_cols16(yacc[t], xc);
        const int n16 = 32 * t + 16 * half;
        uint4 pk[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float v[8], rv[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = __uint_as_float(xc[2 * cb][e]); v[4 + e] = __uint_as_float(xc[2 * cb + 1][e]); }
            const float4 b0 = *reinterpret_cast<const float4*>(sb2 + n16 + 8 * cb);
            const float4 b1v = *reinterpret_cast<const float4*>(sb2 + n16 + 8 * cb + 4);
            v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
            v[4] += b1v.x; v[5] += b1v.y; v[6] += b1v.z; v[7] += b1v.w;
            if (dr.on) {        // residual site: the library's standard draws (ids m * 256 + column, groups of 8), so that
                float dm[8];    // dsvg_drop_apply replays the mask for the unfused backward GEMMs
                drop_mult8(dr, (uint64_t)m * FD + n16 + 8 * cb, dm);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= dm[e];
            }
            unpack8(res[2 * t + cb], rv);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += rv[e];
            pk[cb] = pack8(v);
        }
        if (live) {
            *reinterpret_cast<uint4*>(yrow + n16 * 2) = pk[0];
            *reinterpret_cast<uint4*>(yrow + n16 * 2 + 16) = pk[1];
        }
    }
    ffn_stamp(dbg, 3);
}

// ---------------------------------------------------------------------------------------------------------------------
// forward, half-size workgroups: the same per-wave program (32 rows: LayerNorm -> G1 E1 G2 per chunk -> epilogue, results
// bit-identical to ffn_fwd_kernel) in workgroups of 4 waves = 128 rows with a ring of four 16 KiB HALF chunks (the W1 part /
// the W2 part of a chunk; 67 KiB of LDS), so that two workgroups fit on a CU.  Used for launches of at most 32,768 rows:
// 256 of these workgroups put ONE wave on every SIMD of the chip where 128 of the 256-row workgroups put two waves on
// every SIMD of half the CUs (1,000 rows: 28 us against 39; at full size the two kernels are equal, and delaying the second
// workgroup of a CU so that its prologue runs beside its partner's chunk loop - tried with a per-CU turn counter keyed by
// HW_ID / XCC_ID, removed again - gained nothing: two 128-row workgroups stream the weights twice, which saturates the
// L2 -> LDS path, see HISTORY.md "Round 3").
//   sync(hc) in front of every G: half chunk hc + 1 has landed (the A ring runs on into it), half chunk hc + 3 is issued
//   into the slot half chunk hc - 1 has left; hc + 2 stays in flight across the barrier (counted wait: 4 pieces per wave).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HSLOT = 16 * FRAG;        // half chunk: 16 fragments = 16 KiB
constexpr int HNBUF = 4;

template <bool TRAIN, bool PK>
__global__ __launch_bounds__(256, 2) void ffn_fwd_half_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ img,
                                                              const float* __restrict__ b1, const float* __restrict__ b2,
                                                              bf16_t* __restrict__ y, bf16_t* __restrict__ h_out,
                                                              bf16_t* __restrict__ xh_out, float* __restrict__ rstd_out,
                                                              int M, float eps, float drop_p,
                                                              const uint64_t* __restrict__ seed, uint32_t site_h,
                                                              uint32_t site_r, int n_chunks, unsigned long long* dbg, int warm) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];      // [4 half-chunk slots | b1 (2 KiB) | b2 (1 KiB)]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (dbg && lane == 0) dbg[((size_t)blockIdx.x * 4 + wave) * 4 + 0] = __builtin_amdgcn_s_memtime();
    const int tok = lane & 31, half = lane >> 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)DSVG_LDS_PTR(smem);
    float* sb1 = reinterpret_cast<float*>(smem + HNBUF * HSLOT);
    float* sb2 = sb1 + FF;
    const int n_half = 2 * n_chunks;

    // ---- weight stream: this wave moves pieces 4 wave .. 4 wave + 3 of every half chunk ------------------------------
    const char* my_src = reinterpret_cast<const char*>(img) + wave * 4096;
    const uint32_t my_dst = __builtin_amdgcn_readfirstlane(lds0 + wave * 4096);
    auto issue = [&](int hc) { dma4s(my_src + (size_t)hc * HSLOT, (uint32_t)lane * 16u, my_dst + (uint32_t)(hc % HNBUF) * HSLOT); };
    // (round 6, as in ffn_fwd_kernel: the half chunks behind the first three requested into this XCD's L2 up front, one per
    // workgroup, into this wave's own pieces of the free ring slot)
    if (warm && n_half > 3) dma4s(my_src + (size_t)(3 + (int)((blockIdx.x >> 3) % (unsigned)(n_half - 3))) * HSLOT, (uint32_t)lane * 16u, my_dst + 3u * HSLOT);
#pragma unroll
    for (int hc = 0; hc < 3; ++hc)
        if (hc < n_half) issue(hc);

    {
        const float bsc = PK ? drop_make(drop_p, seed, site_h).scale : 1.f;
        sb1[tid] = b1[tid] * bsc;
        sb1[tid + 256] = b1[tid + 256] * bsc;
    }
    sb2[tid] = b2[tid];

    // ---- the wave's 32 rows: LayerNorm in registers -> 16 B-operand fragments (as in ffn_fwd_kernel) -----------------
    const int row0 = blockIdx.x * 128 + wave * 32;
    const int my_row = min(row0 + tok, M - 1);
    bf16x8 xf[16];
    ffn_ln_rows<TRAIN>(x, my_row, half, TRAIN && row0 + tok < M, xh_out, rstd_out, eps, xf);
    __builtin_amdgcn_sched_barrier(0);

    const DropCtx dh = drop_make(drop_p, seed, site_h);
    const DropCtx dr = drop_make(drop_p, seed, site_r);

    floatx16 yacc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) yacc[t][r] = 0.f;
    floatx16 hid;
    bf16x8 hf[2];
    uint4 ring[4];

    const char* lbase = smem + lane * 16;
    auto slot_of = [&](int hc) -> const char* { return lbase + (hc % HNBUF) * HSLOT; };
    auto ld = [&](const char* p) -> uint4 { return *reinterpret_cast<const uint4*>(p); };

    uint4 stash[2];
    int stash_c = -1;
    char* hrow = TRAIN ? reinterpret_cast<char*>(h_out) + (size_t)my_row * (FF * 2) + half * 16 : nullptr;
    const bool hst = TRAIN && row0 + tok < M;
    auto flush = [&]() {
        if (TRAIN && stash_c >= 0) {
            if (hst) {
                *reinterpret_cast<uint4*>(hrow + (CH * stash_c) * 2) = stash[0];
                *reinterpret_cast<uint4*>(hrow + (CH * stash_c + 16) * 2) = stash[1];
            }
            stash_c = -1;
        }
    };
    auto sync = [&](int hc) {
        // loads return in order: "at most 4 outstanding" means half chunk hc + 1 - older than the 4 pieces of hc + 2 - has
        // landed; the h stores behind a sync can only make the wait stricter
        if (hc + 2 < n_half) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (hc + 3 < n_half) issue(hc + 3);
        flush();
    };
    auto g2frag = [](int p) -> int { return 2 * (p & 7) + (p >> 3); };      // G2 position -> fragment of the W2 chunk
    auto G1 = [&](const char* w1, const char* cont) {
#pragma unroll
        for (int r = 0; r < 16; ++r) hid[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            Frag8 a;
            a.u = ring[ks & 3];
            hid = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, xf[ks], hid, 0, 0, 0);
            if (ks + 4 < 16) ring[ks & 3] = ld(w1 + (ks + 4) * FRAG);
            else if (cont) ring[ks & 3] = ld(cont + g2frag(ks + 4 - 16) * FRAG);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto E1 = [&](int c) {
        const uint64_t id0 = (uint64_t)(row0 + tok) * FF + (uint32_t)(CH * c + 16 * half);
        const uint32_t hh = dh.on ? drop2_group(dh, id0 >> 4) : 0u;
        if (PK) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = hid[r];
            uint32_t pk[8];
            ffn_act_packed(v, dh, hh, pk, sb1 + CH * c + 4 * half);
            Frag8 f0, f1;
            f0.u = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            f1.u = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            hf[0] = f0.v; hf[1] = f1.v;
            if (TRAIN) { stash[0] = f0.u; stash[1] = f1.u; stash_c = c; }
            return;
        }
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
            float v[8];
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
                const int q = 2 * ks2 + qq;
                const float4 bb = *reinterpret_cast<const float4*>(sb1 + CH * c + 8 * q + 4 * half);
                v[4 * qq + 0] = fmaxf(hid[4 * q + 0] + bb.x, 0.f);
                v[4 * qq + 1] = fmaxf(hid[4 * q + 1] + bb.y, 0.f);
                v[4 * qq + 2] = fmaxf(hid[4 * q + 2] + bb.z, 0.f);
                v[4 * qq + 3] = fmaxf(hid[4 * q + 3] + bb.w, 0.f);
            }
            if (dh.on) {
                float m[8];
                drop2_mult8(dh, hh, ks2, m);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= m[e];
            }
            Frag8 f;
            f.u = pack8(v);
            hf[ks2] = f.v;
            if (TRAIN) stash[ks2] = f.u;
        }
        if (TRAIN) stash_c = c;
    };
    auto G2 = [&](const char* w2, const char* cont) {
        // position n: output tile n & 7, K step n >> 3 (fragment 2 (n & 7) + (n >> 3) of the packed chunk): the two MFMAs of
        // an accumulator are 8 apart instead of adjacent with a ring refill between them
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            Frag8 a;
            a.u = ring[n & 3];
            yacc[n & 7] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, hf[n >> 3], yacc[n & 7], 0, 0, 0);
            if (n + 4 < 16) ring[n & 3] = ld(w2 + g2frag(n + 4) * FRAG);
            else if (cont) ring[n & 3] = ld(cont + (n + 4 - 16) * FRAG);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    if (dbg && lane == 0) dbg[((size_t)blockIdx.x * 4 + wave) * 4 + 1] = __builtin_amdgcn_s_memtime();
    if (n_chunks > 0) {
        // half chunk 0 has to be readable before the ring is primed: everything but the newest 4 operations (the last
        // xh stores when training, else the pieces of half chunk 2) done, and the other waves' pieces behind the barrier
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            const char* s0 = slot_of(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) ring[i] = ld(s0 + i * FRAG);
        }
        for (int c = 0; c < n_chunks; ++c) {
            sync(2 * c);
            G1(slot_of(2 * c), slot_of(2 * c + 1));
            E1(c);
            sync(2 * c + 1);
            G2(slot_of(2 * c + 1), (c + 1 < n_chunks) ? slot_of(2 * c + 2) : nullptr);
        }
        flush();
    }
    if (dbg && lane == 0) dbg[((size_t)blockIdx.x * 4 + wave) * 4 + 2] = __builtin_amdgcn_s_memtime();

    // ---- epilogue: + b2, dropout, + residual, bf16 rows (as in ffn_fwd_kernel) ---------------------------------------
    const int m = row0 + tok;
    const bool live = m < M;
    const char* xres = reinterpret_cast<const char*>(x) + (size_t)my_row * (FD * 2);
    char* yrow = reinterpret_cast<char*>(y) + (size_t)my_row * (FD * 2);
    uint4 res[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        res[2 * t] = *reinterpret_cast<const uint4*>(xres + (32 * t + 16 * half) * 2);
        res[2 * t + 1] = *reinterpret_cast<const uint4*>(xres + (32 * t + 16 * half + 8) * 2);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        uint32_t xc[4][4];
        tile_to_cols16(yacc[t], xc);
        const int n16 = 32 * t + 16 * half;
        uint4 pk[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float v[8], rv[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = __uint_as_float(xc[2 * cb][e]); v[4 + e] = __uint_as_float(xc[2 * cb + 1][e]); }
            const float4 b0 = *reinterpret_cast<const float4*>(sb2 + n16 + 8 * cb);
            const float4 b1v = *reinterpret_cast<const float4*>(sb2 + n16 + 8 * cb + 4);
            v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
            v[4] += b1v.x; v[5] += b1v.y; v[6] += b1v.z; v[7] += b1v.w;
            if (dr.on) {
                float dm[8];
                drop_mult8(dr, (uint64_t)m * FD + n16 + 8 * cb, dm);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= dm[e];
            }
            unpack8(res[2 * t + cb], rv);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += rv[e];
            pk[cb] = pack8(v);
        }
        if (live) {
            *reinterpret_cast<uint4*>(yrow + n16 * 2) = pk[0];
            *reinterpret_cast<uint4*>(yrow + n16 * 2 + 16) = pk[1];
        }
    }
    if (dbg && lane == 0) dbg[((size_t)blockIdx.x * 4 + wave) * 4 + 3] = __builtin_amdgcn_s_memtime();
}

// ---------------------------------------------------------------------------------------------------------------------
// backward: dx = dy + LayerNorm'( dpre . W1' ), the FFN backward's only kernel in this file (dpre comes from the gated GEMM over
// the forward kernel's h, the weight gradients from the library's GEMMs + the finish kernels below).  Token-stationary like the
// forward kernel; the B operands (dpre in fragment order, the layout of the forward kernel's h, see TRAIN above) come straight
// from global memory, one chunk ahead; W1'^T chunks (the last 16 KiB of every 48 KiB backward chunk) stream through a 4-slot LDS
// ring.  The LayerNorm backward needs no gamma (it is inside W1'): dx = dy + rstd * (g - mean(g) - xh * mean(g * xh)), g = dxh,
// statistics over the row in registers.
// ---------------------------------------------------------------------------------------------------------------------
template <bool PROBE>       // (PROBE: the stamps below; the production instantiation carries none of their code - they cost it 33 spilled registers)
__global__ __launch_bounds__(512, 2) void ffn_bwd_dx_kernel(const bf16_t* __restrict__ dpre, const bf16_t* __restrict__ x,
                                                            const bf16_t* __restrict__ dy, const bf16_t* __restrict__ img,
                                                            bf16_t* __restrict__ dx, int M, float eps,
                                                            bf16_t* __restrict__ dxm, float drop_p,
                                                            const uint64_t* __restrict__ seed, uint32_t site_m, int warm,
                                                            unsigned long long* dbg) {
    constexpr int NBUF = 4, SLOT = 16 * FRAG;
    if (PROBE) bwd_stamp(dbg, 0);
    extern __shared__ __attribute__((aligned(1024))) char smem[];      // [4 x 16 KiB]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = lane & 31, half = lane >> 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)DSVG_LDS_PTR(smem);
    // this wave moves pieces 2 wave, 2 wave + 1 of every 16-piece chunk
    const char* my_src = reinterpret_cast<const char*>(img) + 32 * FRAG + wave * 2048 + lane * 16;
    const uint32_t my_dst = __builtin_amdgcn_readfirstlane(lds0 + wave * 2048);
    auto issue = [&](int c) { dma2(my_src + (size_t)c * BWD_CHUNK, my_dst + (uint32_t)(c % NBUF) * SLOT); };
    // (round 6, as in ffn_fwd_kernel: the W1'^T chunks are cold in this XCD's L2 and walked in lockstep - the workgroups of an
    // XCD request the chunks behind the first two up front, one each, into this wave's own pieces of ring slot 3)
    if (warm) dma2(my_src + (size_t)(2 + (blockIdx.x >> 3) % (unsigned)(NCH - 2)) * BWD_CHUNK, my_dst + 3u * SLOT);
    issue(0);
    issue(1);

    const int row0 = blockIdx.x * TOK_PER_WG + wave * 32;
    const int m = row0 + tok;
    const int my_row = min(m, M - 1);
    const char* pr = reinterpret_cast<const char*>(dpre) + (size_t)my_row * (FF * 2) + half * 16;
    auto bfrag = [&](int c, int ks2) -> uint4 { return *reinterpret_cast<const uint4*>(pr + (CH * c + 16 * ks2) * 2); };

    floatx16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // B operands: a register ring 4 chunks deep (a chunk is 0.25 us of MFMA work per wave, a global load 1 - 2 us under
    // load).  Per iteration this wave issues 2 DMA pieces (chunk c + 2) and 2 B loads (chunk c + 4), all loads, returned
    // in order: "everything but the 4 newest has landed" = chunk c's DMA (issued 2 iterations ago) and its B operands.
    uint4 bq[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { bq[i][0] = bfrag(i, 0); bq[i][1] = bfrag(i, 1); }
    const char* lbase = smem + lane * 16;
    auto chunk = [&](int c, uint4 (&b)[2], bool more, int pend) {
        // pend = loads this wave may leave in flight: the previous iteration's (4 in the steady state, 2 / 0 in the tail)
        if (pend == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (pend == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();       // chunk c landed for everybody; the slot of chunk c - 2 is free again
        if (PROBE && c == 0) bwd_stamp(dbg, 1);
        if (c + 2 < NCH) issue(c + 2);
        const char* sc = lbase + (c % NBUF) * SLOT;
        Frag8 b0, b1;
        b0.u = b[0]; b1.u = b[1];
        if (more) { b[0] = bfrag(c + 4, 0); b[1] = bfrag(c + 4, 1); }
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            Frag8 a;
            a.u = *reinterpret_cast<const uint4*>(sc + n * FRAG);
            acc[n >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, (n & 1) ? b1.v : b0.v, acc[n >> 1], 0, 0, 0);
        }
    };
    for (int c = 0; c < NCH - 4; c += 4) {
        chunk(c, bq[0], true, 4); chunk(c + 1, bq[1], true, 4); chunk(c + 2, bq[2], true, 4); chunk(c + 3, bq[3], true, 4);
    }
    // tail: no more B loads, only the last two DMA issues (2 pieces each) are left to overlap with
    chunk(NCH - 4, bq[0], false, 0); chunk(NCH - 3, bq[1], false, 2); chunk(NCH - 2, bq[2], false, 2);
    chunk(NCH - 1, bq[3], false, 0);

    if (PROBE) bwd_stamp(dbg, 2);
    // ---- epilogue: LayerNorm backward on the rows in registers ------------------------------------------------------------
    // (scripts/ffn_bwd_dx_probe.py, 63,488 rows: first chunk ready after 6 us, K loop 20 us, then three serialised bursts of the
    // whole launch - x rows 9.5 us, residual rows 10.6 us, stores 10 us.  Round 6 tried to request the x rows before the loop:
    // a wave's loads return IN ORDER, so as its oldest loads they delayed the first chunk by what the epilogue saved (first chunk
    // ready after 16 us, x phase 2 us, step +1.5 %); behind the B operands of chunk c + 2 they can be at most 3 chunks early.)
    // tiles -> the lane's 16 consecutive columns per tile (in place), x row in the same layout
    const char* xrow = reinterpret_cast<const char*>(x) + (size_t)my_row * (FD * 2);
    uint4 xr[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        xr[2 * t] = *reinterpret_cast<const uint4*>(xrow + (32 * t + 16 * half) * 2);
        xr[2 * t + 1] = *reinterpret_cast<const uint4*>(xrow + (32 * t + 16 * half + 8) * 2);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        uint32_t xc[4][4];
        tile_to_cols16(acc[t], xc);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][4 * q + e] = __uint_as_float(xc[q][e]);      // column 4 q + e of the 16
    }
    float s, q, mean, rstd;
    ln_stats_packed(xr, s, q);
    ln_mean_rstd256(s, q, eps, mean, rstd);
    if (PROBE) bwd_stamp(dbg, 3);
    const float shift = -mean * rstd;       // xh = x * rstd + shift
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float v[8];
            unpack8(xr[2 * t + cb], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float g = acc[t][8 * cb + e];
                c1 += g;
                c2 += g * fmaf(v[e], rstd, shift);
            }
        }
    c1 += __shfl_xor(c1, 32, 64);
    c2 += __shfl_xor(c2, 32, 64);
    c1 *= (1.f / FD);
    c2 *= (1.f / FD);
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(xr[i].x), "+v"(xr[i].y), "+v"(xr[i].z), "+v"(xr[i].w));
    // w = rstd * (g - c1 - xh * c2) in place; then the x registers are dead and make room for dy
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float v[8];
            unpack8(xr[2 * t + cb], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[t][8 * cb + e] = rstd * (acc[t][8 * cb + e] - c1 - fmaf(v[e], rstd, shift) * c2);
        }
    // (the dy loads below must not be hoisted above the pass that frees the x registers: an address offset that is
    // opaque to the compiler - always 0 - and ordered behind the last value of that pass pins them here)
    if (PROBE) bwd_stamp(dbg, 4);
    uint32_t zoff = 0;
    asm volatile("" : "+v"(zoff) : "v"(acc[7][15]), "v"(acc[0][0]));
    const char* dyrow = reinterpret_cast<const char*>(dy) + (size_t)my_row * (FD * 2) + zoff;
    char* orow = reinterpret_cast<char*>(dx) + (size_t)my_row * (FD * 2);
    // optional second output: dx with the dropout mask of the attention sub-block's residual site replayed on it (what
    // dsvg_drop_apply would make of the rounded dx: the next two GEMMs of the backward pass read it)
    char* mrow = dxm ? reinterpret_cast<char*>(dxm) + (size_t)my_row * (FD * 2) : nullptr;
    uint4 dr[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        dr[2 * t] = *reinterpret_cast<const uint4*>(dyrow + (32 * t + 16 * half) * 2);
        dr[2 * t + 1] = *reinterpret_cast<const uint4*>(dyrow + (32 * t + 16 * half + 8) * 2);
    }
    if (PROBE) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); bwd_stamp(dbg, 5); }
    if (m < M) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                float v[8];
                unpack8(dr[2 * t + cb], v);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += acc[t][8 * cb + e];
                *reinterpret_cast<uint4*>(orow + (32 * t + 16 * half + 8 * cb) * 2) = pack8(v);
            }
    }
    if (PROBE) bwd_stamp(dbg, 6);
    if (mrow && m < M) {
        // second pass, from the rows this lane has just stored (L2-hot; the registers above are all in use in the first
        // pass): wait for the stores, then read back through an address the compiler cannot match with them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t zo2 = 0;
        asm volatile("" : "+v"(zo2));
        const char* back = orow + zo2;
        const DropCtx dcm = drop_make(drop_p, seed, site_m);
#pragma unroll 2
        for (int i = 0; i < 16; ++i) {
            const int col = 32 * (i >> 1) + 16 * half + 8 * (i & 1);
            const uint4 pk = *reinterpret_cast<const uint4*>(back + col * 2);
            float w[8], mm[8];
            unpack8(pk, w);
            drop_mult8(dcm, (uint64_t)m * FD + col, mm);
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] *= mm[e];
            *reinterpret_cast<uint4*>(mrow + col * 2) = pack8(w);
        }
    }
    if (PROBE) bwd_stamp(dbg, 7);
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradients, last step.  The two split-K GEMMs deliver G1p = dpre^T xh [512 (fragment order), 256], its row sums
// db1p [512 (fragment order)] and G2p = dym^T h [256, 512 (fragment order)]; this kernel undoes the fragment order
// (position p(j): bits 2 and 3 of j swapped) and the LayerNorm fold (see ffn_pack_kernel):
//     dW1[j][k] = gamma[k] G1p[p(j)][k] + beta[k] db1p[p(j)],   db1[j] = db1p[p(j)],   dW2[o][j] = G2p[o][p(j)],
//     dgamma[k] = sum_j W1[j][k] G1p[p(j)][k],                  dbeta[k] = sum_j W1[j][k] db1p[p(j)]
// One workgroup per 4 columns k (and 4 rows o of dW2); fixed summation order (deterministic).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ffn_wgrad_finish_body(const float* __restrict__ G1p, const float* __restrict__ db1p,
                                                      const float* __restrict__ G2p, const float* __restrict__ W1,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ dW1, float* __restrict__ db1,
                                                      float* __restrict__ dW2, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, int block) {
    __shared__ float red[2][4][256];
    const int t = threadIdx.x;
    const int k0 = block * 4;
    const float4 ga = *reinterpret_cast<const float4*>(gamma + k0);
    const float4 be = *reinterpret_cast<const float4*>(beta + k0);
    float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int j = t + 256 * jj, pj = frag_pos(j);
        const float4 g = *reinterpret_cast<const float4*>(G1p + (size_t)pj * FD + k0);
        const float4 w = *reinterpret_cast<const float4*>(W1 + (size_t)j * FD + k0);
        const float b = db1p[pj];
        *reinterpret_cast<float4*>(dW1 + (size_t)j * FD + k0) =
            make_float4(ga.x * g.x + be.x * b, ga.y * g.y + be.y * b, ga.z * g.z + be.z * b, ga.w * g.w + be.w * b);
        dg[0] += w.x * g.x; dg[1] += w.y * g.y; dg[2] += w.z * g.z; dg[3] += w.w * g.w;
        db[0] += w.x * b; db[1] += w.y * b; db[2] += w.z * b; db[3] += w.w * b;
        if (block == 0) db1[j] = b;
        // rows o = k0 .. k0 + 3 of dW2 (block < 64 covers all 256 rows)
#pragma unroll
        for (int oo = 0; oo < 4; ++oo) dW2[(size_t)(k0 + oo) * FF + j] = G2p[(size_t)(k0 + oo) * FF + pj];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[0][i][t] = dg[i]; red[1][i][t] = db[i]; }
    __syncthreads();
    if (t < 8) {        // fixed-order sums: thread t < 4 -> dgamma[k0 + t], t >= 4 -> dbeta[k0 + t - 4]
        const float* r = red[t >> 2][t & 3];
        float a = 0.f;
        for (int i = 0; i < 256; ++i) a += r[i];
        if (t < 4) dgamma[k0 + t] = a; else dbeta[k0 + t - 4] = a;
    }
}
__global__ __launch_bounds__(256) void ffn_wgrad_finish_kernel(const float* __restrict__ G1p, const float* __restrict__ db1p,
                                                               const float* __restrict__ G2p, const float* __restrict__ W1,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ dW1, float* __restrict__ db1,
                                                               float* __restrict__ dW2, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
    ffn_wgrad_finish_body(G1p, db1p, G2p, W1, gamma, beta, dW1, db1, dW2, dgamma, dbeta, (int)blockIdx.x);
}
// the same for up to 16 layers in one launch (the table travels in the kernel arguments): a backward pass finishes all of
// its fused-FFN layers behind the one batched reduction launch
constexpr int FINISH_MAX = 16;
struct FinishTable { const float* in[FINISH_MAX][6]; float* out[FINISH_MAX][5]; };
__global__ __launch_bounds__(256) void ffn_wgrad_finish_many_kernel(const FinishTable t) {
    const int layer = blockIdx.x / (FD / 4), block = blockIdx.x % (FD / 4);
    ffn_wgrad_finish_body(t.in[layer][0], t.in[layer][1], t.in[layer][2], t.in[layer][3], t.in[layer][4], t.in[layer][5],
                          t.out[layer][0], t.out[layer][1], t.out[layer][2], t.out[layer][3], t.out[layer][4], block);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int64_t dsvg_ffn_pack_bytes(int32_t n_layers, int32_t which) {
    return (int64_t)n_layers * NCH * (which == 0 ? FWD_CHUNK : BWD_CHUNK);
}

extern "C" int dsvg_ffn_pack(const float* flat_f32, const int64_t* offs, int32_t n_layers, int32_t d_model, int32_t d_ff,
                             void* packed_fwd, void* packed_bwd, float* b1_folded, void* w2p, void* stream) {
    DSVG_CHECK_ARG(flat_f32 && offs && packed_fwd && packed_bwd && b1_folded, "ffn_pack: null pointer");
    DSVG_CHECK_ARG(d_model == FD && d_ff == FF, "ffn_pack: the fused FFN kernels are built for d_model 256 / dim_ff 512");
    DSVG_CHECK_ARG(n_layers > 0, "ffn_pack: bad layer count");
    const long long n = (long long)n_layers * NCH * 80 * 64;
    hipLaunchKernelGGL(ffn_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flat_f32, offs,
                       n_layers, (bf16_t*)packed_fwd, (bf16_t*)packed_bwd);
    hipLaunchKernelGGL(ffn_fold_bias_kernel, dim3((unsigned)((n_layers * FF + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       flat_f32, offs, n_layers, b1_folded);
    if (w2p) {
        const long long n8 = (long long)n_layers * (FD * FF / 8);
        hipLaunchKernelGGL(ffn_w2p_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flat_f32, offs,
                           n_layers, (bf16_t*)w2p);
    }
    DSVG_LAUNCH_CHECK("ffn_pack");
    return 0;
}

static unsigned long long* g_ffn_dbg_host = nullptr;      // development probe, see dsvg_ffn_debug_clock

extern "C" int dsvg_ffn_fwd(const void* x, const void* packed_fwd_layer, const float* b1_folded, const float* b2, void* y,
                            void* h_out, void* xh_out, float* rstd_out, int64_t rows, float eps, float drop_p,
                            uint32_t site_hidden, uint32_t site_res, const void* seed, int32_t stages, void* stream) {
    DSVG_CHECK_ARG(x && packed_fwd_layer && b1_folded && b2 && y, "ffn_fwd: null pointer");
    DSVG_CHECK_ARG(rows > 0 && rows < (1ll << 31) - TOK_PER_WG, "ffn_fwd: bad row count");
    DSVG_CHECK_ARG(!(drop_p > 0.f) || seed, "ffn_fwd: dropout needs a seed");
    const bool train = h_out != nullptr;
    DSVG_CHECK_ARG(!train || (xh_out && rstd_out), "ffn_fwd: h_out, xh_out and rstd_out come together");
    DSVG_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)packed_fwd_layer | (uintptr_t)h_out | (uintptr_t)xh_out) & 15) == 0,
                   "ffn_fwd: operands must be 16-byte aligned");
    const int nb = (int)((rows + TOK_PER_WG - 1) / TOK_PER_WG);
    hipStream_t st = (hipStream_t)stream;
    // 0 default, 2 half-size workgroups, 3 / 4 ring slots of the 256-row kernel, 6 / 7 = 4 / 2 with the packed activation
    const int stages_arg = stages;
    DSVG_CHECK_ARG(stages == 0 || stages == 2 || stages == 3 || stages == 4 || stages == 6 || stages == 7,
                   "ffn_fwd: stages must be one of 0, 2, 3, 4, 6, 7");
    if (stages == 0 || stages == 2 || stages == 6 || stages == 7) stages = 4;
    // training variant: 4 slots (chunk k + 2's DMA in flight across the syncs, counted waits) or 3 (every sync drains the
    // wave's h stores too); DSVG_FFN_TRAIN_STAGES for the A/B
    static const int train_stages = getenv("DSVG_FFN_TRAIN_STAGES") ? atoi(getenv("DSVG_FFN_TRAIN_STAGES")) : 4;
    if (train) stages = train_stages == 3 ? 3 : 4;
    // timing probe only (results are wrong below 16): number of hidden chunks actually processed
    static const int dbg_chunks = getenv("DSVG_FFN_DBG_CHUNKS") ? atoi(getenv("DSVG_FFN_DBG_CHUNKS")) : NCH;
    static const int w_warm = getenv("DSVG_W_WARM") ? atoi(getenv("DSVG_W_WARM")) : 1;      // A/B knob: weight image into L2 up front
#define DSVG_FFN_FWD(NB, TR, PK)                                                                                      \
    do {                                                                                                              \
        const size_t lds = (size_t)NB * FWD_CHUNK + 3072;                                                             \
        DSVG_ENSURE_LDS((ffn_fwd_kernel<NB, TR, PK>), lds);                                                           \
        hipLaunchKernelGGL((ffn_fwd_kernel<NB, TR, PK>), dim3(nb), dim3(512), lds, st, (const bf16_t*)x,               \
                           (const bf16_t*)packed_fwd_layer, b1_folded, b2, (bf16_t*)y, (bf16_t*)h_out, (bf16_t*)xh_out,\
                           rstd_out, (int)rows, eps, drop_p, (const uint64_t*)seed, site_hidden, site_res, dbg_chunks,    \
                           g_ffn_dbg_host, w_warm);                                                                   \
    } while (0)
    // half-size workgroups (stages 2, or by default up to 32,768 rows; DSVG_FFN_HALF=0 / 1 forces the choice)
    static const int half_env = getenv("DSVG_FFN_HALF") ? atoi(getenv("DSVG_FFN_HALF")) : -1;
    // packed activation (ffn_act_packed; dropout rates up to 0.5): stages 6 / 7 = the 256-row / half-size workgroups with it,
    // 0 = the library's choice (DSVG_FFN_PACKED=0 / 1 forces it for the default)
    static const int pk_env = getenv("DSVG_FFN_PACKED") ? atoi(getenv("DSVG_FFN_PACKED")) : 1;
    const bool pk = !(drop_p > 0.5f) && (stages_arg == 6 || stages_arg == 7 || (stages_arg == 0 && pk_env != 0));
    const bool half_on = stages_arg == 2 || stages_arg == 7 || (stages_arg == 0 && (half_env >= 0 ? half_env != 0 : rows <= 32768));
    if (half_on) {
        const int nbh = (int)((rows + 127) / 128);
        const size_t lds = (size_t)HNBUF * HSLOT + 3072;
#define DSVG_FFN_FWD_HALF(TR, PK)                                                                                     \
    do {                                                                                                              \
        DSVG_ENSURE_LDS((ffn_fwd_half_kernel<TR, PK>), lds);                                                          \
        hipLaunchKernelGGL((ffn_fwd_half_kernel<TR, PK>), dim3(nbh), dim3(256), lds, st, (const bf16_t*)x,             \
                           (const bf16_t*)packed_fwd_layer, b1_folded, b2, (bf16_t*)y, (bf16_t*)h_out, (bf16_t*)xh_out,\
                           rstd_out, (int)rows, eps, drop_p, (const uint64_t*)seed, site_hidden, site_res, dbg_chunks,    \
                           g_ffn_dbg_host, w_warm);                                                                   \
    } while (0)
        if (train && pk) DSVG_FFN_FWD_HALF(true, true);
        else if (train) DSVG_FFN_FWD_HALF(true, false);
        else if (pk) DSVG_FFN_FWD_HALF(false, true);
        else DSVG_FFN_FWD_HALF(false, false);
#undef DSVG_FFN_FWD_HALF
        DSVG_LAUNCH_CHECK("ffn_fwd (half-size workgroups)");
        return 0;
    }
    if (pk) {
        if (train) DSVG_FFN_FWD(4, true, true);
        else DSVG_FFN_FWD(4, false, true);
    } else if (train && stages == 3) DSVG_FFN_FWD(3, true, false);
    else if (train) DSVG_FFN_FWD(4, true, false);
    else if (stages == 3) DSVG_FFN_FWD(3, false, false);
    else DSVG_FFN_FWD(4, false, false);
#undef DSVG_FFN_FWD
    DSVG_LAUNCH_CHECK("ffn_fwd");
    return 0;
}

/* development probe: buf = device buffer of (workgroups * 8 * 4) uint64 or NULL (off); see ffn_stamp */
extern "C" int dsvg_ffn_debug_clock(void* buf) {
    g_ffn_dbg_host = (unsigned long long*)buf;
    return 0;
}

extern "C" int dsvg_ffn_bwd_dx(const void* dpre, const void* x, const void* dy, const void* packed_bwd_layer, void* dx,
                               int64_t rows, float eps, void* dx_masked, float drop_p, uint32_t drop_site, const void* seed,
                               void* stream) {
    DSVG_CHECK_ARG(dpre && x && dy && packed_bwd_layer && dx, "ffn_bwd_dx: null pointer");
    DSVG_CHECK_ARG(!dx_masked || !(drop_p > 0.f) || seed, "ffn_bwd_dx: the masked output needs a seed");
    DSVG_CHECK_ARG(((uintptr_t)dx_masked & 15) == 0, "ffn_bwd_dx: operands must be 16-byte aligned");
    DSVG_CHECK_ARG(rows > 0 && rows < (1ll << 31) - TOK_PER_WG, "ffn_bwd_dx: bad row count");
    DSVG_CHECK_ARG((((uintptr_t)dpre | (uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)packed_bwd_layer) & 15) == 0,
                   "ffn_bwd_dx: operands must be 16-byte aligned");
    const int nb = (int)((rows + TOK_PER_WG - 1) / TOK_PER_WG);
    const size_t lds2 = 4 * 16 * FRAG;
    static const int w_warm = getenv("DSVG_W_WARM") ? atoi(getenv("DSVG_W_WARM")) : 1;      // A/B knob
    unsigned long long* probe = ((uintptr_t)g_ffn_dbg_host & 2) ? g_ffn_dbg_host : nullptr;
    if (probe)
        hipLaunchKernelGGL(ffn_bwd_dx_kernel<true>, dim3(nb), dim3(512), lds2, (hipStream_t)stream, (const bf16_t*)dpre,
                       (const bf16_t*)x, (const bf16_t*)dy, (const bf16_t*)packed_bwd_layer, (bf16_t*)dx, (int)rows, eps,
                       (bf16_t*)dx_masked, drop_p, (const uint64_t*)seed, drop_site, w_warm,
                       probe);
    else
        hipLaunchKernelGGL(ffn_bwd_dx_kernel<false>, dim3(nb), dim3(512), lds2, (hipStream_t)stream, (const bf16_t*)dpre,
                       (const bf16_t*)x, (const bf16_t*)dy, (const bf16_t*)packed_bwd_layer, (bf16_t*)dx, (int)rows, eps,
                       (bf16_t*)dx_masked, drop_p, (const uint64_t*)seed, drop_site, w_warm,
                       (unsigned long long*)nullptr);
    DSVG_LAUNCH_CHECK("ffn_bwd_dx");
    return 0;
}

extern "C" int dsvg_ffn_wgrad_finish(const float* g1p, const float* db1p, const float* g2p, const float* w1,
                                     const float* gamma, const float* beta, float* dw1, float* db1, float* dw2,
                                     float* dgamma, float* dbeta, void* stream) {
    DSVG_CHECK_ARG(g1p && db1p && g2p && w1 && gamma && beta && dw1 && db1 && dw2 && dgamma && dbeta,
                   "ffn_wgrad_finish: null pointer");
    hipLaunchKernelGGL(ffn_wgrad_finish_kernel, dim3(FD / 4), dim3(256), 0, (hipStream_t)stream, g1p, db1p, g2p, w1, gamma,
                       beta, dw1, db1, dw2, dgamma, dbeta);
    DSVG_LAUNCH_CHECK("ffn_wgrad_finish");
    return 0;
}

extern "C" int dsvg_ffn_wgrad_finish_many(const void* const* ptrs, int32_t n_layers, void* stream) {
    DSVG_CHECK_ARG(ptrs && n_layers > 0, "ffn_wgrad_finish_many: bad arguments");
    for (int base = 0; base < n_layers; base += FINISH_MAX) {
        const int n = n_layers - base < FINISH_MAX ? n_layers - base : FINISH_MAX;
        FinishTable t{};
        for (int i = 0; i < n; ++i) {
            const void* const* p = ptrs + (size_t)(base + i) * 11;
            for (int k = 0; k < 11; ++k) DSVG_CHECK_ARG(p[k], "ffn_wgrad_finish_many: null pointer");
            for (int k = 0; k < 6; ++k) t.in[i][k] = (const float*)p[k];
            for (int k = 0; k < 5; ++k) t.out[i][k] = (float*)const_cast<void*>(p[6 + k]);
        }
        hipLaunchKernelGGL(ffn_wgrad_finish_many_kernel, dim3(n * (FD / 4)), dim3(256), 0, (hipStream_t)stream, t);
        DSVG_LAUNCH_CHECK("ffn_wgrad_finish_many");
    }
    return 0;
}
