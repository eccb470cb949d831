// Affine maps of a batch of icons: the zoom / translate / rotate / normalize calls of the reference's SVG class
// (deepsvg/svglib/svg.py:268-300, 392-394 with Point.translate / scale / rotate_, svglib/geom.py:136-151) and the random
// augmentation of its on-the-fly data set (SVGDataset._augment / preprocess, deepsvg/svg_dataset.py:137-156), as a program of
// float32 steps.  The definition is in include/dsvg.h; tests/paths_transform_ref.py restates it in numpy float32 and
// tests/golden/paths/transform.npz holds the reference's own results.
//   dsvg_paths_transform      padded commands [N, G, S] / args [N, G, S, 11] -> args of the same shape.  One workgroup per icon,
//                             one thread per row (8 rounds of 256 for the largest icon); the ballot scan of svg_seq.h gives the
//                             first-EOS rule, and a live row runs the item's steps on its enabled coordinate pairs.
//   dsvg_assemble_augmented   the sibling of dsvg_assemble_batch over a float32 row store: the token layout of
//                             assemble_layout.h with a row source that runs the item's steps, and the rounding, on every row
//                             it loads - the previous real command's end position included, which args_rel is relative to.
// Both stream: 44..48 B read and 44..136 B written per row, a few float32 operations in between.  Consecutive lanes take
// consecutive rows, so a wave reads and writes one contiguous span (64 x 44 B of arguments, 64 x 48 B of store rows as three
// 16-byte loads per lane) and every fetched line is used in full; the 44-byte rows of the padded layout are only 4-byte
// aligned, which leaves their loads and stores at one dword each.  The step kinds are launch
// constants, the parameters device memory [N, K, 3]: no device-to-host read, no atomics, no workspace; every output element
// is written.
#include "dsvg_common.h"
#include "svg_seq.h"             // vocabulary, the argument mask, block_flag_scan
#include "assemble_layout.h"     // the token layout: assemble_kernel over a row source
#include "../../include/dsvg.h"

// every add and every multiply is rounded to float32 on its own, as numpy does it one in-place operation at a time: no fused
// multiply-add ((p - c) * f + c is NOT one fma, and c x - s y is two products and a difference).  The arithmetic below is
// written with plain operators on purpose: the pragma governs the operations written in THIS file; the rotate spelled with
// __fmul_rn / __fsub_rn (inline functions of the HIP headers) compiled to v_pk_fma_f32 here, with plain operators it compiles
// to v_pk_mul_f32 and an add.  Check the ISA (no v_fma / v_pk_fma on a float operand) after touching this arithmetic.
#pragma clang fp contract(off)

namespace {
constexpr int PT_THREADS = SP_THREADS;
constexpr int PT_MAX_ROWS = SP_MAX_TOK;   // G * S rows of one icon
typedef unsigned short pt_u16;

// ---- the step interpreter, written once for both kernels -------------------------------------------------------------------
// kinds: 2 bits per step, step k in bits 2k..2k+1; p: the item's parameters [K, 3]
struct StepProgram {
    int K;
    uint32_t kinds;
    const float* __restrict__ params;     // [N, K, 3]
    int num;                              // numericalize: 0 = off
    __device__ __forceinline__ const float* of(long long n) const { return params + n * (long long)K * 3; }
};

__device__ __forceinline__ float pt_num(float v, int n) { return fminf(fmaxf(rintf(v), 0.f), (float)(n - 1)); }

// one coordinate pair through all steps
__device__ __forceinline__ void steps_point(const StepProgram& sp, const float* __restrict__ p, float& x, float& y) {
    for (int k = 0; k < sp.K; ++k) {
        const int kind = (int)((sp.kinds >> (2 * k)) & 3u);
        const float p0 = p[3 * k], p1 = p[3 * k + 1];
        if (kind == DSVG_STEP_TRANSLATE) {
            x = x + p0;
            y = y + p1;
        } else if (kind == DSVG_STEP_SCALE) {
            x = x * p0;
            y = y * p0;
        } else {                          // rotate: p0 = cos, p1 = sin
            const float cx = p0 * x, sy = p1 * y, sx = p1 * x, cy = p0 * y;
            const float nx = cx - sy;
            const float ny = sx + cy;
            x = nx;
            y = ny;
        }
    }
    if (sp.num > 0) {
        x = pt_num(x, sp.num);
        y = pt_num(y, sp.num);
    }
}

// a whole row: command c with its 11 arguments, for item n
__device__ __forceinline__ void steps_row(const StepProgram& sp, long long n, int c, float* __restrict__ a) {
    const float* p = sp.of(n);
    if (c == CMD_M || c == CMD_L || c == CMD_C || c == CMD_A) steps_point(sp, p, a[ARG_END], a[ARG_END + 1]);
    if (c == CMD_C) {
        steps_point(sp, p, a[ARG_CONTROL1], a[ARG_CONTROL1 + 1]);
        steps_point(sp, p, a[ARG_CONTROL2], a[ARG_CONTROL2 + 1]);
    }
    if (c == CMD_A) {
        // radii: scale steps only (Radius.translate is a no-op); a rotate step turns the x axis; flags are copied
        for (int k = 0; k < sp.K; ++k) {
            const int kind = (int)((sp.kinds >> (2 * k)) & 3u);
            if (kind == DSVG_STEP_SCALE) {
                a[0] = a[0] * p[3 * k];
                a[1] = a[1] * p[3 * k];
            } else if (kind == DSVG_STEP_ROTATE) {
                a[2] = a[2] + p[3 * k + 2];
            }
        }
        if (sp.num > 0) {
#pragma unroll
            for (int q = 0; q < ARG_CONTROL1; ++q) a[q] = pt_num(a[q], sp.num);
        }
    }
}

// ---- dsvg_paths_transform ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_THREADS) void paths_transform_kernel(const float* __restrict__ commands,
                                                                      const float* __restrict__ args, int G, int S,
                                                                      const StepProgram sp, float* __restrict__ out_args) {
    __shared__ pt_u16 pe[PT_MAX_ROWS + 1];    // EOS rows before row t
    __shared__ int wtot[PT_MAX_ROWS / 64];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int R = G * S;
    const float* cmd = commands + b * R;
    const float* arg = args + b * R * N_ARGS;
    float* out = out_args + b * R * N_ARGS;

    // a group ends at its first EOS
    block_flag_scan<PT_MAX_ROWS>(R, pe, wtot, [&](int t) { return t < R && (int)cmd[t] == CMD_EOS; });
    for (int t = tid; t < R; t += PT_THREADS) {
        float v[N_ARGS];
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) v[a] = arg[(long long)t * N_ARGS + a];
        const bool live = pe[t + 1] == pe[(t / S) * S];
        if (live) steps_row(sp, b, (int)cmd[t], v);
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) out[(long long)t * N_ARGS + a] = v[a];
    }
}

// ---- dsvg_assemble_augmented: the float32 store, transformed and rounded as it is loaded ---------------------------------
constexpr int FROW_W = N_ARGS + 1;        // floats per stored row

struct FloatRows {
    const float* __restrict__ rows;
    StepProgram sp;

    __device__ __forceinline__ Row load(long long r) const {
        // 48-byte rows: three 16-byte loads (the array base is 16-byte aligned)
        const float4* p = reinterpret_cast<const float4*>(rows + r * FROW_W);
        const float4 q0 = p[0], q1 = p[1], q2 = p[2];
        Row o;
        o.cmd = q0.x;
        o.a[0] = q0.y; o.a[1] = q0.z; o.a[2] = q0.w;
        o.a[3] = q1.x; o.a[4] = q1.y; o.a[5] = q1.z; o.a[6] = q1.w;
        o.a[7] = q2.x; o.a[8] = q2.y; o.a[9] = q2.z; o.a[10] = q2.w;
        return o;
    }
    __device__ __forceinline__ void finish(Row& o, long long n) const { steps_row(sp, n, (int)o.cmd, o.a); }
    __device__ __forceinline__ bool prev_end(long long j, long long n, float& px, float& py) const {
        const float* pr = rows + j * FROW_W;
        if (!(pr[0] < (float)CMD_EOS)) return false;
        px = pr[1 + ARG_END];
        py = pr[2 + ARG_END];
        steps_point(sp, sp.of(n), px, py);
        return true;
    }
};

inline int steps_ok(const char* name, int32_t K, uint32_t kinds, const float* params, int32_t numericalize) {
    DSVG_CHECK_ARG(K >= 1 && K <= DSVG_MAX_STEPS, "%s: K = %d steps, need 1..%d", name, K, DSVG_MAX_STEPS);
    DSVG_CHECK_ARG(params, "%s: null step parameters", name);
    for (int k = 0; k < K; ++k)
        DSVG_CHECK_ARG(((kinds >> (2 * k)) & 3u) <= DSVG_STEP_ROTATE, "%s: step %d has no known kind", name, k);
    DSVG_CHECK_ARG(K == DSVG_MAX_STEPS || (kinds >> (2 * K)) == 0u, "%s: kinds has bits behind step %d", name, K - 1);
    DSVG_CHECK_ARG(numericalize >= 0 && numericalize <= (1 << 24), "%s: numericalize = %d, need 0 (off) .. 2^24", name,
                   numericalize);
    return 0;
}
}  // namespace

extern "C" int dsvg_paths_transform(const float* commands, const float* args, int64_t N, int32_t G, int32_t S, int32_t K,
                                    uint32_t kinds, const float* params, int32_t numericalize, float* out_args,
                                    void* stream) {
    DSVG_CHECK_ARG(commands && args && out_args, "paths_transform: null pointer");
    DSVG_CHECK_ARG(N > 0 && N < (1ll << 31) && G >= 1 && S >= 1 && (int64_t)G * S <= PT_MAX_ROWS,
                   "paths_transform: bad shape (N=%lld G=%d S=%d; G * S <= %d rows per icon)", (long long)N, G, S, PT_MAX_ROWS);
    if (steps_ok("paths_transform", K, kinds, params, numericalize)) return -1;
    hipLaunchKernelGGL(paths_transform_kernel, dim3((unsigned)N), dim3(PT_THREADS), 0, (hipStream_t)stream, commands, args, G,
                       S, StepProgram{K, kinds, params, numericalize}, out_args);
    DSVG_LAUNCH_CHECK("paths_transform");
    return 0;
}

extern "C" int dsvg_assemble_augmented(const float* rows, int64_t n_rows, const int32_t* slot_off, int64_t n_slots,
                                       const int32_t* variant, int64_t n_items, int32_t G, int32_t grouped, int32_t L,
                                       float pad_val, int32_t args_dim, int32_t K, uint32_t kinds, const float* params,
                                       int32_t numericalize, float* commands, float* args, float* args_rel, void* stream) {
    if (assemble_args_ok("assemble_augmented", rows, n_rows, slot_off, n_slots, variant, n_items, G, grouped, L, commands, 16))
        return -1;
    if (steps_ok("assemble_augmented", K, kinds, params, numericalize)) return -1;
    const long long n_seq = grouped ? n_items : n_items * G;
    hipLaunchKernelGGL(assemble_kernel<FloatRows>, dim3((unsigned)dsvg_cdiv(n_seq * L, 256)), dim3(256), 0,
                       (hipStream_t)stream, FloatRows{rows, StepProgram{K, kinds, params, numericalize}}, (long long)n_rows,
                       slot_off, (long long)n_slots, variant, G, grouped, n_seq, L, pad_val, (float)(args_dim - 1), commands,
                       args, args_rel);
    DSVG_LAUNCH_CHECK("assemble_augmented");
    return 0;
}
