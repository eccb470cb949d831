// Sequences of drawing commands on the device, stated once for csrc/metrics.hip (sample_points and its backward),
// csrc/raster.hip (the chords of an image and their backward), csrc/paths.hip (canonical path order),
// csrc/paths_expand.hip (commands split, arcs converted), csrc/paths_simplify.hip (Beziers fitted), csrc/paths_transform.hip
// (affine step programs), csrc/paths_fill.hip (overlap counts and filling) and csrc/assemble.hip (batch assembly): the command
// vocabulary, the argument mask and the argument columns of SVGTensor (deepsvg/difflib/tensor.py:8-41), the ballot prefix scan
// that gives every drawing command its output offset and the scans built on it, the prefix sum of counts for rows that become
// several, the count clamp of a cloud, the chord record with its crossing test, the orientation of a path, and the curve a
// drawing command draws with its transpose.
//
// The contracts that live here: the rasteriser's vertices are sample_points' points, and the backward kernels run on the
// forward's offsets.  A drawing command (`l`, `c`) of token t starts at the end position of the row before it, whatever that
// row holds, and at (0, 0) on row 0 of its sequence (tensor.py:75-82).  A `c` is evaluated in the power basis of CubicPower,
// Horner in z.  The straight line is NOT shared, on purpose: sample_points takes fma(z, p3 - p0, p0), the rasteriser the
// exact numerator ((n - 1 - q) p0 + q p3) / (n - 1) with vertex 0 and vertex n - 1 the start point and the end position bit for
// bit, so that consecutive chords share their vertices exactly; each kernel keeps its own.
#pragma once
#include "dsvg_common.h"

namespace {
// ---- vocabulary and layout -------------------------------------------------------------------------------------------
constexpr int CMD_M = 0, CMD_L = 1, CMD_C = 2, CMD_A = 3, CMD_EOS = 4, CMD_SOS = 5, CMD_Z = 6, N_CMD = 7;
constexpr int N_ARGS = 11;                // rx, ry, phi, fA, fS, control1 (x, y), control2 (x, y), end (x, y)
constexpr int ARG_CONTROL1 = 5, ARG_CONTROL2 = 7, ARG_END = 9;      // column of x; y is the column after it
// deepsvg/difflib/tensor.py:15-21, bit a of entry c = CMD_ARGS_MASK[c][a]
__device__ __constant__ uint32_t kCmdArgsMask[N_CMD] = {0x600u, 0x600u, 0x7E0u, 0x61Fu, 0u, 0u, 0u};

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_TOK = 2048;          // G * L tokens of one cloud / image / icon: 8 chunks of 256

// ---- the scan ----------------------------------------------------------------------------------------------------------
// Exclusive prefix count of a flag by one workgroup of SP_THREADS threads: a ballot per wave and chunk, then a prefix sum
// over the wave totals.  pre[t] = number of set flags among items < t, for t in 0..n (pre[n] = the total), 1 <= n <= MAXT (a
// multiple of SP_THREADS: the chunks are unrolled into registers); C = int, or a 16-bit type where LDS is short.  flag(t) is
// called by every thread for t < the chunk-rounded n and must return false past n.  wtot: one slot per wave of every chunk.
template <int MAXT, typename C, typename F>
__device__ __forceinline__ void block_flag_scan(int n, C* __restrict__ pre, int* __restrict__ wtot, F flag) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (n + SP_THREADS - 1) / SP_THREADS;
    int below[MAXT / SP_THREADS];           // flags below this lane inside its wave, per chunk (unrolled: registers)
#pragma unroll
    for (int c = 0; c < MAXT / SP_THREADS; ++c) {
        below[c] = 0;
        if (c < n_chunks) {
            const unsigned long long b = __ballot(flag(c * SP_THREADS + tid));
            below[c] = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) wtot[c * (SP_THREADS / 64) + wave] = __popcll(b);
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXT / SP_THREADS; ++c) {
        if (c < n_chunks) {
            const int w = c * (SP_THREADS / 64) + wave;
            int base = 0;
            for (int q = 0; q < w; ++q) base += wtot[q];      // <= 31 broadcast reads
            const int t = c * SP_THREADS + tid;
            if (t < n) pre[t] = (C)(base + below[c]);
            if (t == n - 1) {
                int tot = base;
                for (int q = w; q < n_chunks * (SP_THREADS / 64); ++q) tot += wtot[q];
                pre[n] = (C)tot;
            }
        }
    }
    __syncthreads();
}

// Exclusive prefix SUM of a non-negative count by one workgroup of SP_THREADS threads, for the kernels where an item becomes
// 0..k output rows (csrc/paths_expand.hip, csrc/paths_simplify.hip): an inclusive shuffle scan per wave and chunk, then the
// prefix over the wave totals as above.  pre[t] = sum of count(i) over items i < t, for t in 0..n (pre[n] = the total); the caller keeps n times the
// largest count below 2^31.  count(t) is called by every thread for t < the chunk-rounded n and must return 0 past n.
template <int MAXT, typename F>
__device__ __forceinline__ void block_count_sum(int n, int* __restrict__ pre, int* __restrict__ wtot, F count) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (n + SP_THREADS - 1) / SP_THREADS;
    int below[MAXT / SP_THREADS];           // counts below this lane inside its wave, per chunk (unrolled: registers)
#pragma unroll
    for (int c = 0; c < MAXT / SP_THREADS; ++c) {
        below[c] = 0;
        if (c < n_chunks) {
            const int v = count(c * SP_THREADS + tid);
            int inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(inc, d, 64);
                if (lane >= d) inc += up;
            }
            below[c] = inc - v;
            if (lane == 63) wtot[c * (SP_THREADS / 64) + wave] = inc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXT / SP_THREADS; ++c) {
        if (c < n_chunks) {
            const int w = c * (SP_THREADS / 64) + wave;
            int base = 0;
            for (int q = 0; q < w; ++q) base += wtot[q];
            const int t = c * SP_THREADS + tid;
            if (t < n) pre[t] = base + below[c];
            if (t == n - 1) {
                int tot = base;
                for (int q = w; q < n_chunks * (SP_THREADS / 64); ++q) tot += wtot[q];
                pre[n] = tot;
            }
        }
    }
    __syncthreads();
}

// The three flags the geometry kernels scan with block_flag_scan<SP_MAX_TOK> over int counts, forward and backward alike.
// They are predicates called from a [&] lambda at the scan: a function that wraps the scan, or one that returns the lambda,
// moves the registers of sample_points_kernel and sample_points_bwd_kernel.
// pre[t] = drawing commands (`l`, `c`) among the tokens before t: token t of the T_ tokens at cmd draws
template <typename T>
__device__ __forceinline__ bool is_drawing(const T* cmd, int t, int T_) {
    if (t >= T_) return false;
    const int c = (int)cmd[t];
    return c == CMD_L || c == CMD_C;
}
// full[g] = sequences with at least one drawing command among the sequences before g: sequence g of G has one
__device__ __forceinline__ bool sequence_draws(const int* pre, int g, int G, int L) {
    return g < G && pre[(g + 1) * L] > pre[g * L];
}
// cl[t] = sub-paths that end before token t (fill mode; all zero otherwise): a sub-path ends at a drawing token that is the
// last row of its sequence or has a non-drawing row after it
__device__ __forceinline__ bool subpath_ends(const int* pre, int t, const int& T_, const int& L, const int& fill) {
    if (!fill || t >= T_ || pre[t + 1] == pre[t]) return false;
    return t % L == L - 1 || pre[t + 2] == pre[t + 1];
}

// ---- the count clamp: the points (records) in use of cloud b, whatever n[b] holds ------------------------------------
__device__ __forceinline__ int chamfer_count(const int32_t* n, long long b, long long cap) {
    return (int)min((long long)max(n[b], 0), cap);
}

// ---- chord records and the crossing test (csrc/raster.hip writes and sweeps them, csrc/paths_fill.hip counts with them) ----
constexpr int RS_REC = 5;                 // words of a chord record: ax, ay, bx - ax, by - ay, flags
constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 32;               // pixels per side of a workgroup's tile
constexpr int RS_QUAD = 16;               // pixels per side of a wave's quadrant
constexpr int RS_PIX = 4;                 // pixels of a lane: rows ly, ly + 4, ly + 8, ly + 12 of its quadrant
constexpr int RS_CHORDS = 512;            // chords per LDS tile (16 KiB of records, 8 KiB of boxes when culling)

// The y of record j's end vertex AS THE NEXT CHORD HOLDS IT: the a of the record after it, on a closing chord (flags word fl,
// bits 1.. = records back) the a of its sub-path's first record.  ay + dy is that value only up to rounding, and the half-open
// rule below is watertight only when a shared vertex is one number.  Records that break the rule of include/dsvg.h keep
// ay + dy: in bounds, not watertight.
__device__ __forceinline__ float chord_end_y(const float* sg, int j, int cnt, float ay, float dy, int fl) {
    float by = ay + dy;
    const int back = (int)((unsigned)fl >> 1);
    if (back > 0 && back <= j) by = sg[(long long)(j - back) * RS_REC + 1];
    else if (back == 0 && j + 1 < cnt) by = sg[(long long)(j + 1) * RS_REC + 1];
    return by;
}

// The sign test of the crossing rule.  The chord a -> b (dx, dy = b - a as stored; ay, by its vertices' y, by from chord_end_y)
// adds to the winding count of the sample at a + (px, py) on the row cy, on a ray towards +x with the half-open rule: the
// crossing of the chord's line with the row lies at x > cx when e > 0 going down the image (ay <= cy < by), e < 0 going up
// (by <= cy < ay).  e = fmaf(dx, py, -p) with p = fl(dy px) is the sweeps' test.  It rounds one product and not the other, so for
// a sample ON the chord's line (an end position of an integer icon under an integer sample centre, a chord's midpoint) it
// returns the rounding residual of p, of either sign: a crossing that lies at x == cx is counted or not by chance.  In an
// image that cannot be seen (the coverage there is 0.5 -+ d / s with d zero up to rounding); a sample count is off by one.
// COMPENSATED (csrc/paths_fill.hip only) subtracts that residual, r = fmaf(dy, px, -p) = dy px - p, which fp32 holds exactly
// unless it underflows (|dy px| below 2^-102: r is then flushed and e is the sweeps' value): e = fl(fl(dx py - p) - r).
// With E = dx py - dy px the true value for the fp32 px, py: E == 0 gives e == 0 (dx py - p equals r, a float, and both
// roundings are exact); otherwise e has the sign of E or is 0 (rounding is monotone), and 0 only where |E| is below the
// rounding of dx py - p while that is about |r| <= ulp(p) / 2: |E| <= 2^-24 ulp(p) <= 2^-47 |dy px| - far inside the band in
// which the rounding of px and py decides anyway.
template <bool COMPENSATED = false>
__device__ __forceinline__ float chord_side(float dx, float dy, float px, float py) {
    if constexpr (COMPENSATED) {
        const float p = dy * px;
        return fmaf(dx, py, -p) - fmaf(dy, px, -p);
    } else {
        return fmaf(dx, py, -(dy * px));
    }
}
// (The half-open count itself, (ay <= cy && cy < by && e > 0) - (by <= cy && cy < ay && e < 0), stays written out in the
// three kernels: as a function, with or without the sign test inside, hipcc schedules the two fill sweeps without culling
// differently.)

// ---- orientation (SVGPath.is_clockwise, svglib/svg_path.py:244-252) ------------------------------------------------------
// one command's term of the determinant sum, start (sx, sy) -> end (fx, fy): float64, no fused multiply-add (tests/paths_ref.py
// and tests/paths_fill_ref.py restate it operation by operation)
__device__ __forceinline__ double orientation_term(float sx, float sy, float fx, float fy) {
#pragma clang fp contract(off)
    return (double)sx * (double)fy - (double)sy * (double)fx;
}
// a path of one command is clockwise when start <= end lexicographically, any other when the sum of its terms is >= 0
__device__ __forceinline__ bool single_command_clockwise(float sx, float sy, float fx, float fy) {
    return sx < fx || (sx == fx && sy <= fy);
}

// ---- curve evaluation ----------------------------------------------------------------------------------------------------
// start point of the token whose argument row is `a`, row i of its sequence
template <typename T>
__device__ __forceinline__ float2 start_point(const T* a, int i) {
    return make_float2(i ? (float)a[ARG_END - N_ARGS] : 0.f, i ? (float)a[ARG_END + 1 - N_ARGS] : 0.f);
}

// power basis of the cubic Bezier p0..p3 (exact for integer arguments), Horner in z
struct CubicPower {
    float c1x = 0.f, c1y = 0.f, c2x = 0.f, c2y = 0.f, c3x = 0.f, c3y = 0.f;
    CubicPower() = default;
    template <typename T>
    __device__ __forceinline__ CubicPower(float2 p0, const T* a, float p3x, float p3y) {
        const float p1x = (float)a[ARG_CONTROL1], p1y = (float)a[ARG_CONTROL1 + 1];
        const float p2x = (float)a[ARG_CONTROL2], p2y = (float)a[ARG_CONTROL2 + 1];
        c1x = 3.f * (p1x - p0.x); c2x = 3.f * (p0.x - 2.f * p1x + p2x); c3x = (p3x - p0.x) + 3.f * (p1x - p2x);
        c1y = 3.f * (p1y - p0.y); c2y = 3.f * (p0.y - 2.f * p1y + p2y); c3y = (p3y - p0.y) + 3.f * (p1y - p2y);
    }
    __device__ __forceinline__ float2 eval(float2 p0, float z) const {
        return make_float2(fmaf(fmaf(fmaf(c3x, z, c2x), z, c1x), z, p0.x), fmaf(fmaf(fmaf(c3y, z, c2y), z, c1y), z, p0.y));
    }
};

// The transpose: the gradient of one argument row, float64 sums of the gradients (vx, vy) of the curve's vertices times the
// Bernstein weights CubicPower evaluates (`c`) or (1 - z, z) (`l`); the result is the float32 nearest to the exact sum.
struct ArgRowGrad {
    double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0, ex = 0.0, ey = 0.0;
    // the vertex at z of this row's own command: control1, control2, end.  (V: float or double, widened where it is used)
    template <typename V>
    __device__ __forceinline__ void own(bool cubic, double z, V vx, V vy) {
        const double w = 1.0 - z;
        if (cubic) {
            const double w1 = 3.0 * w * w * z, w2 = 3.0 * w * z * z, w3 = z * z * z;
            c1x += w1 * (double)vx; c1y += w1 * (double)vy;
            c2x += w2 * (double)vx; c2y += w2 * (double)vy;
            ex += w3 * (double)vx; ey += w3 * (double)vy;
        } else {
            ex += z * (double)vx; ey += z * (double)vy;
        }
    }
    // the vertex at z of the command on the row after this one: its start point is this row's end position
    template <typename V>
    __device__ __forceinline__ void next_start(bool cubic, double z, V vx, V vy) {
        const double w = 1.0 - z;
        const double w0 = cubic ? w * w * w : w;
        ex += w0 * (double)vx; ey += w0 * (double)vy;
    }
    // every element of the row is written
    __device__ __forceinline__ void store(float* row) const {
#pragma unroll
        for (int q = 0; q < ARG_CONTROL1; ++q) row[q] = 0.f;
        row[ARG_CONTROL1] = (float)c1x; row[ARG_CONTROL1 + 1] = (float)c1y;
        row[ARG_CONTROL2] = (float)c2x; row[ARG_CONTROL2 + 1] = (float)c2y;
        row[ARG_END] = (float)ex; row[ARG_END + 1] = (float)ey;
    }
};

// ---- host: the (B, G, L, n) arguments dsvg_sample_points, dsvg_raster_segments and their backwards share, refused under the
// name of the caller; `noun` is what a workgroup builds from its G * L tokens ("cloud", "image")
inline int sequence_args_ok(const char* name, const char* noun, int64_t B, int32_t G, int32_t L, int32_t n) {
    DSVG_CHECK_ARG(n >= 2 && n <= 64, "%s: n = %d points per command, need 2..64", name, n);
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && G >= 1 && L >= 1 && (int64_t)G * L <= SP_MAX_TOK,
                   "%s: bad shape (B=%lld G=%d L=%d; G * L <= %d tokens per %s)", name, (long long)B, G, L, SP_MAX_TOK, noun);
    return 0;
}
}  // namespace
