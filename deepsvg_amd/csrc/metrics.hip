// Reconstruction error of decoded icons and its gradient: points sampled on the curves of a command sequence
// (SVGTensor.sample_points, deepsvg/difflib/tensor.py:191-230) and the Chamfer distance between two such clouds
// (chamfer_loss, deepsvg/difflib/loss.py:5-7), forward and backward.
//
// The reference samples one path at a time on the host and takes the Chamfer distance from the full torch.cdist matrix
// (512 icons of ~2,400 points: 11.8 GB of fp32 distances).  Here:
//   dsvg_sample_points  one workgroup per cloud (the G sequences of an icon, in group order): a ballot + prefix sum gives
//                       every drawing command its output offset, then the (command, sample) pairs are evaluated by
//                       consecutive lanes, so the stores are contiguous.  float32 or int64 inputs are read as they are.
//   dsvg_chamfer        one workgroup per (icon, direction, slice of 1,024 points): each thread keeps up to 4 points of one
//                       cloud in registers, the other cloud streams through LDS in tiles (every lane reads the same
//                       address: a broadcast), running minimum of the SQUARED distance, one sqrt per point after the
//                       sweep; a one-thread-per-icon finish launch adds the slices in a fixed order.  No distance matrix,
//                       no atomics.
//   dsvg_chamfer_nn     the same sweep, instantiated a second time, that also keeps the arg-min index (strict <: the lowest index
//                       wins a tie); same minima, same sums, same finish launch, so `out` has dsvg_chamfer's bits.
//   dsvg_chamfer_bwd    the same decomposition: a thread keeps up to 4 points of its cloud and their direct terms
//                       u(x_i, y_j*(i)) / n_x in registers; the other cloud streams through LDS as (c_j, i*(j)) with
//                       c_j = u(x_i*(j), y_j) / n_y computed once by the loading thread; every thread adds the c_j whose index
//                       is one of its points, in ascending j.  No atomics, no workspace, no [n_x, n_y] buffer.
//   dsvg_sample_points_bwd  one workgroup per cloud, one thread per token: sample_points is linear in the arguments, so
//                       a token gathers the weighted sums of its own samples' gradients (columns 5..10) and the start-point
//                       share of the row after it (columns 9, 10), in float64, and writes all 11 columns of its row.
#include "dsvg_common.h"
#include "svg_seq.h"             // vocabulary, block_flag_scan and its scans, chamfer_count, the curve and its transpose
#include "../../include/dsvg.h"

namespace {
template <typename T>
__global__ __launch_bounds__(SP_THREADS) void sample_points_kernel(const T* __restrict__ commands, const T* __restrict__ args,
                                                                   int G, int L, int n, long long cap,
                                                                   float* __restrict__ points, int32_t* __restrict__ counts) {
    __shared__ int pre[SP_MAX_TOK + 1];       // drawing commands of the cloud before token t
    __shared__ int full[SP_MAX_TOK + 1];      // sequences with at least one drawing command before sequence g
    __shared__ int src[SP_MAX_TOK];           // token of the j-th drawing command
    __shared__ int wtot[SP_MAX_TOK / 64];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int T_ = G * L;
    const T* cmd = commands + b * T_;
    const T* arg = args + b * T_ * N_ARGS;

    // ---- pass 1: where every drawing command's points go -----------------------------------------------------------
    block_flag_scan<SP_MAX_TOK>(T_, pre, wtot, [&](int t) { return is_drawing(cmd, t, T_); });
    block_flag_scan<SP_MAX_TOK>(G, full, wtot, [&](int g) { return sequence_draws(pre, g, G, L); });
    for (int t = tid; t < T_; t += SP_THREADS)
        if (pre[t + 1] > pre[t]) src[pre[t]] = t;
    __syncthreads();
    const int K = pre[T_];
    if (tid == 0) counts[b] = K * (n - 1) + full[G];      // k (n - 1) + 1 points per sequence with k > 0 drawing commands

    // ---- pass 2: work item (j, k) = sample k of the j-th drawing command; k = n - 1 only on a sequence's last one --------
    float* out = points + b * cap * 2;
    for (int w = tid; w < K * n; w += SP_THREADS) {
        const int j = w / n, k = w - j * n;
        const int t = src[j];
        const int g = t / L, i = t - g * L;
        const bool last = j + 1 == pre[(g + 1) * L];
        if (k == n - 1 && !last) continue;
        const T* a = arg + (long long)t * N_ARGS;
        const float2 p0 = start_point(a, i);
        const float p3x = (float)a[ARG_END], p3y = (float)a[ARG_END + 1];
        const float z = (float)k / (float)(n - 1);
        float2 v;
        if ((int)cmd[t] == CMD_L) v = make_float2(fmaf(z, p3x - p0.x, p0.x), fmaf(z, p3y - p0.y, p0.y));
        else v = CubicPower(p0, a, p3x, p3y).eval(p0, z);
        const long long o = (long long)pre[t] * (n - 1) + full[g] + k;
        reinterpret_cast<float2*>(out)[o] = v;
    }
}

// Backward of sample_points_kernel<float>: dargs[b, t, :] from dpoints[b, :, :].  The offsets are the forward's; a token
// reads the gradients of its own samples (weights of control1, control2, end) and those of the row after it (weight of
// the start point, which is this row's end position whatever this row holds; row 0's start is the constant (0, 0)).
// Weights and sums in float64: the result is the float32 nearest to the exact sum (fp32 sums of up to 2 n products of
// weights <= 1 could pass n * 2^-22 * max|dP| only on average, not in the worst case).  Every element of the row is written.
// A thread runs two serial loops of up to n 8-byte loads.
__global__ __launch_bounds__(SP_THREADS) void sample_points_bwd_kernel(const float* __restrict__ commands, int G, int L, int n,
                                                                       long long cap, const float* __restrict__ dpoints,
                                                                       float* __restrict__ dargs) {
    __shared__ int pre[SP_MAX_TOK + 1];
    __shared__ int full[SP_MAX_TOK + 1];
    __shared__ int wtot[SP_MAX_TOK / 64];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int T_ = G * L;
    const float* cmd = commands + b * T_;
    block_flag_scan<SP_MAX_TOK>(T_, pre, wtot, [&](int t) { return is_drawing(cmd, t, T_); });
    block_flag_scan<SP_MAX_TOK>(G, full, wtot, [&](int g) { return sequence_draws(pre, g, G, L); });
    const float2* dp = reinterpret_cast<const float2*>(dpoints) + b * cap;
    float* out = dargs + b * T_ * N_ARGS;
    const double step = 1.0 / (double)(n - 1);
    for (int t = tid; t < T_; t += SP_THREADS) {
        const int g = t / L, i = t - g * L;
        const int n_draw = pre[(g + 1) * L];              // drawing commands up to the end of this sequence
        ArgRowGrad acc;
        const int c = (int)cmd[t];
        if (c == CMD_L || c == CMD_C) {
            const long long o = (long long)pre[t] * (n - 1) + full[g];
            const int cnt = pre[t] + 1 == n_draw ? n : n - 1;
            for (int k = 0; k < cnt; ++k) {
                const float2 d = dp[o + k];
                acc.own(c == CMD_C, (double)k * step, d.x, d.y);
            }
        }
        if (i + 1 < L) {
            const int c_next = (int)cmd[t + 1];
            if (c_next == CMD_L || c_next == CMD_C) {
                const long long o = (long long)pre[t + 1] * (n - 1) + full[g];
                const int cnt = pre[t + 1] + 1 == n_draw ? n : n - 1;
                for (int k = 0; k < cnt; ++k) {
                    const float2 d = dp[o + k];
                    acc.next_start(c_next == CMD_C, (double)k * step, (double)d.x, (double)d.y);
                }
            }
        }
        acc.store(out + (long long)t * N_ARGS);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int CH_THREADS = 256;
constexpr int CH_WAVES = CH_THREADS / 64;
constexpr int CH_R = 4;                   // chunks of 64 points a wave keeps in registers (one point per lane and chunk)
constexpr int CH_SLICE = CH_WAVES * CH_R * 64;      // points of one cloud per workgroup: 1,024
constexpr int CH_TILE = 1024;             // points of the other cloud per LDS tile (8 KiB)

// running minimum of the squared distance from R register points to the first cnt4 (a multiple of 4) points of the tile.
// NN: a[r] = the index (j0 + position in the tile) of the first point that reached m[r]; the copies of the last point that
// pad a tile can never win: strict <.  (`a` and j0 are not touched without NN.)
template <bool NN, int R>
__device__ __forceinline__ void chamfer_sweep(const float4* __restrict__ tile, int cnt4, int j0, const float2 (&x)[CH_R],
                                              float (&m)[CH_R], int (&a)[CH_R]) {
#pragma unroll 2
    for (int jj = 0; jj < cnt4 / 2; jj += 2) {
        const float4 q0 = tile[jj], q1 = tile[jj + 1];        // 4 points, the same address in every lane
        const int j = j0 + 2 * jj;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // (written out four times: a loop or a lambda over the four points schedules the arg-min kernel differently)
            float dx = x[r].x - q0.x, dy = x[r].y - q0.y;
            float d = fmaf(dx, dx, dy * dy);
            if constexpr (NN) { if (d < m[r]) { m[r] = d; a[r] = j; } } else m[r] = fminf(m[r], d);
            dx = x[r].x - q0.z; dy = x[r].y - q0.w;
            d = fmaf(dx, dx, dy * dy);
            if constexpr (NN) { if (d < m[r]) { m[r] = d; a[r] = j + 1; } } else m[r] = fminf(m[r], d);
            dx = x[r].x - q1.x; dy = x[r].y - q1.y;
            d = fmaf(dx, dx, dy * dy);
            if constexpr (NN) { if (d < m[r]) { m[r] = d; a[r] = j + 2; } } else m[r] = fminf(m[r], d);
            dx = x[r].x - q1.z; dy = x[r].y - q1.w;
            d = fmaf(dx, dx, dy * dy);
            if constexpr (NN) { if (d < m[r]) { m[r] = d; a[r] = j + 3; } } else m[r] = fminf(m[r], d);
        }
    }
}

// Workgroup (icon b, direction d, slice s): sum_i min_j |x_i - y_j| over the points i of slice s of cloud x (d = 0: x = px,
// y = py; d = 1: the roles swapped - the same code on swapped pointers, so chamfer(x, y) and chamfer(y, x) add the same
// numbers).  The 16 chunks of 64 points of a slice are dealt round-robin to the 4 waves, up to CH_R chunks per wave in
// registers; y streams through the LDS tile.  part[(b * 2 + d) * n_slices + s] takes the sum; slices past the cloud's end
// and icons with an empty cloud write nothing (the finish kernel does not read them).
// NN: also idx_x[b, i] = arg-min_j |x_i - y_j| (d = 0) / idx_y[b, j] = arg-min_i |x_i - y_j| (d = 1) for the points in use
// (idx_x / idx_y are not touched without NN); `part` takes the same numbers.  Both instantiations have, instruction for
// instruction and in VGPRs, SGPRs, LDS and scratch, the code of the two separate kernels they replace
// (profiles/geometry_header_isa.log); tests/test_metrics_grad_gpu.py compares the two outputs in bits.
template <bool NN>
__global__ __launch_bounds__(CH_THREADS) void chamfer_slice_kernel(const float* __restrict__ px, const int32_t* __restrict__ nx,
                                                                   long long capx, const float* __restrict__ py,
                                                                   const int32_t* __restrict__ ny, long long capy,
                                                                   int n_slices, double* __restrict__ part,
                                                                   int32_t* __restrict__ idx_x, int32_t* __restrict__ idx_y) {
    __shared__ __attribute__((aligned(16))) float2 tile[CH_TILE];
    __shared__ double red[CH_WAVES];
    const long long blk = blockIdx.x;
    const int s = (int)(blk % n_slices);
    const long long bd = blk / n_slices, b = bd >> 1;
    const bool swap = bd & 1;
    const int cx = chamfer_count(nx, b, capx), cy = chamfer_count(ny, b, capy);
    const int n_x = swap ? cy : cx, n_y = swap ? cx : cy;
    if (n_x == 0 || n_y == 0 || (long long)s * CH_SLICE >= n_x) return;      // (block-uniform)
    const float2* x = reinterpret_cast<const float2*>(swap ? py : px) + b * (swap ? capy : capx);
    const float2* y = reinterpret_cast<const float2*>(swap ? px : py) + b * (swap ? capx : capy);
    int32_t* idx = (swap ? idx_y : idx_x) + b * (swap ? capy : capx);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (n_x + 63) >> 6;

    float2 xr[CH_R];
    float m[CH_R];
    int am[CH_R];
    int nr = 0;                                        // chunks of this wave (wave-uniform)
#pragma unroll
    for (int r = 0; r < CH_R; ++r) {
        const int c = s * (CH_SLICE / 64) + r * CH_WAVES + wave;
        if (c < n_chunks) nr = r + 1;
        xr[r] = x[min(c * 64 + lane, n_x - 1)];
        m[r] = INFINITY;
        am[r] = 0;
    }
    for (int j0 = 0; j0 < n_y; j0 += CH_TILE) {
        if (j0) __syncthreads();                       // the tile of the step before has been read
#pragma unroll
        for (int h = 0; h < CH_TILE / CH_THREADS; ++h)          // past n_y: the last point again (it cannot move a minimum)
            tile[h * CH_THREADS + tid] = y[min(j0 + h * CH_THREADS + tid, n_y - 1)];
        __syncthreads();
        const int cnt4 = (min(CH_TILE, n_y - j0) + 3) & ~3;
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        switch (nr) {
            case 4: chamfer_sweep<NN, 4>(t4, cnt4, j0, xr, m, am); break;
            case 3: chamfer_sweep<NN, 3>(t4, cnt4, j0, xr, m, am); break;
            case 2: chamfer_sweep<NN, 2>(t4, cnt4, j0, xr, m, am); break;
            case 1: chamfer_sweep<NN, 1>(t4, cnt4, j0, xr, m, am); break;
            default: break;
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < CH_R; ++r) {
        const int c = s * (CH_SLICE / 64) + r * CH_WAVES + wave;
        if (c < n_chunks && c * 64 + lane < n_x) {
            sum += sqrtf(m[r]);
            if constexpr (NN) idx[c * 64 + lane] = am[r];
        }
    }
    // fixed-order sum: butterfly inside the wave, then the waves in ascending order
    double t = (double)sum;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) red[wave] = t;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < CH_WAVES; ++w) tot += red[w];
        part[blk] = tot;
    }
}

// out[b] = mean over x + mean over y: the slices of each direction in ascending order, one thread per icon
__global__ __launch_bounds__(256) void chamfer_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ nx,
                                                             long long capx, const int32_t* __restrict__ ny, long long capy,
                                                             int n_slices, long long B, float* __restrict__ out) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int cnt[2] = {chamfer_count(nx, b, capx), chamfer_count(ny, b, capy)};
    if (cnt[0] == 0 || cnt[1] == 0) {                   // the mean over an empty set
        out[b] = __builtin_nanf("");
        return;
    }
    float mean[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double* p = part + (b * 2 + d) * n_slices;
        double tot = 0.0;
        for (int s = 0; s < (cnt[d] + CH_SLICE - 1) / CH_SLICE; ++s) tot += p[s];
        mean[d] = (float)(tot / (double)cnt[d]);
    }
    out[b] = mean[0] + mean[1];
}

// (a - b) / (|a - b| cnt); 0 where a == b (and where a coordinate is NaN)
__device__ __forceinline__ float2 chamfer_unit_over(float2 a, float2 b, float cnt) {
    const float dx = a.x - b.x, dy = a.y - b.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    if (!(d2 > 0.f)) return make_float2(0.f, 0.f);
    const float den = sqrtf(d2) * cnt;
    return make_float2(dx / den, dy / den);
}

constexpr int CB_R = CH_SLICE / CH_THREADS;       // points of its cloud a thread owns: rows s * 1,024 + r * 256 + tid

// Workgroup (icon b, direction d, slice s) writes rows s * 1,024 .. + 1,023 of dpx[b] (d = 0) or of dpy[b] (d = 1: the same
// code on swapped pointers, so d chamfer(x, y) / dx and the second gradient of chamfer(y, x) are the same numbers):
//   d out / d x_i = u(x_i, y_j*(i)) / n_x + sum over {j : i*(j) = i} of u(x_i, y_j) / n_y,   times dout[b]
// with j* = ix, i* = iy the arg-min indices of the forward (clamped into their cloud here: a bad index cannot leave it).
// Rows past the count are zero; so is every row of an icon with an empty cloud, whatever dout[b] holds.
__global__ __launch_bounds__(CH_THREADS) void chamfer_bwd_kernel(const float* __restrict__ px, const int32_t* __restrict__ nx,
                                                                 long long capx, const float* __restrict__ py,
                                                                 const int32_t* __restrict__ ny, long long capy,
                                                                 const int32_t* __restrict__ idx_x,
                                                                 const int32_t* __restrict__ idx_y, const float* __restrict__ dout,
                                                                 int n_slices, float* __restrict__ dpx, float* __restrict__ dpy) {
    __shared__ __attribute__((aligned(16))) float4 tile[CH_TILE];      // (c_j.x, c_j.y, i*(j), -)
    const long long blk = blockIdx.x;
    const int s = (int)(blk % n_slices);
    const long long bd = blk / n_slices, b = bd >> 1;
    const bool swap = bd & 1;
    const long long cap_x = swap ? capy : capx, cap_y = swap ? capx : capy;
    const long long row0 = (long long)s * CH_SLICE;
    if (row0 >= cap_x) return;                                         // (block-uniform)
    const int tid = threadIdx.x;
    const int cx = chamfer_count(nx, b, capx), cy = chamfer_count(ny, b, capy);
    const int n_x = swap ? cy : cx, n_y = swap ? cx : cy;
    float2* g = reinterpret_cast<float2*>(swap ? dpy : dpx) + b * cap_x;
    if (n_x == 0 || n_y == 0 || row0 >= n_x) {                         // nothing in use in these rows (block-uniform)
#pragma unroll
        for (int r = 0; r < CB_R; ++r) {
            const long long i = row0 + r * CH_THREADS + tid;
            if (i < cap_x) g[i] = make_float2(0.f, 0.f);
        }
        return;
    }
    const float2* x = reinterpret_cast<const float2*>(swap ? py : px) + b * cap_x;
    const float2* y = reinterpret_cast<const float2*>(swap ? px : py) + b * cap_y;
    const int32_t* ix = (swap ? idx_y : idx_x) + b * cap_x;
    const int32_t* iy = (swap ? idx_x : idx_y) + b * cap_y;
    const float fx = (float)n_x, fy = (float)n_y;

    float2 acc[CB_R];
    int mine[CB_R];
#pragma unroll
    for (int r = 0; r < CB_R; ++r) {
        const int i = (int)row0 + r * CH_THREADS + tid;
        acc[r] = make_float2(0.f, 0.f);
        mine[r] = -1;
        if (i < n_x) {
            const int j = min(max(ix[i], 0), n_y - 1);
            acc[r] = chamfer_unit_over(x[i], y[j], fx);
            mine[r] = i;
        }
    }
    for (int j0 = 0; j0 < n_y; j0 += CH_TILE) {
        if (j0) __syncthreads();
#pragma unroll
        for (int h = 0; h < CH_TILE / CH_THREADS; ++h) {
            const int jl = h * CH_THREADS + tid, j = j0 + jl;
            float4 e = make_float4(0.f, 0.f, __int_as_float(-2), 0.f);
            if (j < n_y) {
                const int i = min(max(iy[j], 0), n_x - 1);
                const float2 c = chamfer_unit_over(x[i], y[j], fy);
                e = make_float4(c.x, c.y, __int_as_float(i), 0.f);
            }
            tile[jl] = e;
        }
        __syncthreads();
        const int cnt = min(CH_TILE, n_y - j0);
        for (int jl = 0; jl < cnt; ++jl) {
            const float4 e = tile[jl];                    // the same address in every lane
            const int i = __float_as_int(e.z);
#pragma unroll
            for (int r = 0; r < CB_R; ++r) {
                const bool hit = i == mine[r];
                acc[r].x += hit ? e.x : 0.f;
                acc[r].y += hit ? e.y : 0.f;
            }
        }
    }
    const float d = dout[b];
#pragma unroll
    for (int r = 0; r < CB_R; ++r) {
        const long long i = row0 + r * CH_THREADS + tid;
        if (i < cap_x) g[i] = mine[r] >= 0 ? make_float2(d * acc[r].x, d * acc[r].y) : make_float2(0.f, 0.f);
    }
}

inline int64_t chamfer_slices(int64_t capx, int64_t capy) {
    return ((capx > capy ? capx : capy) + CH_SLICE - 1) / CH_SLICE;
}

// ---------------------------------------------------------------------------------------------------------------------
// The ordered losses of deepsvg/difflib/loss.py: svg_emd_loss (:21-51) and the polyline length behind svg_length_loss /
// continuity_loss (:10-18).  Lengths, the orientation sum and the shift sums are float64 so that every choice (flip, match,
// shift) is a property of the input and not of a summation order.
constexpr int EM_THREADS = 256;
constexpr int EM_WAVES = EM_THREADS / 64;
constexpr int EM_PER = 4;                              // consecutive target points of a chunk per thread
constexpr int EM_CHUNK = EM_THREADS * EM_PER;          // target points per chunk of the arc-length scan: 1,024
constexpr int EM_SHIFTS = 256;                         // shifts per workgroup of emd_shift_kernel, one per thread
constexpr int EM_KTILE = 1024;                         // pred points per LDS tile of emd_shift_kernel
constexpr int EM_MAX_N = 65536;                        // pred points per cloud (the shift search is quadratic in them)

__device__ __forceinline__ double segment_length(float2 a, float2 b) {
    const double dx = (double)b.x - (double)a.x, dy = (double)b.y - (double)a.y;
    return sqrt(dx * dx + dy * dy);
}

// the sum of v over the workgroup, in a fixed order (butterfly inside the wave, the waves ascending), in every thread
__device__ __forceinline__ double block_sum_f64(double v, double* __restrict__ red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                   // red of a call before has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < EM_WAVES; ++w) tot += red[w];
    return tot;
}

// v[r] -> the inclusive prefix sum over the workgroup's EM_CHUNK items (thread tid holds items 4 tid .. 4 tid + 3): the sums
// inside a thread, plus the totals of the threads before it added from left to right.  What a thread starts from is the
// last sum of the thread before it, bit for bit, so the sums never decrease, and the returned chunk total is the last
// item's sum.  sc: EM_THREADS doubles.
__device__ __forceinline__ double block_scan_f64(double (&v)[EM_PER], double* __restrict__ sc) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 1; r < EM_PER; ++r) v[r] += v[r - 1];
    __syncthreads();                                   // sc of a call before has been read
    sc[tid] = v[EM_PER - 1];
    __syncthreads();
    double run = 0.0, before = 0.0;
    for (int q = 0; q < EM_THREADS; ++q) {             // the same address in every lane
        if (q == tid) before = run;
        run += sc[q];
    }
#pragma unroll
    for (int r = 0; r < EM_PER; ++r) v[r] += before;
    return run;
}

// the first slot in [lo, hi] whose value is >= u; d[hi] >= u is known
__device__ __forceinline__ int lower_slot(const double* __restrict__ d, int lo, int hi, double u) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d[mid] >= u) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Workgroup b: orientation of the target, its normalised arc-length distribution D (chunk by chunk, never stored), and
// for every pred point i the target point whose D is nearest to u_i = i / (n - 1) (the lowest index of a tie):
//   match[b, i] = that point's index into the target AS PASSED, t[b, i] = its coordinates.
// An icon with an empty cloud writes nothing.
__global__ __launch_bounds__(EM_THREADS) void emd_match_kernel(const int32_t* __restrict__ nx, long long capx,
                                                               const float* __restrict__ py, const int32_t* __restrict__ ny,
                                                               long long capy, int32_t* __restrict__ match,
                                                               float* __restrict__ t) {
    __shared__ double Dl[EM_CHUNK + 1];                // slot 0: the last D of the chunk before; slot 1 + q: D of item j0 + q
    __shared__ double sc[EM_THREADS];
    __shared__ double red[EM_WAVES];
    __shared__ double total_sh;
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = chamfer_count(nx, b, capx), m = chamfer_count(ny, b, capy);
    if (n == 0 || m == 0) return;                      // (block-uniform)
    const float2* y = reinterpret_cast<const float2*>(py) + b * capy;
    int32_t* mt = match + b * capx;
    float2* tt = reinterpret_cast<float2*>(t) + b * capx;

    // orientation: the open polyline's shoelace sum (utils.py:52-60); not (A > 0) reverses
    double a = 0.0;
    for (int j = tid; j < m - 1; j += EM_THREADS) {
        const float2 p = y[j], q = y[j + 1];
        a += (double)p.x * (double)q.y - (double)q.x * (double)p.y;
    }
    const bool flip = !(block_sum_f64(a, red) > 0.0);
    auto yo = [&](int j) { return y[flip ? m - 1 - j : j]; };
    auto item = [&](int j) { return j >= 1 && j < m ? segment_length(yo(j - 1), yo(j)) : 0.0; };

    // total length: the scan below without its stores, taken at the last point, so that the last D is total / total = 1
    double head = 0.0;
    for (int j0 = 0; j0 < m; j0 += EM_CHUNK) {
        double v[EM_PER];
#pragma unroll
        for (int r = 0; r < EM_PER; ++r) v[r] = item(j0 + tid * EM_PER + r);
        const double tot = block_scan_f64(v, sc);
#pragma unroll
        for (int r = 0; r < EM_PER; ++r)
            if (j0 + tid * EM_PER + r == m - 1) total_sh = head + v[r];
        head += tot;
    }
    __syncthreads();
    const double total = total_sh;
    if (!(total > 0.0)) {                              // one point, or all points the same: everything matches index 0
        const int orig = flip ? m - 1 : 0;
        for (int i = tid; i < n; i += EM_THREADS) { mt[i] = orig; tt[i] = y[orig]; }
        return;
    }
    const double un = n > 1 ? (double)(n - 1) : 1.0;
    double carry = 0.0, prev_last = -1.0;              // prev_last < 0 <= every u: the first chunk has nothing before it
    int carry_run = 0;                                 // the first index whose D equals prev_last
    for (int j0 = 0; j0 < m; j0 += EM_CHUNK) {
        double v[EM_PER];
#pragma unroll
        for (int r = 0; r < EM_PER; ++r) v[r] = item(j0 + tid * EM_PER + r);
        const double tot = block_scan_f64(v, sc);
        __syncthreads();                               // Dl of the chunk before has been read
        const int cnt = min(EM_CHUNK, m - j0);
        if (tid == 0) Dl[0] = prev_last;
#pragma unroll
        for (int r = 0; r < EM_PER; ++r) {
            const int q = tid * EM_PER + r;
            if (q < cnt) Dl[1 + q] = (carry + v[r]) / total;
        }
        __syncthreads();
        const double lo_d = Dl[0], hi_d = Dl[cnt];
        for (int i = tid; i < n; i += EM_THREADS) {
            const double u = (double)i / un;
            if (!(u > lo_d && u <= hi_d)) continue;
            const int lb = lower_slot(Dl, 1, cnt, u);
            int g = j0 + lb - 1;
            if (!(j0 == 0 && lb == 1) && u - Dl[lb - 1] <= Dl[lb] - u) {      // the point below is as near: lowest index
                const int fa = lower_slot(Dl, 0, lb - 1, Dl[lb - 1]);           // ... of the run of equal D it ends
                g = fa == 0 ? carry_run : j0 + fa - 1;
            }
            const int orig = flip ? m - 1 - g : g;
            mt[i] = orig;
            tt[i] = y[orig];
        }
        const int fl = lower_slot(Dl, 0, cnt, hi_d);
        carry_run = fl == 0 ? carry_run : j0 + fl - 1;
        prev_last = hi_d;
        carry += tot;
    }
}

// Workgroup (icon b, block of EM_SHIFTS shifts): thread s walks S(s) = sum_k |x_k - t_{(k + s) mod n}| in ascending k, float64
// running sum of fp32 terms (one sqrtf each).  x and the window of t a tile needs go through LDS: x[k] is a broadcast,
// t[k + s] consecutive addresses across the lanes.  bmin / barg [b, block] take the block's minimum and its lowest shift.
__global__ __launch_bounds__(EM_SHIFTS) void emd_shift_kernel(const float* __restrict__ px, const int32_t* __restrict__ nx,
                                                              long long capx, const int32_t* __restrict__ ny, long long capy,
                                                              const float* __restrict__ t, int n_blocks,
                                                              double* __restrict__ bmin, int32_t* __restrict__ barg) {
    __shared__ float2 xs[EM_KTILE];
    __shared__ float2 ts[EM_KTILE + EM_SHIFTS];
    __shared__ double rs[EM_WAVES];
    __shared__ int ra[EM_WAVES];
    const long long blk = blockIdx.x;
    const long long b = blk / n_blocks;
    const int s0 = (int)(blk % n_blocks) * EM_SHIFTS;
    const int n = chamfer_count(nx, b, capx);
    if (s0 >= n || chamfer_count(ny, b, capy) == 0) return;          // (block-uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2* x = reinterpret_cast<const float2*>(px) + b * capx;
    const float2* tg = reinterpret_cast<const float2*>(t) + b * capx;
    const int s = s0 + tid;
    double sum = 0.0;
    for (int k0 = 0; k0 < n; k0 += EM_KTILE) {
        const int kc = min(EM_KTILE, n - k0);
        if (k0) __syncthreads();                       // the tiles of the step before have been read
        for (int i = tid; i < kc; i += EM_SHIFTS) xs[i] = x[k0 + i];
        const int base = (k0 + s0) % n;
        for (int i = tid; i < kc + EM_SHIFTS - 1; i += EM_SHIFTS) ts[i] = tg[(base + i) % n];
        __syncthreads();
        if (s < n) {
#pragma unroll 4
            for (int k = 0; k < kc; ++k) {
                const float2 p = xs[k], q = ts[k + tid];
                const float dx = p.x - q.x, dy = p.y - q.y;
                sum += (double)sqrtf(fmaf(dx, dx, dy * dy));
            }
        }
    }
    // (minimum, lowest shift) of the block
    double best = s < n ? sum : INFINITY;
    int arg = s < n ? s : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) { rs[wave] = best; ra[wave] = arg; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < EM_WAVES; ++w)
            if (rs[w] < best || (rs[w] == best && ra[w] < arg)) { best = rs[w]; arg = ra[w]; }
        bmin[blk] = best;
        barg[blk] = arg;
    }
}

// Workgroup b: the blocks in ascending order with strict < give (S(s*), s*); loss = (S(s*) + 9 |x_0 - t_{s*}| with the
// first-point weight) / n, matched[k] = match[(k + s*) mod n], -1 past the count.  n == 0: loss 0 (loss.py:25-26);
// n > 0 with an empty target: NaN.  shift is 0 and matched -1 in both.
__global__ __launch_bounds__(EM_THREADS) void emd_finish_kernel(const float* __restrict__ px, const int32_t* __restrict__ nx,
                                                                long long capx, const int32_t* __restrict__ ny, long long capy,
                                                                const float* __restrict__ t, const int32_t* __restrict__ match,
                                                                const double* __restrict__ bmin, const int32_t* __restrict__ barg,
                                                                int n_blocks, int weighted, float* __restrict__ out,
                                                                int32_t* __restrict__ shift, int32_t* __restrict__ matched) {
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = chamfer_count(nx, b, capx), m = chamfer_count(ny, b, capy);
    int32_t* mo = matched + b * capx;
    if (n == 0 || m == 0) {                            // (block-uniform)
        if (tid == 0) { out[b] = n == 0 ? 0.f : __builtin_nanf(""); shift[b] = 0; }
        for (long long k = tid; k < capx; k += EM_THREADS) mo[k] = -1;
        return;
    }
    double best = bmin[b * n_blocks];                  // every thread scans: the same address in every lane
    int s = barg[b * n_blocks];
    for (int q = 1; q < (n + EM_SHIFTS - 1) / EM_SHIFTS; ++q) {
        const double v = bmin[b * n_blocks + q];
        if (v < best) { best = v; s = barg[b * n_blocks + q]; }
    }
    s = min(max(s, 0), n - 1);
    if (tid == 0) {
        if (weighted) {
            const float2 p = reinterpret_cast<const float2*>(px)[b * capx], q = reinterpret_cast<const float2*>(t)[b * capx + s];
            const float dx = p.x - q.x, dy = p.y - q.y;
            best += 9.0 * (double)sqrtf(fmaf(dx, dx, dy * dy));
        }
        out[b] = (float)(best / (double)n);
        shift[b] = s;
    }
    const int32_t* mt = match + b * capx;
    for (long long k = tid; k < capx; k += EM_THREADS) {
        int j = (int)k + s;
        if (j >= n) j -= n;
        mo[k] = k < n ? mt[j] : -1;
    }
}

// dpx[b, k] = dout[b] w_k (x_k - t_{(k + s*) mod n}) / (|...| n), one thread per row; zero rows past the count and on an
// icon with an empty cloud (whatever dout[b] holds)
__global__ __launch_bounds__(256) void emd_bwd_kernel(const float* __restrict__ px, const int32_t* __restrict__ nx, long long capx,
                                                      const int32_t* __restrict__ ny, const float* __restrict__ t,
                                                      const int32_t* __restrict__ shift, const float* __restrict__ dout,
                                                      int weighted, long long rows, float* __restrict__ dpx) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const long long b = r / capx;
    const int k = (int)(r - b * capx);
    const int n = chamfer_count(nx, b, capx);
    float2 g = make_float2(0.f, 0.f);
    if (k < n && ny[b] > 0) {
        int j = k + min(max(shift[b], 0), n - 1);
        if (j >= n) j -= n;
        const float2 u = chamfer_unit_over(reinterpret_cast<const float2*>(px)[r], reinterpret_cast<const float2*>(t)[b * capx + j],
                                           (float)n);
        const float d = dout[b] * (weighted && k == 0 ? 10.f : 1.f);
        g = make_float2(d * u.x, d * u.y);
    }
    reinterpret_cast<float2*>(dpx)[r] = g;
}

// Workgroup b: L = sum_i |p_{i+1} - p_i| over the points in use, float64 in a fixed order
__global__ __launch_bounds__(EM_THREADS) void polyline_length_kernel(const float* __restrict__ p, const int32_t* __restrict__ n,
                                                                     long long cap, float* __restrict__ out) {
    __shared__ double red[EM_WAVES];
    const long long b = blockIdx.x;
    const int cnt = chamfer_count(n, b, cap);
    const float2* x = reinterpret_cast<const float2*>(p) + b * cap;
    double a = 0.0;
    for (int i = threadIdx.x; i < cnt - 1; i += EM_THREADS) a += segment_length(x[i], x[i + 1]);
    const double tot = block_sum_f64(a, red);
    if (threadIdx.x == 0) out[b] = (float)tot;
}

// dp[b, i] = dout[b] (u(p_i, p_{i-1}) - u(p_{i+1}, p_i)), u = 0 on a zero-length segment; zero rows past the count
__global__ __launch_bounds__(256) void polyline_length_bwd_kernel(const float* __restrict__ p, const int32_t* __restrict__ n,
                                                                  long long cap, const float* __restrict__ dout, long long rows,
                                                                  float* __restrict__ dp) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const long long b = r / cap;
    const int i = (int)(r - b * cap);
    const int cnt = chamfer_count(n, b, cap);
    const float2* x = reinterpret_cast<const float2*>(p);
    float2 g = make_float2(0.f, 0.f);
    if (i < cnt) {
        const float2 c = x[r];
        if (i > 0) { const float2 u = chamfer_unit_over(c, x[r - 1], 1.f); g.x += u.x; g.y += u.y; }
        if (i + 1 < cnt) { const float2 u = chamfer_unit_over(x[r + 1], c, 1.f); g.x -= u.x; g.y -= u.y; }
        const float d = dout[b];
        g = make_float2(d * g.x, d * g.y);
    }
    reinterpret_cast<float2*>(dp)[r] = g;
}

inline int64_t emd_blocks(int64_t capx) { return (capx + EM_SHIFTS - 1) / EM_SHIFTS; }
}  // namespace

extern "C" int dsvg_sample_points(int32_t itype, const void* commands, const void* args, int64_t B, int32_t G, int32_t L,
                                  int32_t n, float* points, int32_t* counts, void* stream) {
    DSVG_CHECK_ARG(commands && args && points && counts, "sample_points: null pointer");
    DSVG_CHECK_ARG(itype == DSVG_F32 || itype == DSVG_I64, "sample_points: itype %d is neither DSVG_F32 nor DSVG_I64", itype);
    if (sequence_args_ok("sample_points", "cloud", B, G, L, n)) return -1;
    const int64_t cap = (int64_t)G * ((int64_t)L * (n - 1) + 1);
    DSVG_CHECK_ARG(cap < (1ll << 31), "sample_points: %lld points per cloud do not fit int32", (long long)cap);
    hipStream_t st = (hipStream_t)stream;
    if (itype == DSVG_I64)
        hipLaunchKernelGGL(sample_points_kernel<long long>, dim3((unsigned)B), dim3(SP_THREADS), 0, st,
                           (const long long*)commands, (const long long*)args, G, L, n, (long long)cap, points, counts);
    else
        hipLaunchKernelGGL(sample_points_kernel<float>, dim3((unsigned)B), dim3(SP_THREADS), 0, st, (const float*)commands,
                           (const float*)args, G, L, n, (long long)cap, points, counts);
    DSVG_LAUNCH_CHECK("sample_points");
    return 0;
}

extern "C" int64_t dsvg_chamfer_workspace_bytes(int64_t B, int64_t capx, int64_t capy) {
    if (B <= 0 || capx <= 0 || capy <= 0) return 0;
    return B * 2 * chamfer_slices(capx, capy) * (int64_t)sizeof(double);
}

namespace {
// the arguments dsvg_chamfer, _nn and _bwd share, refused under the name of the caller; the workspace only `with_ws`.
// -> *n_slices: slices per cloud and direction
int chamfer_args_ok(const char* name, bool pointers, int64_t B, int64_t capx, int64_t capy, int64_t* n_slices, bool with_ws,
                    const void* workspace, int64_t workspace_bytes) {
    DSVG_CHECK_ARG(pointers, "%s: null pointer", name);
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && capx > 0 && capy > 0 && capx < (1ll << 31) && capy < (1ll << 31),
                   "%s: bad shape (B=%lld capx=%lld capy=%lld; clouds hold 1 .. 2^31 - 1 points)", name, (long long)B,
                   (long long)capx, (long long)capy);
    *n_slices = chamfer_slices(capx, capy);
    const int64_t blocks = B * 2 * *n_slices;
    DSVG_CHECK_ARG(blocks < (1ll << 31), "%s: %lld workgroups (B=%lld, %lld slices of %d points, 2 directions)", name,
                   (long long)blocks, (long long)B, (long long)*n_slices, CH_SLICE);
    if (with_ws)
        DSVG_CHECK_ARG(workspace_bytes >= dsvg_chamfer_workspace_bytes(B, capx, capy) && ((uintptr_t)workspace & 7) == 0,
                       "%s: workspace of %lld bytes, need %lld (8-byte aligned)", name, (long long)workspace_bytes,
                       (long long)dsvg_chamfer_workspace_bytes(B, capx, capy));
    return 0;
}

int chamfer_launch(const char* name, const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny,
                   int64_t capy, int64_t B, float* out, int32_t* idx_x, int32_t* idx_y, bool nn, void* workspace,
                   int64_t workspace_bytes, void* stream) {
    int64_t n_slices;
    if (chamfer_args_ok(name, px && nx && py && ny && out && workspace && ((idx_x && idx_y) || !nn), B, capx, capy, &n_slices,
                        true, workspace, workspace_bytes))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * 2 * n_slices)), block(CH_THREADS);
    if (nn)
        hipLaunchKernelGGL(chamfer_slice_kernel<true>, grid, block, 0, st, px, nx, (long long)capx, py, ny, (long long)capy,
                           (int)n_slices, (double*)workspace, idx_x, idx_y);
    else
        hipLaunchKernelGGL(chamfer_slice_kernel<false>, grid, block, 0, st, px, nx, (long long)capx, py, ny, (long long)capy,
                           (int)n_slices, (double*)workspace, idx_x, idx_y);
    DSVG_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(chamfer_finish_kernel, dim3((unsigned)dsvg_cdiv(B, 256)), dim3(256), 0, st, (const double*)workspace,
                       nx, (long long)capx, ny, (long long)capy, (int)n_slices, (long long)B, out);
    DSVG_LAUNCH_CHECK("chamfer_finish");
    return 0;
}
}  // namespace

extern "C" int dsvg_chamfer(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny,
                            int64_t capy, int64_t B, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    return chamfer_launch("chamfer", px, nx, capx, py, ny, capy, B, out, nullptr, nullptr, false, workspace, workspace_bytes,
                          stream);
}

extern "C" int dsvg_chamfer_nn(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny,
                               int64_t capy, int64_t B, float* out, int32_t* idx_x, int32_t* idx_y, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    return chamfer_launch("chamfer_nn", px, nx, capx, py, ny, capy, B, out, idx_x, idx_y, true, workspace, workspace_bytes,
                          stream);
}

extern "C" int dsvg_chamfer_bwd(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny,
                                int64_t capy, int64_t B, const int32_t* idx_x, const int32_t* idx_y, const float* dout,
                                float* dpx, float* dpy, void* stream) {
    int64_t n_slices;
    if (chamfer_args_ok("chamfer_bwd", px && nx && py && ny && idx_x && idx_y && dout && dpx && dpy, B, capx, capy, &n_slices,
                        false, nullptr, 0))
        return -1;
    hipLaunchKernelGGL(chamfer_bwd_kernel, dim3((unsigned)(B * 2 * n_slices)), dim3(CH_THREADS), 0, (hipStream_t)stream, px, nx,
                       (long long)capx, py, ny, (long long)capy, idx_x, idx_y, dout, (int)n_slices, dpx, dpy);
    DSVG_LAUNCH_CHECK("chamfer_bwd");
    return 0;
}

extern "C" int dsvg_sample_points_bwd(const float* commands, int64_t B, int32_t G, int32_t L, int32_t n, const float* dpoints,
                                      float* dargs, void* stream) {
    DSVG_CHECK_ARG(commands && dpoints && dargs, "sample_points_bwd: null pointer");
    if (sequence_args_ok("sample_points_bwd", "cloud", B, G, L, n)) return -1;
    const int64_t cap = (int64_t)G * ((int64_t)L * (n - 1) + 1);
    DSVG_CHECK_ARG(cap < (1ll << 31), "sample_points_bwd: %lld points per cloud do not fit int32", (long long)cap);
    hipLaunchKernelGGL(sample_points_bwd_kernel, dim3((unsigned)B), dim3(SP_THREADS), 0, (hipStream_t)stream, commands, G, L,
                       n, (long long)cap, dpoints, dargs);
    DSVG_LAUNCH_CHECK("sample_points_bwd");
    return 0;
}

extern "C" int64_t dsvg_emd_workspace_bytes(int64_t B, int64_t capx) {
    if (B <= 0 || capx <= 0) return 0;
    return B * emd_blocks(capx) * (int64_t)(sizeof(double) + sizeof(int32_t)) + B * capx * (int64_t)sizeof(int32_t);
}

extern "C" int dsvg_emd(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny, int64_t capy,
                        int64_t B, int32_t first_point_weight, float* out, int32_t* shift, int32_t* matched, float* t,
                        void* workspace, int64_t workspace_bytes, void* stream) {
    DSVG_CHECK_ARG(px && nx && py && ny && out && shift && matched && t && workspace, "emd: null pointer");
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && capx > 0 && capy > 0 && capy < (1ll << 31),
                   "emd: bad shape (B=%lld capx=%lld capy=%lld; target clouds hold 1 .. 2^31 - 1 points)", (long long)B,
                   (long long)capx, (long long)capy);
    DSVG_CHECK_ARG(capx <= EM_MAX_N, "emd: capx = %lld, a pred cloud holds at most %d points", (long long)capx, EM_MAX_N);
    const int64_t n_blocks = emd_blocks(capx), blocks = B * n_blocks;
    DSVG_CHECK_ARG(blocks < (1ll << 31), "emd: %lld workgroups (B=%lld, %lld blocks of %d shifts)", (long long)blocks,
                   (long long)B, (long long)n_blocks, EM_SHIFTS);
    DSVG_CHECK_ARG(workspace_bytes >= dsvg_emd_workspace_bytes(B, capx) && ((uintptr_t)workspace & 7) == 0,
                   "emd: workspace of %lld bytes, need %lld (8-byte aligned)", (long long)workspace_bytes,
                   (long long)dsvg_emd_workspace_bytes(B, capx));
    double* bmin = (double*)workspace;                 // [B, n_blocks], then barg int32 [B, n_blocks], match int32 [B, capx]
    int32_t* barg = (int32_t*)(bmin + blocks);
    int32_t* match = barg + blocks;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(emd_match_kernel, dim3((unsigned)B), dim3(EM_THREADS), 0, st, nx, (long long)capx, py, ny,
                       (long long)capy, match, t);
    DSVG_LAUNCH_CHECK("emd_match");
    hipLaunchKernelGGL(emd_shift_kernel, dim3((unsigned)blocks), dim3(EM_SHIFTS), 0, st, px, nx, (long long)capx, ny,
                       (long long)capy, (const float*)t, (int)n_blocks, bmin, barg);
    DSVG_LAUNCH_CHECK("emd_shift");
    hipLaunchKernelGGL(emd_finish_kernel, dim3((unsigned)B), dim3(EM_THREADS), 0, st, px, nx, (long long)capx, ny,
                       (long long)capy, (const float*)t, (const int32_t*)match, (const double*)bmin, (const int32_t*)barg,
                       (int)n_blocks, first_point_weight ? 1 : 0, out, shift, matched);
    DSVG_LAUNCH_CHECK("emd_finish");
    return 0;
}

extern "C" int dsvg_emd_bwd(const float* px, const int32_t* nx, int64_t capx, const int32_t* ny, const float* t,
                            const int32_t* shift, const float* dout, int32_t first_point_weight, int64_t B, float* dpx,
                            void* stream) {
    DSVG_CHECK_ARG(px && nx && ny && t && shift && dout && dpx, "emd_bwd: null pointer");
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && capx > 0, "emd_bwd: bad shape (B=%lld capx=%lld)", (long long)B, (long long)capx);
    DSVG_CHECK_ARG(capx <= EM_MAX_N, "emd_bwd: capx = %lld, a pred cloud holds at most %d points", (long long)capx, EM_MAX_N);
    const int64_t rows = B * capx;
    DSVG_CHECK_ARG((rows + 255) / 256 < (1ll << 31), "emd_bwd: %lld rows (B=%lld capx=%lld)", (long long)rows, (long long)B,
                   (long long)capx);
    hipLaunchKernelGGL(emd_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, px, nx,
                       (long long)capx, ny, t, shift, dout, first_point_weight ? 1 : 0, (long long)rows, dpx);
    DSVG_LAUNCH_CHECK("emd_bwd");
    return 0;
}

extern "C" int dsvg_polyline_length(const float* p, const int32_t* n, int64_t cap, int64_t B, float* out, void* stream) {
    DSVG_CHECK_ARG(p && n && out, "polyline_length: null pointer");
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && cap > 0 && cap < (1ll << 31),
                   "polyline_length: bad shape (B=%lld cap=%lld; clouds hold 1 .. 2^31 - 1 points)", (long long)B, (long long)cap);
    hipLaunchKernelGGL(polyline_length_kernel, dim3((unsigned)B), dim3(EM_THREADS), 0, (hipStream_t)stream, p, n, (long long)cap,
                       out);
    DSVG_LAUNCH_CHECK("polyline_length");
    return 0;
}

extern "C" int dsvg_polyline_length_bwd(const float* p, const int32_t* n, int64_t cap, int64_t B, const float* dout, float* dp,
                                        void* stream) {
    DSVG_CHECK_ARG(p && n && dout && dp, "polyline_length_bwd: null pointer");
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && cap > 0 && cap < (1ll << 31),
                   "polyline_length_bwd: bad shape (B=%lld cap=%lld; clouds hold 1 .. 2^31 - 1 points)", (long long)B,
                   (long long)cap);
    const int64_t rows = B * cap;
    DSVG_CHECK_ARG((rows + 255) / 256 < (1ll << 31), "polyline_length_bwd: %lld rows (B=%lld cap=%lld)", (long long)rows,
                   (long long)B, (long long)cap);
    hipLaunchKernelGGL(polyline_length_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, n,
                       (long long)cap, dout, (long long)rows, dp);
    DSVG_LAUNCH_CHECK("polyline_length_bwd");
    return 0;
}
