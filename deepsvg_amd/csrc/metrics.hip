// Reconstruction error of decoded icons, for evaluation only (no gradients): points sampled on the curves of a command
// sequence (SVGTensor.sample_points, deepsvg/difflib/tensor.py:191-230) and the Chamfer distance between two such clouds
// (chamfer_loss, deepsvg/difflib/loss.py:5-7).
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
#include "dsvg_common.h"
#include "../../include/dsvg.h"

namespace {
constexpr int SP_THREADS = 256;
constexpr int SP_MAX_TOK = 2048;          // G * L tokens of one cloud: 8 chunks of 256
constexpr int SP_N_ARGS = 11;
constexpr int SP_CMD_L = 1, SP_CMD_C = 2;

// pre[t] = number of set flags among items < t, for t in 0..n (pre[n] = the total), n <= SP_MAX_TOK.  flag(t) is called
// by every thread for t < the chunk-rounded n and must return false past n.  wtot: one slot per wave of every chunk.
template <typename F>
__device__ __forceinline__ void block_flag_scan(int n, int* __restrict__ pre, int* __restrict__ wtot, F flag) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (n + SP_THREADS - 1) / SP_THREADS;
    int below[SP_MAX_TOK / SP_THREADS];     // flags below this lane inside its wave, per chunk (unrolled: registers)
#pragma unroll
    for (int c = 0; c < SP_MAX_TOK / SP_THREADS; ++c) {
        below[c] = 0;
        if (c < n_chunks) {
            const unsigned long long b = __ballot(flag(c * SP_THREADS + tid));
            below[c] = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) wtot[c * (SP_THREADS / 64) + wave] = __popcll(b);
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SP_MAX_TOK / SP_THREADS; ++c) {
        if (c < n_chunks) {
            const int w = c * (SP_THREADS / 64) + wave;
            int base = 0;
            for (int q = 0; q < w; ++q) base += wtot[q];      // <= 31 broadcast reads
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
    const T* arg = args + b * T_ * SP_N_ARGS;

    // ---- pass 1: where every drawing command's points go -----------------------------------------------------------
    block_flag_scan(T_, pre, wtot, [&](int t) {
        if (t >= T_) return false;
        const int c = (int)cmd[t];
        return c == SP_CMD_L || c == SP_CMD_C;
    });
    block_flag_scan(G, full, wtot, [&](int g) { return g < G && pre[(g + 1) * L] > pre[g * L]; });
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
        const T* a = arg + (long long)t * SP_N_ARGS;
        // start point: the end position of the row before, whatever that row holds; (0, 0) on row 0 (tensor.py:75-82)
        const float p0x = i ? (float)a[9 - SP_N_ARGS] : 0.f, p0y = i ? (float)a[10 - SP_N_ARGS] : 0.f;
        const float p3x = (float)a[9], p3y = (float)a[10];
        const float z = (float)k / (float)(n - 1);
        float x, y;
        if ((int)cmd[t] == SP_CMD_L) {
            x = fmaf(z, p3x - p0x, p0x);
            y = fmaf(z, p3y - p0y, p0y);
        } else {
            const float p1x = (float)a[5], p1y = (float)a[6], p2x = (float)a[7], p2y = (float)a[8];
            // power basis of the cubic Bezier (exact for integer arguments), Horner in z
            const float c1x = 3.f * (p1x - p0x), c2x = 3.f * (p0x - 2.f * p1x + p2x), c3x = (p3x - p0x) + 3.f * (p1x - p2x);
            const float c1y = 3.f * (p1y - p0y), c2y = 3.f * (p0y - 2.f * p1y + p2y), c3y = (p3y - p0y) + 3.f * (p1y - p2y);
            x = fmaf(fmaf(fmaf(c3x, z, c2x), z, c1x), z, p0x);
            y = fmaf(fmaf(fmaf(c3y, z, c2y), z, c1y), z, p0y);
        }
        const long long o = (long long)pre[t] * (n - 1) + full[g] + k;
        reinterpret_cast<float2*>(out)[o] = make_float2(x, y);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int CH_THREADS = 256;
constexpr int CH_WAVES = CH_THREADS / 64;
constexpr int CH_R = 4;                   // chunks of 64 points a wave keeps in registers (one point per lane and chunk)
constexpr int CH_SLICE = CH_WAVES * CH_R * 64;      // points of one cloud per workgroup: 1,024
constexpr int CH_TILE = 1024;             // points of the other cloud per LDS tile (8 KiB)

// running minimum of the squared distance from R register points to the first cnt4 (a multiple of 4) points of the tile
template <int R>
__device__ __forceinline__ void chamfer_sweep(const float4* __restrict__ tile, int cnt4, const float2 (&x)[CH_R],
                                              float (&m)[CH_R]) {
#pragma unroll 2
    for (int jj = 0; jj < cnt4 / 2; jj += 2) {
        const float4 q0 = tile[jj], q1 = tile[jj + 1];        // 4 points, the same address in every lane
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float dx = x[r].x - q0.x, dy = x[r].y - q0.y;
            m[r] = fminf(m[r], fmaf(dx, dx, dy * dy));
            dx = x[r].x - q0.z; dy = x[r].y - q0.w;
            m[r] = fminf(m[r], fmaf(dx, dx, dy * dy));
            dx = x[r].x - q1.x; dy = x[r].y - q1.y;
            m[r] = fminf(m[r], fmaf(dx, dx, dy * dy));
            dx = x[r].x - q1.z; dy = x[r].y - q1.w;
            m[r] = fminf(m[r], fmaf(dx, dx, dy * dy));
        }
    }
}

__device__ __forceinline__ int chamfer_count(const int32_t* n, long long b, long long cap) {
    return (int)min((long long)max(n[b], 0), cap);
}

// Workgroup (icon b, direction d, slice s): sum_i min_j |x_i - y_j| over the points i of slice s of cloud x (d = 0: x = px,
// y = py; d = 1: the roles swapped - the same code on swapped pointers, so chamfer(x, y) and chamfer(y, x) add the same
// numbers).  The 16 chunks of 64 points of a slice are dealt round-robin to the 4 waves, up to CH_R chunks per wave in
// registers; y streams through the LDS tile.  part[(b * 2 + d) * n_slices + s] takes the sum; slices past the cloud's end
// and icons with an empty cloud write nothing (the finish kernel does not read them).
__global__ __launch_bounds__(CH_THREADS) void chamfer_slice_kernel(const float* __restrict__ px, const int32_t* __restrict__ nx,
                                                                   long long capx, const float* __restrict__ py,
                                                                   const int32_t* __restrict__ ny, long long capy,
                                                                   int n_slices, double* __restrict__ part) {
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (n_x + 63) >> 6;

    float2 xr[CH_R];
    float m[CH_R];
    int nr = 0;                                        // chunks of this wave (wave-uniform)
#pragma unroll
    for (int r = 0; r < CH_R; ++r) {
        const int c = s * (CH_SLICE / 64) + r * CH_WAVES + wave;
        if (c < n_chunks) nr = r + 1;
        xr[r] = x[min(c * 64 + lane, n_x - 1)];
        m[r] = INFINITY;
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
            case 4: chamfer_sweep<4>(t4, cnt4, xr, m); break;
            case 3: chamfer_sweep<3>(t4, cnt4, xr, m); break;
            case 2: chamfer_sweep<2>(t4, cnt4, xr, m); break;
            case 1: chamfer_sweep<1>(t4, cnt4, xr, m); break;
            default: break;
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < CH_R; ++r) {
        const int c = s * (CH_SLICE / 64) + r * CH_WAVES + wave;
        if (c < n_chunks && c * 64 + lane < n_x) sum += sqrtf(m[r]);
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

inline int64_t chamfer_slices(int64_t capx, int64_t capy) {
    return ((capx > capy ? capx : capy) + CH_SLICE - 1) / CH_SLICE;
}
}  // namespace

extern "C" int dsvg_sample_points(int32_t itype, const void* commands, const void* args, int64_t B, int32_t G, int32_t L,
                                  int32_t n, float* points, int32_t* counts, void* stream) {
    DSVG_CHECK_ARG(commands && args && points && counts, "sample_points: null pointer");
    DSVG_CHECK_ARG(itype == DSVG_F32 || itype == DSVG_I64, "sample_points: itype %d is neither DSVG_F32 nor DSVG_I64", itype);
    DSVG_CHECK_ARG(n >= 2 && n <= 64, "sample_points: n = %d points per command, need 2..64", n);
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && G >= 1 && L >= 1 && (int64_t)G * L <= SP_MAX_TOK,
                   "sample_points: bad shape (B=%lld G=%d L=%d; G * L <= %d tokens per cloud)", (long long)B, G, L, SP_MAX_TOK);
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

extern "C" int dsvg_chamfer(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny,
                            int64_t capy, int64_t B, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    DSVG_CHECK_ARG(px && nx && py && ny && out && workspace, "chamfer: null pointer");
    DSVG_CHECK_ARG(B > 0 && B < (1ll << 31) && capx > 0 && capy > 0 && capx < (1ll << 31) && capy < (1ll << 31),
                   "chamfer: bad shape (B=%lld capx=%lld capy=%lld; clouds hold 1 .. 2^31 - 1 points)", (long long)B,
                   (long long)capx, (long long)capy);
    const int64_t n_slices = chamfer_slices(capx, capy), blocks = B * 2 * n_slices;
    DSVG_CHECK_ARG(blocks < (1ll << 31), "chamfer: %lld workgroups (B=%lld, %lld slices of %d points, 2 directions)",
                   (long long)blocks, (long long)B, (long long)n_slices, CH_SLICE);
    DSVG_CHECK_ARG(workspace_bytes >= dsvg_chamfer_workspace_bytes(B, capx, capy) && ((uintptr_t)workspace & 7) == 0,
                   "chamfer: workspace of %lld bytes, need %lld (8-byte aligned)", (long long)workspace_bytes,
                   (long long)dsvg_chamfer_workspace_bytes(B, capx, capy));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chamfer_slice_kernel, dim3((unsigned)blocks), dim3(CH_THREADS), 0, st, px, nx, (long long)capx, py, ny,
                       (long long)capy, (int)n_slices, (double*)workspace);
    DSVG_LAUNCH_CHECK("chamfer");
    hipLaunchKernelGGL(chamfer_finish_kernel, dim3((unsigned)dsvg_cdiv(B, 256)), dim3(256), 0, st, (const double*)workspace,
                       nx, (long long)capx, ny, (long long)capy, (int)n_slices, (long long)B, out);
    DSVG_LAUNCH_CHECK("chamfer_finish");
    return 0;
}
