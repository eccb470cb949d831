// Exclusive prefix count of a flag over the tokens of one cloud / image, by one workgroup of SP_THREADS threads: a ballot per
// wave and chunk, then a prefix sum over the wave totals.  Shared by csrc/metrics.hip (sample_points and its backward) and
// csrc/raster.hip (the chord offsets of an image); both give every drawing command its output offset with it.
#pragma once
#include "dsvg_common.h"

namespace {
constexpr int SP_THREADS = 256;
constexpr int SP_MAX_TOK = 2048;          // G * L tokens of one cloud: 8 chunks of 256

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
}  // namespace
