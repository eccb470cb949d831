// Images of a decoded batch: the curves sample_points draws (SVGTensor.sample_points, deepsvg/difflib/tensor.py:191-230),
// rasterised into anti-aliased coverage images, as outlines or filled - what the reference gets one icon at a time from
// SVG.draw -> cairosvg on the host (deepsvg/svglib/svg.py:172-204; fill without stroke: svglib/svg_primitive.py:34-38).
// The definition of an image is in include/dsvg.h; tests/raster_ref.py restates it in float64.
//   dsvg_raster_segments  one workgroup per image (the G sequences of an icon, in group order): ballots + prefix sums give
//                         every drawing command, and in fill mode every sub-path's closing chord, its offset
//                         (block_flag_scan of flag_scan.h, as dsvg_sample_points); the (command, chord) pairs are then
//                         evaluated by consecutive lanes.  Vertex 0 of a command is its start point and vertex n - 1 its end
//                         position bit for bit, so consecutive chords share their vertices exactly.
//   dsvg_raster_sweep     one workgroup per (image, tile of 32 x 32 pixels): a wave owns a 16 x 16 quadrant, a lane four
//                         pixels of one column, 4 rows apart, in registers; the image's chords stream through LDS in tiles
//                         (every lane reads the same address: a broadcast); running minimum of the SQUARED distance, one sqrt
//                         per pixel after the sweep; in fill mode a running winding count per pixel, folded into an
//                         `inside` bit at every sequence start.  No atomics, no scratch: bit-reproducible.
//   dsvg_raster_sweep_nn  the same kernel with one more template flag: the running minimum also keeps the record index of the
//                         chord that set it (a strict <: of equal d^2 the lowest index), stored where 0 < ink < 1, -1 elsewhere.
// Layered RGB images (per-group outline / fill / erase, colours and opacities painted in group order):
//   dsvg_raster_segments_layers  dsvg_raster_segments' kernel under a template flag: closing chords by the group's mode,
//                                and the record offset of every group's first chord.
//   dsvg_raster_sweep_layers     the sweep's tiling with three canvas channels per pixel; at a layer's last record the
//                                workgroup folds: one sqrt, the layer's coverage, the blend, a reset.  Bit-reproducible.
// The gradient of an image (a pixel's ink depends on the chords only through the distance d to its nearest chord):
//   dsvg_raster_sweep_bwd     a group of 16 or 64 lanes per chord walks the chord's bounding box, dilated by the reach the sweep
//                             culls with and clipped to the image, in a fixed order; lanes accumulate the pixels whose saved
//                             index is this chord (t and q recomputed with the sweep's expressions), a fixed-shape __shfl_xor
//                             reduction, one lane stores d / d(ax, ay, bx, by).  A gather: no atomics, bit-reproducible.
//   dsvg_raster_segments_bwd  the transpose of dsvg_raster_segments (linear in args): one workgroup per image, the forward's two
//                             scans, one thread per token gathers its own command's chords, the next row's (whose start point
//                             is this row's end position) and the closing chords that start or end at it, in float64.
// The gradient of a layered image (a layer's coverage depends on the chords through the distance to the nearest chord of ITS group):
//   dsvg_raster_sweep_layers_nn      dsvg_raster_sweep_layers' kernel with one more template flag: every fold also stores the
//                                    layer's clamped coverage and the record index of its nearest chord (-1 where saturated).
//   dsvg_raster_blend_bwd            one workgroup per image, a lane per pixel: a forward walk over the layers rebuilds the canvas
//                                    and leaves sum_c dout_c (p_c - C_{g-1,c}) in the dcov slot, a reverse walk carries T = prod (1 -
//                                    alpha) and finishes the slot; d colour and d opacity through a shuffle tree per wave into LDS
//                                    accumulators of the wave's own, summed in wave order.  No atomics, bit-reproducible.
//   dsvg_raster_sweep_layers_bwd     dsvg_raster_sweep_bwd's walk with the layer of a record found from the layer table.
//   dsvg_raster_segments_layers_bwd  dsvg_raster_segments_bwd's kernel under a template flag: closing chords by the group's mode.
#include <type_traits>

#include "dsvg_common.h"
#include "svg_seq.h"
#include "../../include/dsvg.h"

namespace {
// (the record and tile constants RS_* are in svg_seq.h, shared with csrc/paths_fill.hip)
constexpr int RS_MAX_SIZE = 4096;

// chords an image can hold: n - 1 per token, and in fill mode one closing chord per sub-path (two sub-paths of a sequence
// have a non-drawing row between them: at most (L + 1) / 2 of them)
inline int64_t raster_cap(int64_t G, int64_t L, int64_t n, int fill) {
    return G * (L * (n - 1) + (fill ? (L + 1) / 2 : 0));
}

// flags word of a record: bit 0 = the first chord of a sequence; bits 1..31 = on a closing chord, how many records back
// its sub-path's first chord lies (>= n - 1 >= 1), 0 on every other chord
// LAYERS (dsvg_raster_segments_layers): `fill` is per group, read from modes[b, g] (1 = FILL and 2 = ERASE close their
// sub-paths, every other value is an outline), and layer_first[b, 0..G] receives the record offset of every group's first
// chord, the count last.  Without LAYERS `modes` and `layer_first` are not touched.
template <typename T, bool LAYERS>
__global__ __launch_bounds__(SP_THREADS) void raster_segments_kernel(const T* __restrict__ commands, const T* __restrict__ args,
                                                                     int G, int L, int n, int fill, long long cap,
                                                                     float* __restrict__ segs, int32_t* __restrict__ seg_counts,
                                                                     const int32_t* __restrict__ modes,
                                                                     int32_t* __restrict__ layer_first) {
    __shared__ int pre[SP_MAX_TOK + 1];       // drawing commands of the image before token t
    __shared__ int cl[SP_MAX_TOK + 1];        // sub-paths that end before token t (fill mode; all zero otherwise)
    __shared__ int src[SP_MAX_TOK];           // token of the j-th drawing command
    __shared__ int first[SP_MAX_TOK];         // first token of the q-th sub-path
    __shared__ int wtot[SP_MAX_TOK / 64];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int T_ = G * L;
    const T* cmd = commands + b * T_;
    const T* arg = args + b * T_ * N_ARGS;

    // whether the sub-paths of token t's group are closed (t < T_)
    auto closes = [&](int t) -> int {
        if constexpr (LAYERS) {
            const int m = modes[b * G + t / L];
            return m == DSVG_LAYER_FILL || m == DSVG_LAYER_ERASE;
        } else {
            return fill;
        }
    };

    // ---- pass 1: where every command's chords and every sub-path's closing chord go --------------------------------------
    block_flag_scan<SP_MAX_TOK>(T_, pre, wtot, [&](int t) { return is_drawing(cmd, t, T_); });
    if constexpr (LAYERS)
        block_flag_scan<SP_MAX_TOK>(T_, cl, wtot, [&](int t) { return subpath_ends(pre, t, T_, L, t < T_ ? closes(t) : 0); });
    else
        block_flag_scan<SP_MAX_TOK>(T_, cl, wtot, [&](int t) { return subpath_ends(pre, t, T_, L, fill); });
    for (int t = tid; t < T_; t += SP_THREADS)
        if (pre[t + 1] > pre[t]) {
            src[pre[t]] = t;
            if (closes(t) && (t % L == 0 || pre[t] == pre[t - 1])) first[cl[t]] = t;      // cl[t] sub-paths lie before this one
        }
    __syncthreads();
    const int K = pre[T_];
    if (tid == 0) seg_counts[b] = K * (n - 1) + cl[T_];
    if constexpr (LAYERS)
        for (int g = tid; g <= G; g += SP_THREADS) layer_first[b * (G + 1) + g] = pre[g * L] * (n - 1) + cl[g * L];

    float* out = segs + b * cap * RS_REC;
    auto put = [&](long long o, float ax, float ay, float bx, float by, int flags) {
        float* r = out + o * RS_REC;
        r[0] = ax; r[1] = ay; r[2] = bx - ax; r[3] = by - ay; r[4] = __int_as_float(flags);
    };
    // start point of token t, in the one-branch form (start_point's two selects load the coordinates one by one here)
    auto start_of = [&](int t) {
        const T* a = arg + (long long)t * N_ARGS;
        return t % L ? make_float2((float)a[ARG_END - N_ARGS], (float)a[ARG_END + 1 - N_ARGS]) : make_float2(0.f, 0.f);
    };

    // ---- pass 2: work item (j, k) = chord k (vertex k -> vertex k + 1) of the j-th drawing command ----------------------------
    const float nm1 = (float)(n - 1);
    for (int w = tid; w < K * (n - 1); w += SP_THREADS) {
        const int j = w / (n - 1), k = w - j * (n - 1);
        const int t = src[j];
        const int g = t / L;
        const T* a = arg + (long long)t * N_ARGS;
        const float2 p0 = start_of(t);
        const float p3x = (float)a[ARG_END], p3y = (float)a[ARG_END + 1];
        const bool cubic = (int)cmd[t] == CMD_C;
        CubicPower curve;
        if (cubic) curve = CubicPower(p0, a, p3x, p3y);
        // vertex q: the start point and the end position themselves at q = 0 and q = n - 1; between them Horner in z =
        // q / (n - 1) for `c`, and ((n - 1 - q) p0 + q p3) / (n - 1) for `l` (an exact numerator for integer arguments)
        float2 v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int q = k + e;
            const float fq = (float)q;
            if (q == 0) v[e] = p0;
            else if (q == n - 1) v[e] = make_float2(p3x, p3y);
            else if (cubic) v[e] = curve.eval(p0, fq / nm1);
            else {
                const float fr = (float)(n - 1 - q);
                v[e] = make_float2(fmaf(fq, p3x, fr * p0.x) / nm1, fmaf(fq, p3y, fr * p0.y) / nm1);
            }
        }
        put((long long)j * (n - 1) + cl[t] + k, v[0].x, v[0].y, v[1].x, v[1].y, k == 0 && j == pre[g * L] ? 1 : 0);
    }
    // ---- pass 3 (fill): the closing chord of every sub-path, from its last vertex to its first, behind its last chord ----------
    if (LAYERS || fill)
        for (int t = tid; t < T_; t += SP_THREADS)
            if (cl[t + 1] > cl[t]) {
                const int tf = first[cl[t]];
                const T* a = arg + (long long)t * N_ARGS;
                const float2 p = start_of(tf);
                put((long long)(pre[t] + 1) * (n - 1) + cl[t], (float)a[ARG_END], (float)a[ARG_END + 1], p.x, p.y,
                    ((pre[t] + 1 - pre[tf]) * (n - 1)) << 1);
            }
}

// Workgroup (image b, tile row ty, tile column tx).  LDS record of a chord: (ax, ay, dx, dy), (1 / |d|^2 or 0, by, flags, -)
// with by the y of the chord's end vertex AS THE NEXT CHORD HOLDS IT (the record after it; on a closing chord its sub-path's
// first record): ay + dy is that value only up to rounding, and the half-open crossing rule is watertight only when a
// shared vertex is one number.  With CULL a wave skips the distance work of a chord whose bounding box is farther from the
// wave's 16 x 16 pixel centres than the distance at which ink saturates (plus a margin far above the rounding of either
// side); such a chord cannot change a pixel.  The crossing test is never skipped.
// NN: the minimum keeps the index of the record that set it (`idx` is not touched without NN); a chord culled for a wave is
// farther from every pixel of the wave than the distance at which ink saturates, so the index of an unsaturated pixel is the
// same with and without CULL.
template <bool FILL, bool CULL, bool NN>
__global__ __launch_bounds__(RS_THREADS) void raster_sweep_kernel(const float* __restrict__ segs, const int32_t* __restrict__ seg_counts,
                                                                  long long cap, int size, int tiles, float s, float half_w,
                                                                  float* __restrict__ out, int32_t* __restrict__ idx) {
    __shared__ __attribute__((aligned(16))) float4 rec[RS_CHORDS * 2];
    __shared__ __attribute__((aligned(16))) float4 box[CULL ? RS_CHORDS : 1];
    const long long blk = blockIdx.x;
    const int tx = (int)(blk % tiles), ty = (int)((blk / tiles) % tiles);
    const long long b = blk / ((long long)tiles * tiles);
    const int cnt = chamfer_count(seg_counts, b, cap);
    const float* sg = segs + b * cap * RS_REC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col0 = tx * RS_TILE + (wave & 1) * RS_QUAD, row0 = ty * RS_TILE + (wave >> 1) * RS_QUAD;
    const int col = col0 + (lane & 15), row = row0 + (lane >> 4);
    const float cx = ((float)col + 0.5f) * s;
    float cy[RS_PIX], m[RS_PIX];
    int wind[RS_PIX], inside[RS_PIX], mi[RS_PIX];
#pragma unroll
    for (int r = 0; r < RS_PIX; ++r) {
        cy[r] = ((float)(row + 4 * r) + 0.5f) * s;
        m[r] = INFINITY;
        mi[r] = -1;
        wind[r] = 0;
        inside[r] = 0;
    }
    // the wave's pixel centres span [qx0, qx1] x [qy0, qy1]
    const float qx0 = ((float)col0 + 0.5f) * s, qx1 = ((float)(col0 + RS_QUAD - 1) + 0.5f) * s;
    const float qy0 = ((float)row0 + 0.5f) * s, qy1 = ((float)(row0 + RS_QUAD - 1) + 0.5f) * s;
    const float reach = (FILL ? 0.5f * s : half_w + 0.5f * s) * 1.001f + 0.01f;
    const float reach2 = reach * reach;

    for (int j0 = 0; j0 < cnt; j0 += RS_CHORDS) {
        if (j0) __syncthreads();                       // the tile of the step before has been read
#pragma unroll
        for (int h = 0; h < RS_CHORDS / RS_THREADS; ++h) {
            const int jl = h * RS_THREADS + tid, j = j0 + jl;
            if (j < cnt) {
                const float* r = sg + (long long)j * RS_REC;
                const float ax = r[0], ay = r[1], dx = r[2], dy = r[3];
                const int fl = __float_as_int(r[4]);
                const float len2 = fmaf(dx, dx, dy * dy);
                float by = ay + dy;
                if (FILL) by = chord_end_y(sg, j, cnt, ay, dy, fl);
                rec[2 * jl] = make_float4(ax, ay, dx, dy);
                rec[2 * jl + 1] = make_float4(len2 > 1e-30f ? 1.f / len2 : 0.f, by, __int_as_float(fl), 0.f);
                if (CULL) box[jl] = make_float4(fminf(ax, ax + dx), fminf(ay, ay + dy), fmaxf(ax, ax + dx), fmaxf(ay, ay + dy));
            }
        }
        __syncthreads();
        const int c = min(RS_CHORDS, cnt - j0);
        // one chord against the lane's four pixels; `near` is wave-uniform
        auto chord = [&](int jl, bool near) {
            const float4 A = rec[2 * jl], B = rec[2 * jl + 1];        // the same address in every lane
            if (FILL && (__builtin_amdgcn_readfirstlane(__float_as_int(B.z)) & 1)) {
#pragma unroll
                for (int r = 0; r < RS_PIX; ++r) {
                    inside[r] |= wind[r] != 0;
                    wind[r] = 0;
                }
            }
            const float px = cx - A.x;
#pragma unroll
            for (int r = 0; r < RS_PIX; ++r) {
                const float py = cy[r] - A.y;
                if (FILL) {
                    const float e = chord_side(A.z, A.w, px, py);
                    wind[r] += (int)(A.y <= cy[r] && cy[r] < B.y && e > 0.f) - (int)(B.y <= cy[r] && cy[r] < A.y && e < 0.f);
                }
                if (near) {
                    const float t = fminf(fmaxf(fmaf(px, A.z, py * A.w) * B.x, 0.f), 1.f);
                    const float qx = fmaf(-t, A.z, px), qy = fmaf(-t, A.w, py);
                    const float d2 = fmaf(qx, qx, qy * qy);
                    if (NN) {             // the value fminf keeps (d2 >= +0; a NaN loses either way), and who set it
                        if (d2 < m[r]) {
                            m[r] = d2;
                            mi[r] = j0 + jl;
                        }
                    } else m[r] = fminf(m[r], d2);
                }
            }
        };
        if (!CULL) {
            for (int jl = 0; jl < c; ++jl) chord(jl, true);
        } else {
            // 64 chords at a time: lane l tests the box of chord base + l against the wave's pixels, the ballot is the list
            // of chords within reach.  Stroke mode visits those only; fill mode visits every chord for its crossings
            for (int base = 0; base < c; base += 64) {
                bool within = false;
                if (base + lane < c) {
                    const float4 bb = box[base + lane];
                    const float gx = fmaxf(fmaxf(bb.x - qx1, qx0 - bb.z), 0.f), gy = fmaxf(fmaxf(bb.y - qy1, qy0 - bb.w), 0.f);
                    within = !(fmaf(gx, gx, gy * gy) > reach2);
                }
                unsigned long long mask = __ballot(within);
                if (FILL) {
                    const int end = min(base + 64, c);
                    for (int jl = base; jl < end; ++jl) chord(jl, (mask >> (jl - base)) & 1ull);
                } else {
                    while (mask) {
                        chord(base + __ffsll((long long)mask) - 1, true);
                        mask &= mask - 1ull;
                    }
                }
            }
        }
    }
    if (col >= size) return;
#pragma unroll
    for (int r = 0; r < RS_PIX; ++r) {
        if (row + 4 * r >= size) continue;
        const float d = sqrtf(m[r]);
        float ink;
        if (FILL) ink = (inside[r] | (wind[r] != 0)) ? 0.5f + d / s : 0.5f - d / s;
        else ink = 0.5f + (half_w - d) / s;
        ink = fminf(fmaxf(ink, 0.f), 1.f);
        out[(b * size + (row + 4 * r)) * size + col] = ink;
        if (NN) idx[(b * size + (row + 4 * r)) * size + col] = ink > 0.f && ink < 1.f ? mi[r] : -1;
    }
}

// Layered images (include/dsvg.h, "Layered images"): raster_sweep_kernel's tiling, chord tiles and chord expressions, with
// three canvas channels per pixel next to the running minimum and the winding count.  The records of an image are cut into
// layers by the layer table in LDS (dynamic: NL entries of paint r, g, b, opacity, then NL words `first record | mode << 28`;
// NL = G, or 1 with COMPOUND; layer g ends where the next one starts, the last one at the count).  A layer without records
// is skipped.  The walk over a chord tile stops at every layer end that falls into it and folds there: one sqrt per pixel,
// coverage by the layer's mode, the blend, m and wind reset.  Layer ends depend on the record index alone, so the fold is
// uniform over the workgroup and the layer's constants live in scalar registers.  An OUTLINE layer visits only the chords
// within reach of the wave (CULL); FILL and ERASE layers visit every chord for its crossings, as raster_sweep_kernel<true>.
// A table from another producer cannot lead out of bounds: entries are clamped into 0..count, a layer runs from wherever
// the layer before it ended, and entries that run backwards give layers without records.
constexpr int RL_MODE_SHIFT = 28;          // above every record offset (cap < 2^26)
constexpr int RL_ENTRY_BYTES = 20;

// NN (dsvg_raster_sweep_layers_nn): the minimum keeps the index of the record that set it, as raster_sweep_kernel's NN, and
// every fold also stores the layer's clamped coverage and that index (where 0 < cov < 1, -1 elsewhere) at [b, g]; a layer
// the walk passes over gets 0 and -1.  `cov` and `idx` are not touched without NN.
template <bool CULL, bool NN>
__global__ __launch_bounds__(RS_THREADS) void raster_sweep_layers_kernel(
    const float* __restrict__ segs, const int32_t* __restrict__ seg_counts, const int32_t* __restrict__ layer_first,
    const int32_t* __restrict__ modes, const float* __restrict__ paint, long long cap, int G, int NL, int size, int tiles, float s,
    float half_w, int compound_mode, int evenodd, float bg0, float bg1, float bg2, float* __restrict__ out,
    float* __restrict__ cov_out, int32_t* __restrict__ idx_out) {
    __shared__ __attribute__((aligned(16))) float4 rec[RS_CHORDS * 2];
    __shared__ __attribute__((aligned(16))) float4 box[CULL ? RS_CHORDS : 1];
    extern __shared__ __attribute__((aligned(16))) float4 lpaint[];
    int* lfirst = reinterpret_cast<int*>(lpaint + NL);
    const long long blk = blockIdx.x;
    const int tx = (int)(blk % tiles), ty = (int)((blk / tiles) % tiles);
    const long long b = blk / ((long long)tiles * tiles);
    const int cnt = chamfer_count(seg_counts, b, cap);
    const float* sg = segs + b * cap * RS_REC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col0 = tx * RS_TILE + (wave & 1) * RS_QUAD, row0 = ty * RS_TILE + (wave >> 1) * RS_QUAD;
    const int col = col0 + (lane & 15), row = row0 + (lane >> 4);
    const float cx = ((float)col + 0.5f) * s;
    float cy[RS_PIX], m[RS_PIX], cv0[RS_PIX], cv1[RS_PIX], cv2[RS_PIX];
    int wind[RS_PIX], mi[RS_PIX];
#pragma unroll
    for (int r = 0; r < RS_PIX; ++r) {
        cy[r] = ((float)(row + 4 * r) + 0.5f) * s;
        m[r] = INFINITY;
        wind[r] = 0;
        cv0[r] = bg0; cv1[r] = bg1; cv2[r] = bg2;
        if constexpr (NN) mi[r] = -1;
    }
    // NN: what layer gl keeps of the lane's pixel r (lanes past the image edge keep nothing)
    auto keep = [&](int gl, int r, float cov, int nearest) {
        if constexpr (NN) {
            if (col < size && row + 4 * r < size) {
                const long long o = ((b * NL + gl) * size + (row + 4 * r)) * size + col;
                cov_out[o] = cov;
                idx_out[o] = nearest;
            }
        }
    };
    auto pass_over = [&](int gl) {            // a layer without records
        if constexpr (NN) {
#pragma unroll
            for (int r = 0; r < RS_PIX; ++r) keep(gl, r, 0.f, -1);
        }
    };
    const float qx0 = ((float)col0 + 0.5f) * s, qx1 = ((float)(col0 + RS_QUAD - 1) + 0.5f) * s;
    const float qy0 = ((float)row0 + 0.5f) * s, qy1 = ((float)(row0 + RS_QUAD - 1) + 0.5f) * s;
    // the culling reach of raster_sweep_kernel, per layer mode
    const float reach_fill = (0.5f * s) * 1.001f + 0.01f, reach_line = (half_w + 0.5f * s) * 1.001f + 0.01f;
    const float reach2_fill = reach_fill * reach_fill, reach2_line = reach_line * reach_line;

    // ---- the layer table: values in 0..1 (a NaN reads as 0), offsets in 0..cnt, modes in 0..2 -------------------------------
    for (int g = tid; g < NL; g += RS_THREADS) {
        const float* p = paint + (b * G + g) * 4;
        auto unit = [](float v) { return fminf(fmaxf(v, 0.f), 1.f); };
        lpaint[g] = make_float4(unit(p[0]), unit(p[1]), unit(p[2]), unit(p[3]));
        int first = 0, mode = compound_mode;
        if (compound_mode < 0) {
            first = min(max(layer_first[b * (G + 1) + g], 0), cnt);
            mode = modes[b * G + g];
            mode = mode == DSVG_LAYER_FILL || mode == DSVG_LAYER_ERASE ? mode : DSVG_LAYER_OUTLINE;
        }
        lfirst[g] = first | (mode << RL_MODE_SHIFT);
    }
    __syncthreads();
    auto end_of = [&](int g) {        // wave-uniform: the record at which layer g ends
        return __builtin_amdgcn_readfirstlane(g + 1 < NL ? lfirst[g + 1] & ((1 << RL_MODE_SHIFT) - 1) : cnt);
    };
    int g = 0;                        // the layer the next record belongs to: the first one that ends past it
    while (g < NL && end_of(g) <= 0) {
        pass_over(g);
        ++g;
    }

    for (int j0 = 0; j0 < cnt; j0 += RS_CHORDS) {
        if (j0) __syncthreads();                       // the tile of the step before has been read
#pragma unroll
        for (int h = 0; h < RS_CHORDS / RS_THREADS; ++h) {
            const int jl = h * RS_THREADS + tid, j = j0 + jl;
            if (j < cnt) {
                const float* r = sg + (long long)j * RS_REC;
                const float ax = r[0], ay = r[1], dx = r[2], dy = r[3];
                const int fl = __float_as_int(r[4]);
                const float len2 = fmaf(dx, dx, dy * dy);
                const float by = chord_end_y(sg, j, cnt, ay, dy, fl);      // (as raster_sweep_kernel<true> takes it)
                rec[2 * jl] = make_float4(ax, ay, dx, dy);
                rec[2 * jl + 1] = make_float4(len2 > 1e-30f ? 1.f / len2 : 0.f, by, 0.f, 0.f);
                if (CULL) box[jl] = make_float4(fminf(ax, ax + dx), fminf(ay, ay + dy), fmaxf(ax, ax + dx), fmaxf(ay, ay + dy));
            }
        }
        __syncthreads();
        const int c = min(RS_CHORDS, cnt - j0);
        // one chord against the lane's four pixels; `near` is wave-uniform
        auto chord = [&](int jl, bool near, auto filled) {
            const float4 A = rec[2 * jl], B = rec[2 * jl + 1];        // the same address in every lane
            const float px = cx - A.x;
#pragma unroll
            for (int r = 0; r < RS_PIX; ++r) {
                const float py = cy[r] - A.y;
                if (filled.value) {
                    const float e = chord_side(A.z, A.w, px, py);
                    wind[r] += (int)(A.y <= cy[r] && cy[r] < B.y && e > 0.f) - (int)(B.y <= cy[r] && cy[r] < A.y && e < 0.f);
                }
                if (near) {
                    const float t = fminf(fmaxf(fmaf(px, A.z, py * A.w) * B.x, 0.f), 1.f);
                    const float qx = fmaf(-t, A.z, px), qy = fmaf(-t, A.w, py);
                    if constexpr (NN) {   // the value fminf keeps and who set it, as raster_sweep_kernel
                        const float d2 = fmaf(qx, qx, qy * qy);
                        if (d2 < m[r]) {
                            m[r] = d2;
                            mi[r] = j0 + jl;
                        }
                    } else m[r] = fminf(m[r], fmaf(qx, qx, qy * qy));
                }
            }
        };
        // chords lo..hi - 1 of the tile, all of one layer
        auto run = [&](int lo, int hi, auto filled) {
            if (!CULL) {
                for (int jl = lo; jl < hi; ++jl) chord(jl, true, filled);
            } else {
                const float reach2 = filled.value ? reach2_fill : reach2_line;
                for (int base = lo; base < hi; base += 64) {
                    bool within = false;
                    if (base + lane < hi) {
                        const float4 bb = box[base + lane];
                        const float gx = fmaxf(fmaxf(bb.x - qx1, qx0 - bb.z), 0.f), gy = fmaxf(fmaxf(bb.y - qy1, qy0 - bb.w), 0.f);
                        within = !(fmaf(gx, gx, gy * gy) > reach2);
                    }
                    unsigned long long mask = __ballot(within);
                    if (filled.value) {
                        const int end = min(base + 64, hi);
                        for (int jl = base; jl < end; ++jl) chord(jl, (mask >> (jl - base)) & 1ull, filled);
                    } else {
                        while (mask) {
                            chord(base + __ffsll((long long)mask) - 1, true, filled);
                            mask &= mask - 1ull;
                        }
                    }
                }
            }
        };
        int jl = 0;
        while (jl < c) {                               // g < NL here: the last layer ends at cnt
            const int le = end_of(g), hi = min(c, le - j0);
            const int mode = __builtin_amdgcn_readfirstlane(lfirst[g]) >> RL_MODE_SHIFT;
            if (mode == DSVG_LAYER_OUTLINE) run(jl, hi, std::false_type{});
            else run(jl, hi, std::true_type{});
            jl = hi;
            if (j0 + hi < le) break;                   // the layer goes on in the next tile
            // ---- the layer is complete: fold it into the canvas ------------------------------------------------------------
            const float4 P = lpaint[g];
            const float opacity = P.w;
            const float p0 = mode == DSVG_LAYER_ERASE ? bg0 : P.x, p1 = mode == DSVG_LAYER_ERASE ? bg1 : P.y;
            const float p2 = mode == DSVG_LAYER_ERASE ? bg2 : P.z;
#pragma unroll
            for (int r = 0; r < RS_PIX; ++r) {
                const float d = sqrtf(m[r]);
                float cov;
                if (mode == DSVG_LAYER_OUTLINE) cov = 0.5f + (half_w - d) / s;
                else cov = (evenodd ? wind[r] & 1 : wind[r] != 0) ? 0.5f + d / s : 0.5f - d / s;
                cov = fminf(fmaxf(cov, 0.f), 1.f);
                const float alpha = opacity * cov;
                cv0[r] = fmaf(alpha, p0 - cv0[r], cv0[r]);
                cv1[r] = fmaf(alpha, p1 - cv1[r], cv1[r]);
                cv2[r] = fmaf(alpha, p2 - cv2[r], cv2[r]);
                m[r] = INFINITY;
                wind[r] = 0;
                if constexpr (NN) {
                    keep(g, r, cov, cov > 0.f && cov < 1.f ? mi[r] : -1);
                    mi[r] = -1;
                }
            }
            ++g;
            while (g < NL && end_of(g) <= le) {
                pass_over(g);
                ++g;
            }
        }
    }
    if (col >= size) return;
    const long long plane = (long long)size * size;
#pragma unroll
    for (int r = 0; r < RS_PIX; ++r) {
        if (row + 4 * r >= size) continue;
        float* o = out + b * 3 * plane + (long long)(row + 4 * r) * size + col;
        o[0] = cv0[r]; o[plane] = cv1[r]; o[2 * plane] = cv2[r];
    }
}

constexpr int RB_THREADS = 256;

// One group of GW lanes (16, or a whole wave) per chord record j of image b.  The chord can be the saved nearest chord only
// of pixels whose ink is not saturated, i.e. whose centre lies within `reach` (the sweep's culling distance) of the chord's
// bounding box: the group walks that box, clipped to the image and one pixel wider against rounding, row-major with stride
// GW.  For a pixel with idx == j and 0 < ink < 1 as stored: t, q, d^2 by the sweep's expressions, d ink / d d = -1 / s (stroke
// and fill outside, ink <= 0.5) or +1 / s (fill inside), d d / d a = -(1 - t) q / d, d d / d b = -t q / d; d == 0 contributes
// nothing.  Every record below the image's count is written (zeros where no pixel points at it).
template <bool FILL, int GW>
__global__ __launch_bounds__(RB_THREADS) void raster_sweep_bwd_kernel(const float* __restrict__ segs, const int32_t* __restrict__ seg_counts,
                                                                      const float* __restrict__ out, const int32_t* __restrict__ idx,
                                                                      const float* __restrict__ dout, long long cap, int size,
                                                                      int blocks_per_image, float s, float reach,
                                                                      float* __restrict__ dsegs) {
    constexpr int PER = RB_THREADS / GW;                  // chords of a workgroup
    const long long b = blockIdx.x / blocks_per_image;
    const int j = (int)(blockIdx.x % blocks_per_image) * PER + (int)threadIdx.x / GW;
    const int l = (int)threadIdx.x % GW;
    const int cnt = chamfer_count(seg_counts, b, cap);
    if (j >= cnt) return;                                 // whole groups leave: the shuffles below stay inside a group
    const float* r = segs + (b * cap + j) * RS_REC;
    const float ax = r[0], ay = r[1], dx = r[2], dy = r[3];
    const float len2 = fmaf(dx, dx, dy * dy);
    const float inv = len2 > 1e-30f ? 1.f / len2 : 0.f;
    // pixel k has its centre at (k + 0.5) s; a NaN or an infinite vertex clamps to an empty or a full range, in bounds
    const float fsize = (float)size;
    auto first = [&](float v) { return (int)fminf(fmaxf(floorf((v - reach) / s - 0.5f), 0.f), fsize); };
    auto end = [&](float v) { return (int)fminf(fmaxf(ceilf((v + reach) / s - 0.5f) + 1.f, 0.f), fsize); };
    const int c0 = first(fminf(ax, ax + dx)), c1 = end(fmaxf(ax, ax + dx));
    const int r0 = first(fminf(ay, ay + dy)), r1 = end(fmaxf(ay, ay + dy));
    const int w = c1 - c0, np = w > 0 && r1 > r0 ? w * (r1 - r0) : 0;          // <= 4096^2
    const float* ob = out + b * size * size;
    const int32_t* ib = idx + b * size * size;
    const float* gb = dout + b * size * size;
    float sax = 0.f, say = 0.f, sbx = 0.f, sby = 0.f;
    for (int p = l; p < np; p += GW) {
        const int pr = p / w;
        const int row = r0 + pr, col = c0 + (p - pr * w);
        const long long pix = (long long)row * size + col;
        if (ib[pix] != j) continue;
        const float ink = ob[pix];
        if (!(ink > 0.f && ink < 1.f)) continue;
        const float px = ((float)col + 0.5f) * s - ax, py = ((float)row + 0.5f) * s - ay;
        const float t = fminf(fmaxf(fmaf(px, dx, py * dy) * inv, 0.f), 1.f);
        const float qx = fmaf(-t, dx, px), qy = fmaf(-t, dy, py);
        const float d2 = fmaf(qx, qx, qy * qy);
        if (!(d2 > 0.f)) continue;
        const float g = (FILL && ink > 0.5f ? gb[pix] : -gb[pix]) / (s * sqrtf(d2));          // dL/dd / d
        const float gx = g * qx, gy = g * qy;
        sax = fmaf(t - 1.f, gx, sax); say = fmaf(t - 1.f, gy, say);
        sbx = fmaf(-t, gx, sbx); sby = fmaf(-t, gy, sby);
    }
#pragma unroll
    for (int o = GW / 2; o; o >>= 1) {
        sax += __shfl_xor(sax, o, GW); say += __shfl_xor(say, o, GW);
        sbx += __shfl_xor(sbx, o, GW); sby += __shfl_xor(sby, o, GW);
    }
    if (l == 0) reinterpret_cast<float4*>(dsegs)[b * cap + j] = make_float4(sax, say, sbx, sby);
}

// The transpose of raster_segments_kernel<float>: dargs[b, t, :] from the vertex gradients dsegs[b, :, :] = d / d(ax, ay, bx,
// by) of every record.  The offsets are the forward's.  Vertex q of a command is the a of its chord q and the b of its chord
// q - 1; its weights are the Bernstein ones for `c` (what the forward's Horner form evaluates) and ((n - 1 - q), q) / (n - 1)
// for `l`, with vertex 0 the start point and vertex n - 1 the end position themselves.  A token sums, in this order: its own
// command's vertices (control1, control2, end), the vertices of the command on the row after it (whose start point is this
// row's end position, whatever this row holds; row 0's start is the constant (0, 0)), the a of the closing chord of the
// sub-path that ends at it and the b of the closing chord of the sub-path that starts on the row after it.  float64 sums,
// as sample_points_bwd_kernel; records at or past seg_counts[b] read as zero.  Every element of the row is written.
// LAYERS (dsvg_raster_segments_layers_bwd, the transpose of raster_segments_kernel<float, true>): `fill` is per group, read from
// modes[b, g] as the forward reads it; without LAYERS `modes` is not touched.
template <bool LAYERS>
__global__ __launch_bounds__(SP_THREADS) void raster_segments_bwd_kernel(const float* __restrict__ commands, const float* __restrict__ dsegs,
                                                                         const int32_t* __restrict__ seg_counts, int G, int L, int n,
                                                                         int fill, long long cap, float* __restrict__ dargs,
                                                                         const int32_t* __restrict__ modes) {
    __shared__ int pre[SP_MAX_TOK + 1];
    __shared__ int cl[SP_MAX_TOK + 1];
    __shared__ int last[SP_MAX_TOK];          // last token of the q-th sub-path
    __shared__ int wtot[SP_MAX_TOK / 64];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int T_ = G * L;
    const float* cmd = commands + b * T_;
    // whether the sub-paths of token t's group are closed (t < T_)
    auto closes = [&](int t) -> int {
        if constexpr (LAYERS) {
            const int m = modes[b * G + t / L];
            return m == DSVG_LAYER_FILL || m == DSVG_LAYER_ERASE;
        } else {
            return fill;
        }
    };
    block_flag_scan<SP_MAX_TOK>(T_, pre, wtot, [&](int t) { return is_drawing(cmd, t, T_); });
    if constexpr (LAYERS)
        block_flag_scan<SP_MAX_TOK>(T_, cl, wtot, [&](int t) { return subpath_ends(pre, t, T_, L, t < T_ ? closes(t) : 0); });
    else
        block_flag_scan<SP_MAX_TOK>(T_, cl, wtot, [&](int t) { return subpath_ends(pre, t, T_, L, fill); });
    for (int t = tid; t < T_; t += SP_THREADS)
        if (cl[t + 1] > cl[t]) last[cl[t]] = t;
    __syncthreads();
    const int cnt = chamfer_count(seg_counts, b, cap);
    const float4* ds = reinterpret_cast<const float4*>(dsegs) + b * cap;
    auto rec = [&](int o) { return o < cnt ? ds[o] : make_float4(0.f, 0.f, 0.f, 0.f); };
    float* out = dargs + b * T_ * N_ARGS;
    const double step = 1.0 / (double)(n - 1);
    for (int t = tid; t < T_; t += SP_THREADS) {
        const int i = t % L;
        // (ArgRowGrad of svg_seq.h written out: with the struct, or its updates as functions, hipcc orders this kernel differently)
        double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0, ex = 0.0, ey = 0.0;
        const bool draws = pre[t + 1] > pre[t];
        if (draws) {
            const bool cubic = (int)cmd[t] == CMD_C;
            const int o = pre[t] * (n - 1) + cl[t];
            for (int q = 1; q < n; ++q) {                  // (vertex 0 has no weight on this row)
                const float4 lo = rec(o + q - 1);
                double vx = (double)lo.z, vy = (double)lo.w;
                if (q < n - 1) {
                    const float4 hi = rec(o + q);
                    vx += (double)hi.x; vy += (double)hi.y;
                }
                const double z = q == n - 1 ? 1.0 : (double)q * step, w = 1.0 - z;
                if (cubic) {
                    const double w1 = 3.0 * w * w * z, w2 = 3.0 * w * z * z, w3 = z * z * z;
                    c1x += w1 * vx; c1y += w1 * vy;
                    c2x += w2 * vx; c2y += w2 * vy;
                    ex += w3 * vx; ey += w3 * vy;
                } else {
                    ex += z * vx; ey += z * vy;
                }
            }
        }
        const bool next_draws = i + 1 < L && pre[t + 2] > pre[t + 1];
        if (next_draws) {
            const bool cubic = (int)cmd[t + 1] == CMD_C;
            const int o = pre[t + 1] * (n - 1) + cl[t + 1];
            for (int q = 0; q < n - 1; ++q) {              // (vertex n - 1 has no weight on the start point)
                const float4 hi = rec(o + q);
                double vx = (double)hi.x, vy = (double)hi.y;
                if (q > 0) {
                    const float4 lo = rec(o + q - 1);
                    vx += (double)lo.z; vy += (double)lo.w;
                }
                const double w = 1.0 - (double)q * step;
                const double w0 = cubic ? w * w * w : w;
                ex += w0 * vx; ey += w0 * vy;
            }
        }
        if (LAYERS ? closes(t) : fill) {
            if (cl[t + 1] > cl[t]) {                       // a sub-path ends here: its closing chord starts at this end position
                const float4 c = rec((pre[t] + 1) * (n - 1) + cl[t]);
                ex += (double)c.x; ey += (double)c.y;
            }
            if (next_draws && !draws) {                    // a sub-path starts on the next row: its closing chord ends here
                const int te = last[cl[t + 1]];
                const float4 c = rec((pre[te] + 1) * (n - 1) + cl[te]);
                ex += (double)c.z; ey += (double)c.w;
            }
        }
        float* row = out + (long long)t * N_ARGS;
#pragma unroll
        for (int q = 0; q < 5; ++q) row[q] = 0.f;
        row[5] = (float)c1x; row[6] = (float)c1y; row[7] = (float)c2x; row[8] = (float)c2y;
        row[9] = (float)ex; row[10] = (float)ey;
    }
}

// The gradient of a layered image (include/dsvg.h, "Layered images: the gradient").
// The record at which layer g ends, as raster_sweep_layers_kernel clamps it
__device__ __forceinline__ int layer_end(const int32_t* __restrict__ layer_first, long long b, int G, int NL, int g, int cnt,
                                         int compound_mode) {
    return g + 1 < NL && compound_mode < 0 ? min(max(layer_first[b * (G + 1) + g + 1], 0), cnt) : cnt;
}

__device__ __forceinline__ int layer_mode(const int32_t* __restrict__ modes, long long b, int G, int g, int compound_mode) {
    if (compound_mode >= 0) return compound_mode;
    const int mode = modes[b * G + g];
    return mode == DSVG_LAYER_FILL || mode == DSVG_LAYER_ERASE ? mode : DSVG_LAYER_OUTLINE;
}

constexpr int BB_LIVE = 4;                 // bit of a layer word next to its mode (0..2): the layer has records

// The backward of the blend chain.  One workgroup of 1, 2 or 4 waves per image, one lane per pixel, 64 pixels of a wave at a
// time.  A layer has records exactly when its end lies past every end before it (the forward's walk passes over the
// others).  Forward walk over the layers that have records: the canvas by the forward's fmaf chain, and sum_c dout_c
// (p_c - C_{g-1,c}) left in the layer's dcov slot; reverse walk with T = prod_{k > g} (1 - alpha_k): d alpha = T * slot,
// dcov = d alpha * opacity, and the pixel's terms of d opacity (d alpha * cov) and d colour (T alpha dout_c; none on an ERASE
// layer) reduced over the wave by a fixed-shape __shfl_xor tree and added to the wave's own LDS accumulator of the layer by
// lane 0: a fixed order, no atomics.  The waves' accumulators are summed in wave order at the end; an element of paint
// outside 0..1 (the forward clamped it) or NaN gets 0.  LDS (dynamic): waves * NL float4, then 2 NL ints.
__global__ __launch_bounds__(256) void raster_blend_bwd_kernel(
    const float* __restrict__ cov, const int32_t* __restrict__ seg_counts, const int32_t* __restrict__ layer_first,
    const int32_t* __restrict__ modes, const float* __restrict__ paint, const float* __restrict__ dout, long long cap, int G,
    int NL, int size, int compound_mode, float bg0, float bg1, float bg2, float* __restrict__ dcov, float* __restrict__ dpaint) {
    extern __shared__ __attribute__((aligned(16))) float4 acc[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6;
    int* lend = reinterpret_cast<int*>(acc + nw * NL);
    int* lword = lend + NL;
    const long long b = blockIdx.x;
    const int cnt = chamfer_count(seg_counts, b, cap);
    const long long plane = (long long)size * size;
    for (int i = tid; i < nw * NL; i += (int)blockDim.x) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g = tid; g < NL; g += (int)blockDim.x) lend[g] = layer_end(layer_first, b, G, NL, g, cnt, compound_mode);
    __syncthreads();
    for (int g = tid; g < NL; g += (int)blockDim.x) {
        int before = 0;
        for (int k = 0; k < g; ++k) before = max(before, lend[k]);
        lword[g] = lend[g] > before ? layer_mode(modes, b, G, g, compound_mode) | BB_LIVE : 0;
    }
    __syncthreads();
    const float* cb = cov + b * NL * plane;
    float* db = dcov + b * NL * plane;
    const float* gb = dout + b * 3 * plane;
    const float* pb = paint + b * G * 4;
    auto unit = [](float v) { return fminf(fmaxf(v, 0.f), 1.f); };
    for (long long base = (long long)wave * 64; base < plane; base += blockDim.x) {          // wave-uniform
        const long long pix = base + lane;
        const bool on = pix < plane;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (on) {
            g0 = gb[pix]; g1 = gb[plane + pix]; g2 = gb[2 * plane + pix];
        }
        float c0 = bg0, c1 = bg1, c2 = bg2;
        for (int g = 0; g < NL; ++g) {
            const int word = __builtin_amdgcn_readfirstlane(lword[g]);
            if (!(word & BB_LIVE)) {
                if (on) db[g * plane + pix] = 0.f;
                continue;
            }
            const bool erase = (word & 3) == DSVG_LAYER_ERASE;
            const float* p = pb + g * 4;
            const float opacity = unit(p[3]);
            const float p0 = erase ? bg0 : unit(p[0]), p1 = erase ? bg1 : unit(p[1]), p2 = erase ? bg2 : unit(p[2]);
            if (on) {
                const float alpha = opacity * cb[g * plane + pix];
                const float e0 = p0 - c0, e1 = p1 - c1, e2 = p2 - c2;
                db[g * plane + pix] = fmaf(g2, e2, fmaf(g1, e1, g0 * e0));
                c0 = fmaf(alpha, e0, c0); c1 = fmaf(alpha, e1, c1); c2 = fmaf(alpha, e2, c2);
            }
        }
        float T = 1.f;
        for (int g = NL - 1; g >= 0; --g) {
            const int word = __builtin_amdgcn_readfirstlane(lword[g]);
            if (!(word & BB_LIVE)) continue;
            const bool erase = (word & 3) == DSVG_LAYER_ERASE;
            const float opacity = unit(pb[g * 4 + 3]);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            if (on) {
                const float cv = cb[g * plane + pix];
                const float alpha = opacity * cv;
                const float dalpha = T * db[g * plane + pix];
                db[g * plane + pix] = dalpha * opacity;
                s3 = dalpha * cv;
                if (!erase) {
                    const float ta = T * alpha;
                    s0 = ta * g0; s1 = ta * g1; s2 = ta * g2;
                }
                T = fmaf(-alpha, T, T);
            }
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64);
                s2 += __shfl_xor(s2, o, 64); s3 += __shfl_xor(s3, o, 64);
            }
            if (lane == 0) {
                float4 v = acc[wave * NL + g];
                v.x += s0; v.y += s1; v.z += s2; v.w += s3;
                acc[wave * NL + g] = v;
            }
        }
    }
    __syncthreads();
    for (int g = tid; g < G; g += (int)blockDim.x) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g < NL)
            for (int w = 0; w < nw; ++w) {
                const float4 a = acc[w * NL + g];
                v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            }
        const float* p = pb + g * 4;
        auto given = [](float x, float d) { return x >= 0.f && x <= 1.f ? d : 0.f; };
        reinterpret_cast<float4*>(dpaint)[b * G + g] = make_float4(given(p[0], v.x), given(p[1], v.y), given(p[2], v.z), given(p[3], v.w));
    }
}

// raster_sweep_bwd_kernel for a layered image: the layer of record j is the first one that ends past j (the forward's walk),
// its mode decides the sign rule and the reach, and cov, idx and dcov are read at [b, g].
template <int GW>
__global__ __launch_bounds__(RB_THREADS) void raster_sweep_layers_bwd_kernel(
    const float* __restrict__ segs, const int32_t* __restrict__ seg_counts, const int32_t* __restrict__ layer_first,
    const int32_t* __restrict__ modes, const float* __restrict__ cov, const int32_t* __restrict__ idx, const float* __restrict__ dcov,
    long long cap, int G, int NL, int size, int blocks_per_image, float s, float reach_line, float reach_fill, int compound_mode,
    float* __restrict__ dsegs) {
    constexpr int PER = RB_THREADS / GW;                  // chords of a workgroup
    const long long b = blockIdx.x / blocks_per_image;
    const int j = (int)(blockIdx.x % blocks_per_image) * PER + (int)threadIdx.x / GW;
    const int l = (int)threadIdx.x % GW;
    const int cnt = chamfer_count(seg_counts, b, cap);
    if (j >= cnt) return;                                 // whole groups leave: the shuffles below stay inside a group
    // a linear search, up to NL dependent loads per record, by every lane of the group: sized for the G of the data sets (8, at
    // most a few dozen), not for the 2048 the table may hold.  The ends of a foreign table need not be monotone, so a binary
    // search would not find the forward's layer; a running maximum of the ends in LDS would allow one
    int g = 0;
    while (g + 1 < NL && layer_end(layer_first, b, G, NL, g, cnt, compound_mode) <= j) ++g;
    const bool fill = layer_mode(modes, b, G, g, compound_mode) != DSVG_LAYER_OUTLINE;
    const float reach = fill ? reach_fill : reach_line;
    const float* r = segs + (b * cap + j) * RS_REC;
    const float ax = r[0], ay = r[1], dx = r[2], dy = r[3];
    const float len2 = fmaf(dx, dx, dy * dy);
    const float inv = len2 > 1e-30f ? 1.f / len2 : 0.f;
    const float fsize = (float)size;
    auto first = [&](float v) { return (int)fminf(fmaxf(floorf((v - reach) / s - 0.5f), 0.f), fsize); };
    auto end = [&](float v) { return (int)fminf(fmaxf(ceilf((v + reach) / s - 0.5f) + 1.f, 0.f), fsize); };
    const int c0 = first(fminf(ax, ax + dx)), c1 = end(fmaxf(ax, ax + dx));
    const int r0 = first(fminf(ay, ay + dy)), r1 = end(fmaxf(ay, ay + dy));
    const int w = c1 - c0, np = w > 0 && r1 > r0 ? w * (r1 - r0) : 0;          // <= 4096^2
    const long long layer = (b * NL + g) * size * size;
    const float* ob = cov + layer;
    const int32_t* ib = idx + layer;
    const float* gb = dcov + layer;
    float sax = 0.f, say = 0.f, sbx = 0.f, sby = 0.f;
    for (int p = l; p < np; p += GW) {
        const int pr = p / w;
        const int row = r0 + pr, col = c0 + (p - pr * w);
        const long long pix = (long long)row * size + col;
        if (ib[pix] != j) continue;
        const float ink = ob[pix];
        if (!(ink > 0.f && ink < 1.f)) continue;
        const float px = ((float)col + 0.5f) * s - ax, py = ((float)row + 0.5f) * s - ay;
        const float t = fminf(fmaxf(fmaf(px, dx, py * dy) * inv, 0.f), 1.f);
        const float qx = fmaf(-t, dx, px), qy = fmaf(-t, dy, py);
        const float d2 = fmaf(qx, qx, qy * qy);
        if (!(d2 > 0.f)) continue;
        const float gd = (fill && ink > 0.5f ? gb[pix] : -gb[pix]) / (s * sqrtf(d2));          // dL/dd / d
        const float gx = gd * qx, gy = gd * qy;
        sax = fmaf(t - 1.f, gx, sax); say = fmaf(t - 1.f, gy, say);
        sbx = fmaf(-t, gx, sbx); sby = fmaf(-t, gy, sby);
    }
#pragma unroll
    for (int o = GW / 2; o; o >>= 1) {
        sax += __shfl_xor(sax, o, GW); say += __shfl_xor(say, o, GW);
        sbx += __shfl_xor(sbx, o, GW); sby += __shfl_xor(sby, o, GW);
    }
    if (l == 0) reinterpret_cast<float4*>(dsegs)[b * cap + j] = make_float4(sax, say, sbx, sby);
}
}  // namespace

extern "C" int64_t dsvg_raster_workspace_bytes(int64_t n_images, int32_t G, int32_t L, int32_t n, int32_t fill) {
    if (n_images <= 0 || G < 1 || L < 1 || n < 2) return 0;
    return n_images * raster_cap(G, L, n, fill) * RS_REC * (int64_t)sizeof(float);
}

namespace {
// dsvg_raster_segments (modes and layer_first null) and dsvg_raster_segments_layers, refused under the name of the caller
int segments_launch(const char* name, int32_t itype, const void* commands, const void* args, int64_t B, int32_t G, int32_t L,
                    int32_t n, int32_t fill, void* segs, int64_t segs_bytes, int32_t* seg_counts, const int32_t* modes,
                    int32_t* layer_first, void* stream) {
    DSVG_CHECK_ARG(commands && args && segs && seg_counts, "%s: null pointer", name);
    DSVG_CHECK_ARG(itype == DSVG_F32 || itype == DSVG_I64, "%s: itype %d is neither DSVG_F32 nor DSVG_I64", name, itype);
    if (sequence_args_ok(name, "image", B, G, L, n)) return -1;
    const int64_t cap = raster_cap(G, L, n, fill);      // <= 2048 * 64: far below 2^31
    DSVG_CHECK_ARG(segs_bytes >= dsvg_raster_workspace_bytes(B, G, L, n, fill) && ((uintptr_t)segs & 3) == 0,
                   "%s: buffer of %lld bytes, need %lld (4-byte aligned)", name, (long long)segs_bytes,
                   (long long)dsvg_raster_workspace_bytes(B, G, L, n, fill));
    hipStream_t st = (hipStream_t)stream;
#define RS_SEGMENTS(T, LAYERS)                                                                                              \
    hipLaunchKernelGGL((raster_segments_kernel<T, LAYERS>), dim3((unsigned)B), dim3(SP_THREADS), 0, st, (const T*)commands,   \
                       (const T*)args, G, L, n, fill ? 1 : 0, (long long)cap, (float*)segs, seg_counts, modes, layer_first)
    if (modes) {
        if (itype == DSVG_I64) RS_SEGMENTS(long long, true);
        else RS_SEGMENTS(float, true);
    } else {
        if (itype == DSVG_I64) RS_SEGMENTS(long long, false);
        else RS_SEGMENTS(float, false);
    }
#undef RS_SEGMENTS
    DSVG_LAUNCH_CHECK(name);
    return 0;
}
}  // namespace

extern "C" int dsvg_raster_segments(int32_t itype, const void* commands, const void* args, int64_t B, int32_t G, int32_t L,
                                    int32_t n, int32_t fill, void* segs, int64_t segs_bytes, int32_t* seg_counts, void* stream) {
    return segments_launch("raster_segments", itype, commands, args, B, G, L, n, fill, segs, segs_bytes, seg_counts, nullptr,
                           nullptr, stream);
}

extern "C" int dsvg_raster_segments_layers(int32_t itype, const void* commands, const void* args, int64_t B, int32_t G,
                                           int32_t L, int32_t n, const int32_t* modes, void* segs, int64_t segs_bytes,
                                           int32_t* seg_counts, int32_t* layer_first, void* stream) {
    DSVG_CHECK_ARG(modes && layer_first, "raster_segments_layers: null pointer");
    return segments_launch("raster_segments_layers", itype, commands, args, B, G, L, n, 1, segs, segs_bytes, seg_counts, modes,
                           layer_first, stream);
}

namespace {
// the arguments dsvg_raster_sweep, _nn and _bwd share, refused under the name of the caller
int sweep_args_ok(const char* name, bool pointers, int64_t B, int64_t cap, int32_t size, float stroke_width, int32_t flags,
                  int32_t known_flags, int64_t groups) {
    DSVG_CHECK_ARG(size >= 1 && size <= RS_MAX_SIZE, "%s: size = %d pixels per side, need 1..%d", name, size, RS_MAX_SIZE);
    DSVG_CHECK_ARG(pointers, "%s: null pointer", name);
    DSVG_CHECK_ARG(stroke_width >= 0.f && stroke_width < 1e6f, "%s: stroke_width %g, need a finite width >= 0", name,
                   (double)stroke_width);
    DSVG_CHECK_ARG((flags & ~known_flags) == 0, "%s: unknown flags 0x%x", name, flags);
    DSVG_CHECK_ARG(B > 0 && cap > 0 && cap < (1ll << 26) && B * groups < (1ll << 31),
                   "%s: bad shape (B=%lld cap=%lld: %lld workgroups; chords per image below 2^26, workgroups below 2^31)", name,
                   (long long)B, (long long)cap, (long long)(B * groups));
    return 0;
}

int sweep_launch(const char* name, const void* segs, const int32_t* seg_counts, int64_t B, int64_t cap, int32_t size,
                 float stroke_width, int32_t flags, float* out, int32_t* idx, bool nn, void* stream) {
    const int64_t tiles = (size + RS_TILE - 1) / RS_TILE;
    if (sweep_args_ok(name, segs && seg_counts && out && (idx || !nn), B, cap, size, stroke_width, flags,
                      DSVG_RASTER_FILL | DSVG_RASTER_CULL, tiles * tiles))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * tiles * tiles)), block(RS_THREADS);
    const float s = 256.f / (float)size, half_w = 0.5f * stroke_width;
    const float* sg = (const float*)segs;
    const bool fill = flags & DSVG_RASTER_FILL, cull = flags & DSVG_RASTER_CULL;
#define RS_LAUNCH(F, C, N)                                                                                                  \
    hipLaunchKernelGGL((raster_sweep_kernel<F, C, N>), grid, block, 0, st, sg, seg_counts, (long long)cap, size, (int)tiles, s, \
                       half_w, out, idx)
#define RS_LAUNCH_NN(F, C)  \
    do {                    \
        if (nn) RS_LAUNCH(F, C, true); \
        else RS_LAUNCH(F, C, false);   \
    } while (0)
    if (fill && cull) RS_LAUNCH_NN(true, true);
    else if (fill) RS_LAUNCH_NN(true, false);
    else if (cull) RS_LAUNCH_NN(false, true);
    else RS_LAUNCH_NN(false, false);
#undef RS_LAUNCH_NN
#undef RS_LAUNCH
    DSVG_LAUNCH_CHECK(name);
    return 0;
}
}  // namespace

extern "C" int dsvg_raster_sweep(const void* segs, const int32_t* seg_counts, int64_t B, int64_t cap, int32_t size,
                                 float stroke_width, int32_t flags, float* out, void* stream) {
    return sweep_launch("raster_sweep", segs, seg_counts, B, cap, size, stroke_width, flags, out, nullptr, false, stream);
}

extern "C" int dsvg_raster_sweep_nn(const void* segs, const int32_t* seg_counts, int64_t B, int64_t cap, int32_t size,
                                    float stroke_width, int32_t flags, float* out, int32_t* idx, void* stream) {
    return sweep_launch("raster_sweep_nn", segs, seg_counts, B, cap, size, stroke_width, flags, out, idx, true, stream);
}

namespace {
// what the layered entry points take a `flags` word for, and the tables a layered (not compound) image needs
constexpr int32_t RL_FLAGS = DSVG_RASTER_CULL | DSVG_RASTER_EVENODD | DSVG_RASTER_COMPOUND;

int layers_args_ok(const char* name, int32_t G, const float* background) {
    DSVG_CHECK_ARG(G >= 1 && G <= SP_MAX_TOK, "%s: G = %d layers per image, need 1..%d", name, G, SP_MAX_TOK);
    for (int q = 0; q < 3; ++q)
        DSVG_CHECK_ARG(background[q] >= 0.f && background[q] <= 1.f, "%s: background[%d] = %g, need 0..1", name, q,
                       (double)background[q]);
    return 0;
}

int layer_compound_mode(int32_t flags) {
    return flags & DSVG_RASTER_COMPOUND ? (flags & DSVG_RASTER_FILL ? DSVG_LAYER_FILL : DSVG_LAYER_OUTLINE) : -1;
}

// dsvg_raster_sweep_layers (cov and idx null) and dsvg_raster_sweep_layers_nn, refused under the name of the caller
int sweep_layers_launch(const char* name, const void* segs, const int32_t* seg_counts, const int32_t* layer_first,
                        const int32_t* modes, const float* paint, const float* background, int64_t B, int64_t cap, int32_t G,
                        int32_t size, float stroke_width, int32_t flags, float* out, float* cov, int32_t* idx, bool nn,
                        void* stream) {
    const int64_t tiles = (size + RS_TILE - 1) / RS_TILE;
    const bool compound = flags & DSVG_RASTER_COMPOUND;
    if (sweep_args_ok(name, segs && seg_counts && paint && background && out && (compound || (layer_first && modes)) &&
                                (!nn || (cov && idx)),
                      B, cap, size, stroke_width, flags, RL_FLAGS | (compound ? DSVG_RASTER_FILL : 0), tiles * tiles))
        return -1;
    if (layers_args_ok(name, G, background)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * tiles * tiles)), block(RS_THREADS);
    const float s = 256.f / (float)size, half_w = 0.5f * stroke_width;
    const int NL = compound ? 1 : G;
    const int compound_mode = layer_compound_mode(flags);
#define RL_LAUNCH(C, N)                                                                                                       \
    hipLaunchKernelGGL((raster_sweep_layers_kernel<C, N>), grid, block, (size_t)NL * RL_ENTRY_BYTES, st, (const float*)segs,   \
                       seg_counts, layer_first, modes, paint, (long long)cap, G, NL, size, (int)tiles, s, half_w, compound_mode, \
                       flags & DSVG_RASTER_EVENODD ? 1 : 0, background[0], background[1], background[2], out, cov, idx)
    if (nn) {
        if (flags & DSVG_RASTER_CULL) RL_LAUNCH(true, true);
        else RL_LAUNCH(false, true);
    } else {
        if (flags & DSVG_RASTER_CULL) RL_LAUNCH(true, false);
        else RL_LAUNCH(false, false);
    }
#undef RL_LAUNCH
    DSVG_LAUNCH_CHECK(name);
    return 0;
}
}  // namespace

extern "C" int dsvg_raster_sweep_layers(const void* segs, const int32_t* seg_counts, const int32_t* layer_first,
                                        const int32_t* modes, const float* paint, const float* background, int64_t B,
                                        int64_t cap, int32_t G, int32_t size, float stroke_width, int32_t flags, float* out,
                                        void* stream) {
    return sweep_layers_launch("raster_sweep_layers", segs, seg_counts, layer_first, modes, paint, background, B, cap, G, size,
                               stroke_width, flags, out, nullptr, nullptr, false, stream);
}

extern "C" int dsvg_raster_sweep_layers_nn(const void* segs, const int32_t* seg_counts, const int32_t* layer_first,
                                           const int32_t* modes, const float* paint, const float* background, int64_t B,
                                           int64_t cap, int32_t G, int32_t size, float stroke_width, int32_t flags, float* out,
                                           float* cov, int32_t* idx, void* stream) {
    return sweep_layers_launch("raster_sweep_layers_nn", segs, seg_counts, layer_first, modes, paint, background, B, cap, G, size,
                               stroke_width, flags, out, cov, idx, true, stream);
}

extern "C" int dsvg_raster_blend_bwd(const float* cov, const int32_t* seg_counts, const int32_t* layer_first, const int32_t* modes,
                                     const float* paint, const float* background, const float* dout, int64_t B, int64_t cap,
                                     int32_t G, int32_t size, int32_t flags, float* dcov, float* dpaint, void* stream) {
    const bool compound = flags & DSVG_RASTER_COMPOUND;
    if (sweep_args_ok("raster_blend_bwd", cov && seg_counts && paint && background && dout && dcov && dpaint &&
                                              (compound || (layer_first && modes)),
                      B, cap, size, 0.f, flags, RL_FLAGS | (compound ? DSVG_RASTER_FILL : 0), 1))
        return -1;
    if (layers_args_ok("raster_blend_bwd", G, background)) return -1;
    DSVG_CHECK_ARG(((uintptr_t)dpaint & 15) == 0, "raster_blend_bwd: dpaint must be 16-byte aligned");
    const int NL = compound ? 1 : G;
    // as many waves as have their accumulators in 64 KiB of LDS next to the layer words: 4 up to 910 layers, 1 at 2048
    int waves = 4;
    while (waves > 1 && (size_t)NL * (16 * waves + 8) > 65536) waves >>= 1;
    hipLaunchKernelGGL(raster_blend_bwd_kernel, dim3((unsigned)B), dim3(64 * waves), (size_t)NL * (16 * waves + 8),
                       (hipStream_t)stream, cov, seg_counts, layer_first, modes, paint, dout, (long long)cap, G, NL, size,
                       layer_compound_mode(flags), background[0], background[1], background[2], dcov, dpaint);
    DSVG_LAUNCH_CHECK("raster_blend_bwd");
    return 0;
}

extern "C" int dsvg_raster_sweep_layers_bwd(const void* segs, const int32_t* seg_counts, const int32_t* layer_first,
                                            const int32_t* modes, const float* cov, const int32_t* idx, const float* dcov,
                                            int64_t B, int64_t cap, int32_t G, int32_t size, float stroke_width, int32_t flags,
                                            float* dsegs, void* stream) {
    const bool compound = flags & DSVG_RASTER_COMPOUND, wide = flags & DSVG_RASTER_WIDE;
    const int per = RB_THREADS / (wide ? 64 : 16);
    const int64_t bpi = (cap + per - 1) / per;
    if (sweep_args_ok("raster_sweep_layers_bwd", segs && seg_counts && cov && idx && dcov && dsegs && (compound || (layer_first && modes)),
                      B, cap, size, stroke_width, flags, RL_FLAGS | DSVG_RASTER_WIDE | (compound ? DSVG_RASTER_FILL : 0), bpi))
        return -1;
    DSVG_CHECK_ARG(G >= 1 && G <= SP_MAX_TOK, "raster_sweep_layers_bwd: G = %d layers per image, need 1..%d", G, SP_MAX_TOK);
    DSVG_CHECK_ARG(((uintptr_t)dsegs & 15) == 0, "raster_sweep_layers_bwd: dsegs must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * bpi)), block(RB_THREADS);
    const float s = 256.f / (float)size;
    // as raster_sweep_layers_kernel culls, per layer mode
    const float reach_fill = (0.5f * s) * 1.001f + 0.01f, reach_line = (0.5f * stroke_width + 0.5f * s) * 1.001f + 0.01f;
#define RB_LAUNCH(W)                                                                                                          \
    hipLaunchKernelGGL((raster_sweep_layers_bwd_kernel<W>), grid, block, 0, st, (const float*)segs, seg_counts, layer_first,   \
                       modes, cov, idx, dcov, (long long)cap, G, compound ? 1 : G, size, (int)bpi, s, reach_line, reach_fill,  \
                       layer_compound_mode(flags), dsegs)
    if (wide) RB_LAUNCH(64);
    else RB_LAUNCH(16);
#undef RB_LAUNCH
    DSVG_LAUNCH_CHECK("raster_sweep_layers_bwd");
    return 0;
}

extern "C" int dsvg_raster_sweep_bwd(const void* segs, const int32_t* seg_counts, const float* out, const int32_t* idx,
                                     const float* dout, int64_t B, int64_t cap, int32_t size, float stroke_width, int32_t flags,
                                     float* dsegs, void* stream) {
    const bool fill = flags & DSVG_RASTER_FILL, wide = flags & DSVG_RASTER_WIDE;
    const int per = RB_THREADS / (wide ? 64 : 16);
    const int64_t bpi = (cap + per - 1) / per;
    if (sweep_args_ok("raster_sweep_bwd", segs && seg_counts && out && idx && dout && dsegs, B, cap, size, stroke_width, flags,
                      DSVG_RASTER_FILL | DSVG_RASTER_WIDE, bpi))
        return -1;
    DSVG_CHECK_ARG(((uintptr_t)dsegs & 15) == 0, "raster_sweep_bwd: dsegs must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * bpi)), block(RB_THREADS);
    const float s = 256.f / (float)size;
    const float reach = (fill ? 0.5f * s : 0.5f * stroke_width + 0.5f * s) * 1.001f + 0.01f;      // as raster_sweep_kernel culls
#define RB_LAUNCH(F, W)                                                                                                  \
    hipLaunchKernelGGL((raster_sweep_bwd_kernel<F, W>), grid, block, 0, st, (const float*)segs, seg_counts, out, idx, dout, \
                       (long long)cap, size, (int)bpi, s, reach, dsegs)
    if (fill && wide) RB_LAUNCH(true, 64);
    else if (fill) RB_LAUNCH(true, 16);
    else if (wide) RB_LAUNCH(false, 64);
    else RB_LAUNCH(false, 16);
#undef RB_LAUNCH
    DSVG_LAUNCH_CHECK("raster_sweep_bwd");
    return 0;
}

extern "C" int dsvg_raster_segments_bwd(const float* commands, const float* dsegs, const int32_t* seg_counts, int64_t B,
                                        int32_t G, int32_t L, int32_t n, int32_t fill, float* dargs, void* stream) {
    DSVG_CHECK_ARG(commands && dsegs && seg_counts && dargs, "raster_segments_bwd: null pointer");
    if (sequence_args_ok("raster_segments_bwd", "image", B, G, L, n)) return -1;
    DSVG_CHECK_ARG(((uintptr_t)dsegs & 15) == 0, "raster_segments_bwd: dsegs must be 16-byte aligned");
    hipLaunchKernelGGL(raster_segments_bwd_kernel<false>, dim3((unsigned)B), dim3(SP_THREADS), 0, (hipStream_t)stream, commands,
                       dsegs, seg_counts, G, L, n, fill ? 1 : 0, (long long)raster_cap(G, L, n, fill), dargs,
                       (const int32_t*)nullptr);
    DSVG_LAUNCH_CHECK("raster_segments_bwd");
    return 0;
}

extern "C" int dsvg_raster_segments_layers_bwd(const float* commands, const float* dsegs, const int32_t* seg_counts,
                                               const int32_t* modes, int64_t B, int32_t G, int32_t L, int32_t n, float* dargs,
                                               void* stream) {
    DSVG_CHECK_ARG(commands && dsegs && seg_counts && modes && dargs, "raster_segments_layers_bwd: null pointer");
    if (sequence_args_ok("raster_segments_layers_bwd", "image", B, G, L, n)) return -1;
    DSVG_CHECK_ARG(((uintptr_t)dsegs & 15) == 0, "raster_segments_layers_bwd: dsegs must be 16-byte aligned");
    hipLaunchKernelGGL(raster_segments_bwd_kernel<true>, dim3((unsigned)B), dim3(SP_THREADS), 0, (hipStream_t)stream, commands,
                       dsegs, seg_counts, G, L, n, 1, (long long)raster_cap(G, L, n, 1), dargs, modes);
    DSVG_LAUNCH_CHECK("raster_segments_layers_bwd");
    return 0;
}
