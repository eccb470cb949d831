// Filling of a decoded batch: which groups of an icon are filled, which are holes, and in what order to paint them - what the
// reference works out one icon at a time on the host with shapely polygons and a networkx graph (SVGPathGroup.overlap_graph and
// compute_filling, deepsvg/svglib/svg_primitive.py:392-441, called on all sub-paths of an icon by SVG.canonicalize_new,
// svg.py:312-331).  The overlap measure is this package's own, on the rasteriser's machinery: the chord records of
// dsvg_raster_segments_layers and the half-open crossing rule of csrc/raster.hip (chord_side, svg_seq.h).  The definition is
// in include/dsvg.h; tests/paths_fill_ref.py restates it in float64.
//   dsvg_overlap_counts       raster_sweep_layers_kernel's tiling without its distance work: one workgroup per (icon, tile of
//                             32 x 32 samples), a wave owns a 16 x 16 quadrant, a lane four samples; the icon's chords stream
//                             through LDS in tiles of RS_CHORDS (broadcast reads); a running winding count per sample, folded
//                             into bit g of the sample's membership mask at group g's last record.  A wave visits only the
//                             chords whose y-range meets its sample rows (a ballot per 64 chords).  After the sweep the counts
//                             are popcounts of ballots over the groups the wave has met, summed in LDS per workgroup and added
//                             to the int32 tables with integer atomics: order-independent, so bit-reproducible.
//   dsvg_filling_from_counts  one lane per icon: the cover graph as 32-bit adjacency masks, the orientation of every group, the
//                             level-by-level walk of compute_filling and the paint order.  Not hot.
#include "dsvg_common.h"
#include "svg_seq.h"
#include "../../include/dsvg.h"

namespace {
constexpr int PF_MAX_GROUPS = 32;         // one mask word
constexpr int PF_MIN_SAMPLES = 8, PF_MAX_SAMPLES = 1024;
constexpr int PF_THREADS = 64;            // icons per workgroup of filling_from_counts_kernel

// Workgroup (icon b, tile row ty, tile column tx) of the K x K samples at the sweep's pixel centres for size = K.  gend[g] is
// the record at which group g ends: layer_first[g + 1] clamped into 0..count and made non-decreasing, the last one the
// count, so that a table from any producer leads nowhere out of bounds.  Group ends depend on the record index alone, so the
// fold is uniform over the workgroup.
__global__ __launch_bounds__(RS_THREADS) void overlap_counts_kernel(const float* __restrict__ segs, const int32_t* __restrict__ seg_counts,
                                                                    const int32_t* __restrict__ layer_first, long long cap, int G,
                                                                    int K, int tiles, float s, int evenodd,
                                                                    int32_t* __restrict__ area, int32_t* __restrict__ inter) {
    __shared__ __attribute__((aligned(16))) float4 rec[RS_CHORDS];      // ax, ay, dx, dy
    __shared__ float eby[RS_CHORDS];                                      // chord_end_y
    __shared__ int gend[PF_MAX_GROUPS];
    __shared__ int acc[PF_MAX_GROUPS * PF_MAX_GROUPS];                    // [i * G + j], i <= j
    const long long blk = blockIdx.x;
    const int tx = (int)(blk % tiles), ty = (int)((blk / tiles) % tiles);
    const long long b = blk / ((long long)tiles * tiles);
    const int cnt = chamfer_count(seg_counts, b, cap);
    const float* sg = segs + b * cap * RS_REC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col0 = tx * RS_TILE + (wave & 1) * RS_QUAD, row0 = ty * RS_TILE + (wave >> 1) * RS_QUAD;
    const int col = col0 + (lane & 15), row = row0 + (lane >> 4);
    const float cx = ((float)col + 0.5f) * s;
    float cy[RS_PIX];
    int wind[RS_PIX];
    unsigned member[RS_PIX];
#pragma unroll
    for (int r = 0; r < RS_PIX; ++r) {
        cy[r] = ((float)(row + 4 * r) + 0.5f) * s;
        wind[r] = 0;
        member[r] = 0u;
    }
    // the wave's sample rows span [qy0, qy1]
    const float qy0 = ((float)row0 + 0.5f) * s, qy1 = ((float)(row0 + RS_QUAD - 1) + 0.5f) * s;

    for (int q = tid; q < G * G; q += RS_THREADS) acc[q] = 0;
    if (tid == 0) {
        int e = 0;
        for (int g = 0; g + 1 < G; ++g) {
            e = max(e, min(max(layer_first[b * (G + 1) + g + 1], 0), cnt));
            gend[g] = e;
        }
        gend[G - 1] = cnt;
    }
    __syncthreads();
    auto end_of = [&](int g) { return __builtin_amdgcn_readfirstlane(gend[g]); };
    int g = 0;                        // the group the next record belongs to: the first one that ends past it
    while (g < G - 1 && end_of(g) <= 0) ++g;

    for (int j0 = 0; j0 < cnt; j0 += RS_CHORDS) {
        if (j0) __syncthreads();                       // the tile of the step before has been read
#pragma unroll
        for (int h = 0; h < RS_CHORDS / RS_THREADS; ++h) {
            const int jl = h * RS_THREADS + tid, j = j0 + jl;
            if (j < cnt) {
                const float* r = sg + (long long)j * RS_REC;
                const float ax = r[0], ay = r[1], dx = r[2], dy = r[3];
                rec[jl] = make_float4(ax, ay, dx, dy);
                eby[jl] = chord_end_y(sg, j, cnt, ay, dy, __float_as_int(r[4]));
            }
        }
        __syncthreads();
        const int c = min(RS_CHORDS, cnt - j0);
        int jl = 0;
        while (jl < c) {                               // g <= G - 1 here: the last group ends at cnt
            const int le = end_of(g), hi = min(c, le - j0);
            // chords jl..hi - 1 of the tile, all of group g; 64 at a time: lane l tests the y-range of chord base + l against
            // the wave's sample rows, the ballot is the list of chords that can cross one of them
            for (int base = jl; base < hi; base += 64) {
                bool meets = false;
                if (base + lane < hi) {
                    const float ay = rec[base + lane].y, by = eby[base + lane];
                    meets = fminf(ay, by) <= qy1 && fmaxf(ay, by) > qy0;
                }
                unsigned long long todo = __ballot(meets);
                while (todo) {
                    const int k = base + __ffsll((long long)todo) - 1;
                    todo &= todo - 1ull;
                    const float4 A = rec[k];                              // the same address in every lane
                    const float by = eby[k];
                    const float px = cx - A.x;
#pragma unroll
                    for (int r = 0; r < RS_PIX; ++r) {
                        // the sweeps' sign test with its rounding residual taken out (svg_seq.h): a sample ON a chord counts nothing
                        const float e = chord_side<true>(A.z, A.w, px, cy[r] - A.y);
                        wind[r] += (int)(A.y <= cy[r] && cy[r] < by && e > 0.f) - (int)(by <= cy[r] && cy[r] < A.y && e < 0.f);
                    }
                }
            }
            jl = hi;
            if (j0 + hi < le) break;                   // the group goes on in the next tile
            // ---- the group is complete: fold it into bit g ------------------------------------------------------------------
#pragma unroll
            for (int r = 0; r < RS_PIX; ++r) {
                member[r] |= (unsigned)(evenodd ? wind[r] & 1 : wind[r] != 0) << g;
                wind[r] = 0;
            }
            if (g == G - 1) break;                     // (hi == c here)
            ++g;
            while (g < G - 1 && end_of(g) <= le) ++g;  // groups without records keep bit 0
        }
    }
    // samples past K in ragged tiles count nothing
#pragma unroll
    for (int r = 0; r < RS_PIX; ++r)
        if (col >= K || row + 4 * r >= K) member[r] = 0u;

    // ---- counts: popcounts of ballots over the groups this wave has met -------------------------------------------------------
    unsigned met = member[0] | member[1] | member[2] | member[3];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) met |= (unsigned)__shfl_xor((int)met, o, 64);
    met = (unsigned)__builtin_amdgcn_readfirstlane((int)met);
    for (unsigned ri = met; ri;) {
        const int i = __ffs((int)ri) - 1;
        ri &= ri - 1u;
        int n = 0;
#pragma unroll
        for (int r = 0; r < RS_PIX; ++r) n += __popcll(__ballot((member[r] >> i) & 1u));
        if (lane == 0) atomicAdd(&acc[i * G + i], n);
        for (unsigned rj = ri; rj;) {
            const int j = __ffs((int)rj) - 1;
            rj &= rj - 1u;
            int m = 0;
#pragma unroll
            for (int r = 0; r < RS_PIX; ++r) m += __popcll(__ballot((member[r] >> i) & (member[r] >> j) & 1u));
            if (lane == 0 && m) atomicAdd(&acc[i * G + j], m);
        }
    }
    __syncthreads();
    for (int q = tid; q < G * G; q += RS_THREADS) {
        const int i = q / G, j = q - i * G;
        const int v = acc[q];
        if (i > j || v == 0) continue;
        atomicAdd(&inter[(b * G + i) * G + j], v);
        if (i == j) atomicAdd(&area[b * G + i], v);
        else atomicAdd(&inter[(b * G + j) * G + i], v);
    }
}

// One lane per icon.  Masks: bit j of cov[i] = "j covers i" (an edge j -> i), bit i of out[j] the same edge from its source.
template <typename T>
__global__ __launch_bounds__(PF_THREADS) void filling_from_counts_kernel(
    const int32_t* __restrict__ area, const int32_t* __restrict__ inter, const T* __restrict__ commands, const T* __restrict__ args,
    const uint8_t* __restrict__ participating, long long N, int G, int S, double threshold, int rule,
    long long* __restrict__ filling, int32_t* __restrict__ depth, int32_t* __restrict__ parent, uint8_t* __restrict__ clockwise,
    long long* __restrict__ paint_order) {
    const long long b = (long long)blockIdx.x * PF_THREADS + threadIdx.x;
    if (b >= N) return;
    const int32_t* ar = area + b * G;
    const int32_t* in = inter + b * G * G;
    long long* fil = filling + b * G;
    int32_t* dep = depth + b * G;
    int32_t* par = parent + b * G;
    unsigned cov[PF_MAX_GROUPS], out[PF_MAX_GROUPS];
    int dv[PF_MAX_GROUPS], via[PF_MAX_GROUPS];

    // ---- participation, orientation ---------------------------------------------------------------------------------------
    unsigned part = 0u, cw = 0u;
    for (int i = 0; i < G; ++i) {
        if (participating[b * G + i] && ar[i] > 0) part |= 1u << i;
        const T* cmd = commands + (b * G + i) * S;
        const T* arg = args + (b * G + i) * S * N_ARGS;
        int n = 0;
        double det = 0.0;
        bool single = true;
        for (int t = 0; t < S; ++t) {
            if (!is_drawing(cmd, t, S)) continue;
            const float2 p = start_point(arg + (long long)t * N_ARGS, t);
            const float fx = (float)arg[(long long)t * N_ARGS + ARG_END], fy = (float)arg[(long long)t * N_ARGS + ARG_END + 1];
            if (n == 0) single = single_command_clockwise(p.x, p.y, fx, fy);
            det += orientation_term(p.x, p.y, fx, fy);
            ++n;
        }
        const bool c = n == 1 ? single : det >= 0.0;
        if (c) cw |= 1u << i;
        clockwise[b * G + i] = c ? 1 : 0;
        fil[i] = DSVG_LAYER_OUTLINE;
        dep[i] = -1;
        par[i] = -1;
        cov[i] = 0u;
        out[i] = 0u;
        dv[i] = 0;
        via[i] = -1;
    }
    // ---- edges ------------------------------------------------------------------------------------------------------------------
    for (int i = 0; i < G; ++i) {
        if (!((part >> i) & 1u)) continue;
        const double need = threshold * (double)ar[i];
        for (int j = 0; j < G; ++j)
            if (j != i && ((part >> j) & 1u) && (double)in[i * G + j] > need) {
                cov[i] |= 1u << j;
                out[j] |= 1u << i;
            }
    }
    // ---- the walk (svg_primitive.py:396-418): roots in ascending order, each level in ascending order ---------------------------
    unsigned alive = part, roots = 0u;
    for (int i = 0; i < G; ++i)
        if (((part >> i) & 1u) && cov[i] == 0u) roots |= 1u << i;
    while (roots) {
        const int root = __ffs((int)roots) - 1;
        roots &= roots - 1u;
        dv[root] = 1;
        via[root] = -1;
        unsigned cur = 1u << root;
        for (int level = 0; cur; ++level) {
            unsigned seen = 0u;
            for (unsigned rc = cur; rc;) {
                const int n = __ffs((int)rc) - 1;
                rc &= rc - 1u;
                const int d = dv[n];
                fil[n] = d != 0 ? DSVG_LAYER_FILL : DSVG_LAYER_ERASE;
                dep[n] = level;
                par[n] = via[n];
                for (unsigned rn = out[n] & alive & ~seen; rn;) {
                    const int n2 = __ffs((int)rn) - 1;
                    rn &= rn - 1u;
                    seen |= 1u << n2;
                    if (rule == DSVG_FILLING_EVENODD) dv[n2] = 1 - d;
                    else dv[n2] = d + ((((cw >> n2) ^ (cw >> n)) & 1u) ? -1 : 1);
                    via[n2] = n;
                }
            }
            alive &= ~cur;
            cur = 0u;
            for (unsigned rs = seen; rs;) {
                const int n = __ffs((int)rs) - 1;
                rs &= rs - 1u;
                if ((cov[n] & alive) == 0u) cur |= 1u << n;
            }
        }
    }
    // ---- paint order: stable by (outlines and unused groups last, depth, index) ---------------------------------------------
    for (int i = 0; i < G; ++i) {
        const int ki = fil[i] == DSVG_LAYER_OUTLINE ? G + 1 : dep[i];
        int rank = 0;
        for (int j = 0; j < G; ++j) {
            const int kj = fil[j] == DSVG_LAYER_OUTLINE ? G + 1 : dep[j];
            rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        paint_order[b * G + rank] = i;
    }
}
}  // namespace

extern "C" int dsvg_overlap_counts(const void* segs, const int32_t* seg_counts, const int32_t* layer_first, int64_t B, int64_t cap,
                                   int32_t G, int32_t samples, int32_t evenodd, int32_t* area, int32_t* inter, void* stream) {
    DSVG_CHECK_ARG(segs && seg_counts && layer_first && area && inter, "overlap_counts: null pointer");
    DSVG_CHECK_ARG(G >= 1 && G <= PF_MAX_GROUPS, "overlap_counts: G = %d groups per icon, need 1..%d", G, PF_MAX_GROUPS);
    DSVG_CHECK_ARG(samples >= PF_MIN_SAMPLES && samples <= PF_MAX_SAMPLES, "overlap_counts: samples = %d per side, need %d..%d",
                   samples, PF_MIN_SAMPLES, PF_MAX_SAMPLES);
    const int64_t tiles = (samples + RS_TILE - 1) / RS_TILE;
    DSVG_CHECK_ARG(B > 0 && cap > 0 && cap < (1ll << 26) && B * tiles * tiles < (1ll << 31),
                   "overlap_counts: bad shape (B=%lld cap=%lld: %lld workgroups; chords per icon below 2^26, workgroups below 2^31)",
                   (long long)B, (long long)cap, (long long)(B * tiles * tiles));
    hipLaunchKernelGGL(overlap_counts_kernel, dim3((unsigned)(B * tiles * tiles)), dim3(RS_THREADS), 0, (hipStream_t)stream,
                       (const float*)segs, seg_counts, layer_first, (long long)cap, G, samples, (int)tiles,
                       256.f / (float)samples, evenodd ? 1 : 0, area, inter);
    DSVG_LAUNCH_CHECK("overlap_counts");
    return 0;
}

extern "C" int dsvg_filling_from_counts(int32_t itype, const int32_t* area, const int32_t* inter, const void* commands,
                                        const void* args, const uint8_t* participating, int64_t N, int32_t G, int32_t S,
                                        double threshold, int32_t rule, int64_t* filling, int32_t* depth, int32_t* parent,
                                        uint8_t* clockwise, int64_t* paint_order, void* stream) {
    DSVG_CHECK_ARG(area && inter && commands && args && participating && filling && depth && parent && clockwise && paint_order,
                   "filling_from_counts: null pointer");
    DSVG_CHECK_ARG(itype == DSVG_F32 || itype == DSVG_I64, "filling_from_counts: itype %d is neither DSVG_F32 nor DSVG_I64", itype);
    DSVG_CHECK_ARG(G >= 1 && G <= PF_MAX_GROUPS, "filling_from_counts: G = %d groups per icon, need 1..%d", G, PF_MAX_GROUPS);
    DSVG_CHECK_ARG(N > 0 && N < (1ll << 31) && S >= 1 && (int64_t)G * S <= SP_MAX_TOK,
                   "filling_from_counts: bad shape (N=%lld G=%d S=%d; G * S <= %d rows per icon)", (long long)N, G, S, SP_MAX_TOK);
    DSVG_CHECK_ARG(threshold > 0.0 && threshold <= 1.0, "filling_from_counts: threshold = %g, need 0 < threshold <= 1", threshold);
    DSVG_CHECK_ARG(rule == DSVG_FILLING_EVENODD || rule == DSVG_FILLING_ORIENTATION, "filling_from_counts: unknown rule %d", rule);
    const dim3 grid((unsigned)((N + PF_THREADS - 1) / PF_THREADS)), block(PF_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define PF_LAUNCH(T)                                                                                                         \
    hipLaunchKernelGGL((filling_from_counts_kernel<T>), grid, block, 0, st, area, inter, (const T*)commands, (const T*)args,    \
                       participating, (long long)N, G, S, threshold, rule, (long long*)filling, depth, parent, clockwise,      \
                       (long long*)paint_order)
    if (itype == DSVG_I64) PF_LAUNCH(long long);
    else PF_LAUNCH(float);
#undef PF_LAUNCH
    DSVG_LAUNCH_CHECK("filling_from_counts");
    return 0;
}
