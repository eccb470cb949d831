// Commands split and arcs converted, for every icon of a batch in one launch: SVGPath.split and SVGPath.simplify_arcs of the
// reference (deepsvg/svglib/svg_path.py:615-630, 280-293; svg_command.py:255-270, 369-413, 458-511), which it runs on the host,
// one Python object at a time.  The definition is in include/dsvg.h; tests/paths_expand_ref.py restates it in float64 and
// tests/golden/paths/expand.npz holds the reference's own results.
//   dsvg_paths_expand   one workgroup per icon, one kernel under a mode flag.  Every input row becomes 0..k output rows: a
//                       ballot scan applies the EOS rule, one lane per live row computes its length (split) or its sweep
//                       (arcs) and from it the number of rows it becomes, a prefix sum over the counts gives every row its
//                       offset (its group's base subtracted), and every output row finds the input row it comes from by
//                       binary search in the prefix and computes its own piece.
// All geometry is float64, one IEEE operation at a time, rounded to fp32 once per written value; the last piece of a row
// carries the row's end position bit for bit.  No atomics, no workspace: bit-reproducible, and nothing is read back.
#include "dsvg_common.h"
#include "svg_seq.h"             // vocabulary, start_point, block_flag_scan (the EOS rule), block_count_sum (the offsets)
#include "../../include/dsvg.h"

// restated operation by operation in tests/paths_expand_ref.py, compared by equality: no fused multiply-add
#pragma clang fp contract(off)

namespace {
constexpr int PE_THREADS = SP_THREADS;
constexpr int PE_MAX_ROWS = SP_MAX_TOK;   // G * S input rows and G * S_out output rows of one icon
constexpr int PE_DEAD = 255;              // class of a row at or behind its group's first EOS
constexpr int PE_UNKNOWN = 7;             // a command outside the vocabulary
constexpr double PE_PI = 3.141592653589793;
constexpr double PE_D2R = PE_PI / 180.0, PE_R2D = 180.0 / PE_PI;      // np.deg2rad / np.rad2deg multiply by these

__device__ __forceinline__ bool pe_finite(double v) { return __builtin_isfinite(v); }
// np.allclose(s, e) of one coordinate: |s - e| <= atol + rtol |e|
__device__ __forceinline__ bool pe_close(double s, double e) { return fabs(s - e) <= 1e-8 + 1e-5 * fabs(e); }
__device__ __forceinline__ double pe_lerp(double a, double b, double t) { return (1.0 - t) * a + t * b; }
__device__ __forceinline__ double pe_clip1(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }      // keeps a NaN

// blossom of the cubic p0..p3: de Casteljau's three levels with u, then v, then w.  B(a, a, b), B(a, b, b), B(b, b, b) are
// the control points and the end of the sub-curve on [a, b]
__device__ __forceinline__ double pe_blossom(double p0, double p1, double p2, double p3, double u, double v, double w) {
    const double p01 = pe_lerp(p0, p1, u), p12 = pe_lerp(p1, p2, u), p23 = pe_lerp(p2, p3, u);
    const double p012 = pe_lerp(p01, p12, v), p123 = pe_lerp(p12, p23, v);
    return pe_lerp(p012, p123, w);
}

// SVGCommandBezier.length: the polyline through the 100 points at z = i / 99.  The points are the Bernstein form in float64 -
// not the fp32 power basis of svg_seq.h, which is the curve sample_points draws; this one only measures
__device__ double pe_cubic_length(double x0, double y0, double x1, double y1, double x2, double y2, double x3, double y3) {
    double len = 0.0, qx = x0, qy = y0;
    for (int i = 1; i < 100; ++i) {
        const double z = (double)i / 99.0, w = 1.0 - z;
        const double b0 = (w * w) * w, b1 = (3.0 * (w * w)) * z, b2 = (3.0 * w) * (z * z), b3 = (z * z) * z;
        const double px = ((b0 * x0 + b1 * x1) + b2 * x2) + b3 * x3;
        const double py = ((b0 * y0 + b1 * y1) + b2 * y2) + b3 * y3;
        const double dx = px - qx, dy = py - qy;
        len += sqrt(dx * dx + dy * dy);
        qx = px; qy = py;
    }
    return len;
}

// the centre parametrisation of an arc (SVGCommandArc._get_center_parametrization), include/dsvg.h has the formulas
struct PeArc {
    double cx = 0.0, cy = 0.0, rx = 0.0, ry = 0.0, cphi = 1.0, sphi = 0.0, th1 = 0.0, dth = 0.0;      // th1, dth in degrees
    int k = PE_BAD;                       // `c` rows it becomes, or one of:
    static constexpr int PE_BAD = -2;     //   an argument or the sweep is not finite
    static constexpr int PE_LINE = -1;    //   exactly one radius is 0: one `l`
    static constexpr int PE_DROP = 0;     //   both radii 0, or start and end close
};

__device__ PeArc pe_arc(float2 s, const float* __restrict__ a) {
    PeArc r;
    const double x1 = s.x, y1 = s.y, x2 = a[ARG_END], y2 = a[ARG_END + 1], phi = a[2];
    double rx = fabs((double)a[0]), ry = fabs((double)a[1]);
    if (!(pe_finite(x1) && pe_finite(y1) && pe_finite(x2) && pe_finite(y2) && pe_finite(phi) && pe_finite(rx) && pe_finite(ry) &&
          pe_finite((double)a[3]) && pe_finite((double)a[4])))
        return r;
    const bool fa = a[3] != 0.f, fs = a[4] != 0.f;
    if ((rx == 0.0 && ry == 0.0) || (pe_close(x1, x2) && pe_close(y1, y2))) { r.k = PeArc::PE_DROP; return r; }
    if (rx == 0.0 || ry == 0.0) { r.k = PeArc::PE_LINE; return r; }
    const double prad = phi * PE_D2R;
    const double cphi = cos(prad), sphi = sin(prad);
    const double hx = 0.5 * (x1 - x2), hy = 0.5 * (y1 - y2), mx = 0.5 * (x1 + x2), my = 0.5 * (y1 + y2);
    const double xp = cphi * hx + sphi * hy, yp = cphi * hy - sphi * hx;
    const double xx = xp * xp, yy = yp * yp, rx2 = rx * rx, ry2 = ry * ry;
    const double lam = xx / rx2 + yy / ry2;
    double coef;
    if (lam > 1.0) {                      // radii too small for the chord: scaled up (implementation note F.6.6), centre on the chord
        const double sl = sqrt(lam);
        rx = sl * rx; ry = sl * ry;
        coef = 0.0;
    } else {
        const double q = ((rx2 * ry2 - rx2 * yy) - ry2 * xx) / (rx2 * yy + ry2 * xx);
        coef = sqrt(q > 0.0 ? q : 0.0);
    }
    if (fa == fs) coef = -coef;
    const double ctx = coef * ((rx * yp) / ry), cty = coef * (-((ry * xp) / rx));
    r.cx = (cphi * ctx - sphi * cty) + mx;
    r.cy = (sphi * ctx + cphi * cty) + my;
    const double dx = (xp - ctx) / rx, dy = (yp - cty) / ry, ex = (-(xp + ctx)) / rx, ey = (-(yp + cty)) / ry;
    const double nd = sqrt(dx * dx + dy * dy), ne = sqrt(ex * ex + ey * ey);
    double th1 = acos(pe_clip1(dx / nd)) * PE_R2D;
    if (dy < 0.0) th1 = -th1;
    double dth = acos(pe_clip1((dx / nd) * (ex / ne) + (dy / nd) * (ey / ne))) * PE_R2D;
    if (dx * ey - dy * ex < 0.0) dth = -dth;
    if (dth < 0.0) dth = dth + 360.0;
    if (!fs && dth > 0.0) dth = dth - 360.0;
    if (lam > 1.0 && pe_finite(dth)) dth = fs ? 180.0 : -180.0;      // the chord is a diameter: half a turn, not acos(-1 + rounding)
    if (!(pe_finite(th1) && pe_finite(dth) && pe_finite(r.cx) && pe_finite(r.cy) && pe_finite(rx) && pe_finite(ry))) return r;
    r.rx = rx; r.ry = ry; r.cphi = cphi; r.sphi = sphi; r.th1 = th1; r.dth = dth;
    const double parts = floor(fabs(dth) / 45.0);      // <= 8
    r.k = parts > 1.0 ? (int)parts : 1;
    return r;
}

// piece i of the arc's k: control1, control2 and end of SVGCommandArc.to_beziers
__device__ void pe_arc_piece(const PeArc& r, int i, double* out) {
    const double inv = 1.0 / (double)r.k;
    const double t1 = (r.th1 + inv * ((double)i * r.dth)) * PE_D2R, t2 = (r.th1 + inv * ((double)(i + 1) * r.dth)) * PE_D2R;
    const double dt = t2 - t1, th = tan(0.5 * dt);
    const double alpha = (sin(dt) * (sqrt(4.0 + 3.0 * (th * th)) - 1.0)) / 3.0;
    const double c1 = cos(t1), s1 = sin(t1), c2 = cos(t2), s2 = sin(t2);
    const double u1x = r.rx * c1, u1y = r.ry * s1, u2x = r.rx * c2, u2y = r.ry * s2;              // on the axis-aligned ellipse
    const double v1x = -(r.rx * s1), v1y = r.ry * c1, v2x = -(r.rx * s2), v2y = r.ry * c2;        // its derivative
    const double p1x = r.cx + (r.cphi * u1x - r.sphi * u1y), p1y = r.cy + (r.sphi * u1x + r.cphi * u1y);
    const double p2x = r.cx + (r.cphi * u2x - r.sphi * u2y), p2y = r.cy + (r.sphi * u2x + r.cphi * u2y);
    const double d1x = r.cphi * v1x - r.sphi * v1y, d1y = r.sphi * v1x + r.cphi * v1y;
    const double d2x = r.cphi * v2x - r.sphi * v2y, d2y = r.sphi * v2x + r.cphi * v2y;
    out[0] = p1x + alpha * d1x; out[1] = p1y + alpha * d1y;
    out[2] = p2x - alpha * d2x; out[3] = p2y - alpha * d2y;
    out[4] = p2x; out[5] = p2y;
}

template <int MODE>
__global__ __launch_bounds__(PE_THREADS) void paths_expand_kernel(
    const float* __restrict__ commands, const float* __restrict__ args, int G, int S, int S_out, int n_pieces, double max_dist,
    int include_lines, float* __restrict__ out_cmd, float* __restrict__ out_args, int32_t* __restrict__ len_groups,
    int32_t* __restrict__ source_row, float* __restrict__ lengths, uint8_t* __restrict__ valid) {
    __shared__ unsigned char cls[PE_MAX_ROWS];      // command of a live row, PE_DEAD at or behind the group's first EOS
    __shared__ int pre[PE_MAX_ROWS + 1];            // scan 1: EOS rows before t; then: output rows of the rows before t
    __shared__ int wtot[PE_MAX_ROWS / 64];
    __shared__ int s_bad;

    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int R = G * S;
    const float* cmd = commands + b * R;
    const float* arg = args + b * R * N_ARGS;

    for (int t = tid; t < R; t += PE_THREADS) {
        const float c = cmd[t];
        cls[t] = (unsigned char)((c >= 0.f && c < (float)N_CMD) ? (int)c : PE_UNKNOWN);      // a NaN is never converted
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();

    // ---- a group ends at its first EOS ---------------------------------------------------------------------------------
    block_flag_scan<PE_MAX_ROWS>(R, pre, wtot, [&](int t) { return t < R && cls[t] == CMD_EOS; });
    for (int t = tid; t < R; t += PE_THREADS)
        if (pre[t + 1] != pre[(t / S) * S]) cls[t] = PE_DEAD;
    __syncthreads();

    // ---- one lane per live row: the rows it becomes ------------------------------------------------------------------
    block_count_sum<PE_MAX_ROWS>(R, pre, wtot, [&](int t) {
        if (t >= R) return 0;
        const int c = cls[t];
        float len32 = 0.f;
        int k = 0;
        if (c != PE_DEAD && t % S != 0) {         // row 0 is the frame
            const float* a = arg + (long long)t * N_ARGS;
            const float2 s = start_point(a, t % S);
            k = 1;
            if (c == PE_UNKNOWN) s_bad = 1;
            else if (c == CMD_L || c == CMD_C) {
                const double x0 = s.x, y0 = s.y, x3 = a[ARG_END], y3 = a[ARG_END + 1];
                bool fin = pe_finite(x0) && pe_finite(y0) && pe_finite(x3) && pe_finite(y3);
                if (c == CMD_C)
                    fin = fin && pe_finite((double)a[ARG_CONTROL1]) && pe_finite((double)a[ARG_CONTROL1 + 1]) &&
                          pe_finite((double)a[ARG_CONTROL2]) && pe_finite((double)a[ARG_CONTROL2 + 1]);
                if (!fin) s_bad = 1;
                else if (MODE == DSVG_EXPAND_SPLIT) {
                    double len;
                    if (c == CMD_L) {
                        const double dx = x3 - x0, dy = y3 - y0;
                        len = sqrt(dx * dx + dy * dy);
                    } else
                        len = pe_cubic_length(x0, y0, a[ARG_CONTROL1], a[ARG_CONTROL1 + 1], a[ARG_CONTROL2], a[ARG_CONTROL2 + 1],
                                              x3, y3);
                    if (!pe_finite(len)) s_bad = 1;
                    else {
                        len32 = (float)len;
                        if (c == CMD_C || include_lines) {
                            if (n_pieces > 0) k = min(n_pieces, S_out);
                            else {
                                const double q = ceil(len / max_dist);      // finite or +inf: len is finite, max_dist > 0
                                k = q >= (double)S_out ? S_out : (q > 1.0 ? (int)q : 1);
                            }
                        }
                    }
                }
            } else if (c == CMD_A) {
                if (MODE == DSVG_EXPAND_SPLIT) s_bad = 1;
                else {
                    const PeArc r = pe_arc(s, a);
                    if (r.k == PeArc::PE_BAD) s_bad = 1;
                    else k = r.k == PeArc::PE_LINE ? 1 : r.k;
                }
            }
        }
        if (MODE == DSVG_EXPAND_SPLIT) lengths[b * R + t] = len32;
        return k;
    });
    for (int g = tid; g < G; g += PE_THREADS)
        if (pre[(g + 1) * S] - pre[g * S] > S_out - 2) s_bad = 1;
    __syncthreads();
    const bool ok = !s_bad;

    if (tid == 0) valid[b] = ok ? 1 : 0;
    for (int g = tid; g < G; g += PE_THREADS) len_groups[b * G + g] = ok ? pre[(g + 1) * S] - pre[g * S] : 0;

    // ---- rows out: every output row finds its input row and computes its own piece ------------------------------------
    const int rows_out = G * S_out;
    float* oc = out_cmd + b * rows_out;
    float* oa = out_args + b * rows_out * N_ARGS;
    int32_t* os = source_row + b * rows_out;
    for (int r = tid; r < rows_out; r += PE_THREADS) {
        const int g = r / S_out, pos = r % S_out;
        float v[N_ARGS];
#pragma unroll
        for (int q = 0; q < N_ARGS; ++q) v[q] = -1.f;
        int c_out = pos == 0 ? CMD_SOS : CMD_EOS, src = -1;
        const int base = pre[g * S];
        if (ok && pos > 0 && pos - 1 < pre[(g + 1) * S] - base) {
            const int target = base + pos - 1;
            int lo = g * S, hi = (g + 1) * S - 1;     // the last row of the group with pre[t] <= target: it has pre[t + 1] > target
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= target) lo = mid; else hi = mid - 1;
            }
            const int t = lo, i = target - pre[t], k = pre[t + 1] - pre[t];
            const float* a = arg + (long long)t * N_ARGS;
            const int c = cls[t];
            src = t - g * S;
            c_out = c;
            if (c == CMD_A && MODE == DSVG_EXPAND_ARCS) {
                const float2 s = start_point(a, t % S);
                const PeArc arc = pe_arc(s, a);       // the same arithmetic as in the count: the same k
                if (arc.k == PeArc::PE_LINE) c_out = CMD_L;
                else {
                    c_out = CMD_C;
                    double p[6];
                    pe_arc_piece(arc, i, p);
#pragma unroll
                    for (int q = 0; q < 6; ++q) v[ARG_CONTROL1 + q] = (float)p[q];
                }
                if (i == k - 1) { v[ARG_END] = a[ARG_END]; v[ARG_END + 1] = a[ARG_END + 1]; }
            } else if (k > 1 && c == CMD_L) {
                const float2 s = start_point(a, t % S);
                const double al = (double)(i + 1) / (double)k;
                v[ARG_END] = i == k - 1 ? a[ARG_END] : (float)pe_lerp((double)s.x, (double)a[ARG_END], al);
                v[ARG_END + 1] = i == k - 1 ? a[ARG_END + 1] : (float)pe_lerp((double)s.y, (double)a[ARG_END + 1], al);
            } else if (k > 1 && c == CMD_C) {
                const float2 s = start_point(a, t % S);
                const double za = (double)i / (double)k, zb = (double)(i + 1) / (double)k;
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const double p0 = d ? s.y : s.x, p1 = a[ARG_CONTROL1 + d], p2 = a[ARG_CONTROL2 + d], p3 = a[ARG_END + d];
                    v[ARG_CONTROL1 + d] = (float)pe_blossom(p0, p1, p2, p3, za, za, zb);
                    v[ARG_CONTROL2 + d] = (float)pe_blossom(p0, p1, p2, p3, za, zb, zb);
                    v[ARG_END + d] = i == k - 1 ? a[ARG_END + d] : (float)pe_blossom(p0, p1, p2, p3, zb, zb, zb);
                }
            } else {                                  // one row, copied: the slots its command enables
                const int first = c == CMD_C ? ARG_CONTROL1 : ((c == CMD_M || c == CMD_L) ? ARG_END : N_ARGS);
#pragma unroll
                for (int q = ARG_CONTROL1; q < N_ARGS; ++q)
                    if (q >= first) v[q] = a[q];
            }
        }
        oc[r] = (float)c_out;
        os[r] = src;
#pragma unroll
        for (int q = 0; q < N_ARGS; ++q) oa[(long long)r * N_ARGS + q] = v[q];
    }
}
}  // namespace

extern "C" int dsvg_paths_expand(int32_t mode, const float* commands, const float* args, int64_t N, int32_t G, int32_t S,
                                 int32_t S_out, int32_t n, double max_dist, int32_t include_lines, float* out_commands,
                                 float* out_args, int32_t* len_groups, int32_t* source_row, float* lengths, uint8_t* valid,
                                 void* stream) {
    DSVG_CHECK_ARG(mode == DSVG_EXPAND_SPLIT || mode == DSVG_EXPAND_ARCS, "paths_expand: unknown mode %d", mode);
    DSVG_CHECK_ARG(commands && args && out_commands && out_args && len_groups && source_row && valid,
                   "paths_expand: null pointer");
    DSVG_CHECK_ARG(N > 0 && N < (1ll << 31) && G >= 1 && S >= 1 && (int64_t)G * S <= PE_MAX_ROWS,
                   "paths_expand: bad shape (N=%lld G=%d S=%d; G * S <= %d rows per icon)", (long long)N, G, S, PE_MAX_ROWS);
    DSVG_CHECK_ARG(S_out >= 2 && (int64_t)G * S_out <= PE_MAX_ROWS,
                   "paths_expand: bad output shape (G=%d S_out=%d; S_out >= 2, G * S_out <= %d rows per icon)", G, S_out,
                   PE_MAX_ROWS);
    hipStream_t st = (hipStream_t)stream;
    if (mode == DSVG_EXPAND_SPLIT) {
        DSVG_CHECK_ARG(lengths, "paths_expand: split needs lengths");
        const bool by_dist = max_dist > 0.0 && max_dist <= 1.7976931348623157e308;      // finite: false for a NaN too
        DSVG_CHECK_ARG((n >= 1 && max_dist == 0.0) || (n == 0 && by_dist),
                       "paths_expand: split takes n >= 1 with max_dist = 0, or n = 0 with a finite max_dist > 0 (n=%d max_dist=%g)",
                       n, max_dist);
        hipLaunchKernelGGL((paths_expand_kernel<DSVG_EXPAND_SPLIT>), dim3((unsigned)N), dim3(PE_THREADS), 0, st, commands, args, G,
                           S, S_out, n, max_dist, include_lines ? 1 : 0, out_commands, out_args, len_groups, source_row, lengths,
                           valid);
    } else {
        hipLaunchKernelGGL((paths_expand_kernel<DSVG_EXPAND_ARCS>), dim3((unsigned)N), dim3(PE_THREADS), 0, st, commands, args, G,
                           S, S_out, 0, 0.0, 0, out_commands, out_args, len_groups, source_row, (float*)nullptr, valid);
    }
    DSVG_LAUNCH_CHECK("paths_expand");
    return 0;
}
