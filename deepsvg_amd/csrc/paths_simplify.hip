// Beziers fitted through the points of every sub-path, for every icon of a batch in one launch: SVGPath.simplify of the
// reference (deepsvg/svglib/svg_path.py:391-613) - Schneider's curve fit with Newton reparametrisation on the smooth
// stretches, Ramer-Douglas-Peucker on the rest - which it runs on the host in pure Python, one Point object at a time.  The
// definition is in include/dsvg.h; tests/paths_simplify_ref.py restates it in float64 and tests/golden/paths/simplify.npz
// holds the reference's own results.
//   dsvg_paths_simplify   one workgroup of 256 threads per icon, three phases:
//     scan   one lane per row: the EOS rule, the class of every row, the chord to the row before it, the segment breaks.
//            From these every row knows the jobs it owns - the fit of the segment it starts, the RDP of the gap of lines it
//            starts, a zero-length line for an empty gap before or behind it - and a prefix sum gives every job a range of
//            slots, one per interval it covers: a job never emits more rows than that.
//     fit    every wave takes the owner rows of its 64-row chunks and runs the job's recursion depth-first, left child
//            first, so rows come out in path order.  Pending right children are adjacent intervals, so the stack is a
//            chain of split indices (nxt[]), and tangents are recomputed from indices: nothing else is kept.  The 64 lanes
//            evaluate points i = lane, lane + 64, ...; sums are 64 strided partials combined by halving, as the definition
//            states, and every lane reads only the u it wrote.
//     pack   a flag scan over the slots in use compacts them into the output, and decides validity.
// Points (fp32 as read, divided by `unit` in float64 at every use), the chord table and u live in LDS; the rows a job emits
// wait in a workspace in global memory (20 bytes per slot).  All geometry is float64, one IEEE operation at a time; end
// positions are copies.  No atomics: bit-reproducible.
#include "dsvg_common.h"
#include "svg_seq.h"             // vocabulary, block_flag_scan (the EOS rule, the slots in use), block_count_sum (the slots)
#include "../../include/dsvg.h"

// restated operation by operation in tests/paths_simplify_ref.py, compared by equality: no fused multiply-add
#pragma clang fp contract(off)

namespace {
constexpr int PS_THREADS = SP_THREADS;
constexpr int PS_MAX_ROWS = SP_MAX_TOK;           // G * S input rows and G * S_out output rows of one icon
constexpr int PS_MAX_SLOTS = 2 * PS_MAX_ROWS;     // a run of n rows behind its `m` takes at most 2 n + 1 slots, the `m` one
// the byte of a row: its class in the low bits ...
constexpr int PS_CLASS = 15, PS_UNKNOWN = 7, PS_FRAME = 14, PS_DEAD = 15;
// ... and the jobs it owns
constexpr int PS_SEG = 16;                        // starts a segment (force_smooth: a run): one fit
constexpr int PS_GAP_BEFORE = 32;                 // an empty gap before its segment: a zero-length `l` at its start point
constexpr int PS_GAP_AFTER = 64;                  // a `c` that ends its run: a zero-length `l` at its end
constexpr int PS_LGAP = 128;                      // starts a gap of `l` rows: one RDP
constexpr int PS_ROW_PASS = 0, PS_ROW_LINE = 1, PS_ROW_CUBIC = 2;      // what a slot holds: kind << 16 | source row; -1: not in use
constexpr double PS_EPS = 1e-12, PS_MACHINE_EPS = 1.12e-16;

__device__ __forceinline__ bool ps_finite(double v) { return __builtin_isfinite(v); }
__device__ __forceinline__ bool ps_close(double s, double e) { return fabs(s - e) <= 1e-8 + 1e-5 * fabs(e); }
__device__ __forceinline__ bool ps_is_lc(int f) { return (f & PS_CLASS) == CMD_L || (f & PS_CLASS) == CMD_C; }
__device__ __forceinline__ double ps_norm(double dx, double dy) { return sqrt(dx * dx + dy * dy); }

__device__ __forceinline__ double ps_bezier(double p0, double c1, double c2, double p3, double t) {
    const double w = 1.0 - t;
    const double b0 = (w * w) * w, b1 = (3.0 * (w * w)) * t, b2 = (3.0 * w) * (t * t), b3 = (t * t) * t;
    return ((b0 * p0 + b1 * c1) + b2 * c2) + b3 * p3;
}
__device__ __forceinline__ double ps_d1(double p0, double c1, double c2, double p3, double t) {
    const double w = 1.0 - t;
    return ((3.0 * (w * w)) * (c1 - p0) + ((6.0 * w) * t) * (c2 - c1)) + (3.0 * (t * t)) * (p3 - c2);
}
__device__ __forceinline__ double ps_d2(double p0, double c1, double c2, double p3, double t) {
    const double w = 1.0 - t;
    return (6.0 * w) * ((c2 - 2.0 * c1) + p0) + (6.0 * t) * ((p3 - 2.0 * c2) + c1);
}

// partial[j] += partial[j + d] for j < d, d = 32 .. 1, every lane holding one partial; all lanes return partial[0]
__device__ __forceinline__ double ps_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d, 64);
    return __shfl(v, 0, 64);
}
// the largest value over the wave, the largest index among equal values (the reference's `>=` in ascending order)
__device__ __forceinline__ void ps_wave_argmax(double& val, int& idx) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(val, d, 64);
        const int oi = __shfl_xor(idx, d, 64);
        if (ov > val || (ov == val && oi > idx)) { val = ov; idx = oi; }
    }
}

// what a wave needs to run a job; a point index is the row (of the icon) whose end position it is
struct PsWave {
    const float2* pts;
    const double* Lc;
    double* u;
    unsigned short* nxt;
    float4* ctrl;          // the icon's slots
    int* meta;
    int* bad;
    double unit, tol, eps;
    int lane;

    __device__ __forceinline__ double px(int i) const { return (double)pts[i].x / unit; }
    __device__ __forceinline__ double py(int i) const { return (double)pts[i].y / unit; }

    // normalize(P[a] - P[b]); false at distance 0
    __device__ __forceinline__ bool direction(int a, int b, double& ox, double& oy) const {
        const double vx = px(a) - px(b), vy = py(a) - py(b);
        const double n = ps_norm(vx, vy);
        if (n == 0.0) return false;
        ox = vx / n; oy = vy / n;
        return true;
    }

    __device__ __forceinline__ void emit(int slot, int kind, int src, double c1x = 0.0, double c1y = 0.0, double c2x = 0.0,
                                         double c2y = 0.0) const {
        if (lane == 0) {
            if (kind == PS_ROW_CUBIC)
                ctrl[slot] = make_float4((float)(c1x * unit), (float)(c1y * unit), (float)(c2x * unit), (float)(c2y * unit));
            meta[slot] = (kind << 16) | src;
        }
    }

    // Ramer-Douglas-Peucker on the points jf..jl into slots slot0..; at most jl - jf rows
    __device__ void rdp(int jf, int jl, int slot0) const {
        int first = jf, last = jl, emitted = 0;
        for (;;) {
            const double ax = px(first), ay = py(first), bx = px(last), by = py(last);
            const bool same = ps_close(ax, bx) && ps_close(ay, by);
            const double dx = bx - ax, dy = by - ay;
            const double len = ps_norm(dx, dy);
            double best = 0.0;
            int idx = -1;
            for (int i = first + 1 + lane; i < last; i += 64) {
                const double qx = px(i), qy = py(i);
                const double d = same ? ps_norm(qx - ax, qy - ay) : fabs(dx * (ay - qy) - dy * (ax - qx)) / len;
                if (d >= best) { best = d; idx = i; }
            }
            ps_wave_argmax(best, idx);
            if (best > eps && idx > first && idx < last) {
                nxt[idx] = (unsigned short)last;      // every lane writes the same value and reads its own
                last = idx;
            } else {
                if (emitted < jl - jf) emit(slot0 + emitted, PS_ROW_LINE, last);
                ++emitted;
                if (last == jl) return;
                first = last;
                last = nxt[last];
            }
        }
    }

    // fitCubic on the points jf..jl into slots slot0..; at most jl - jf rows
    __device__ void fit(int jf, int jl, int slot0) const {
        int first = jf, last = jl, emitted = 0;
        for (;;) {
            const int n = last - first;
            double t1x, t1y, t2x, t2y;
            bool ok;
            if (first == jf) ok = direction(first + 1, first, t1x, t1y);
            else {
                ok = direction(first - 1, first + 1, t1x, t1y);
                t1x = -t1x; t1y = -t1y;
            }
            ok = (last == jl ? direction(last - 1, last, t2x, t2y) : direction(last - 1, last + 1, t2x, t2y)) && ok;
            if (!ok) { *bad = 1; return; }
            const double p1x = px(first), p1y = py(first), p2x = px(last), p2y = py(last);
            double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
            bool leaf = false;
            int split = -1;
            if (n == 1) {
                const double d = ps_norm(p1x - p2x, p1y - p2y) / 3.0;
                c1x = p1x + d * t1x; c1y = p1y + d * t1y; c2x = p2x + d * t2x; c2y = p2y + d * t2y;
                leaf = true;
            } else {
                const double total = Lc[last] - Lc[first];
                if (total == 0.0) { *bad = 1; return; }
                // u of the interior points in LDS, of the two ends in the registers of the lanes that own them
                double u_first = 0.0, u_last = 0.0;
                auto get_u = [&](int i) { return i == 0 ? u_first : (i == n ? u_last : u[first + i]); };
                auto set_u = [&](int i, double v) {
                    if (i == 0) u_first = v; else if (i == n) u_last = v; else u[first + i] = v;
                };
                for (int i = lane; i <= n; i += 64) set_u(i, (Lc[first + i] - Lc[first]) / total);
                double limit = tol * tol > tol ? tol * tol : tol;
                bool ordered = true;
                for (int it = 0; it < 5; ++it) {
                    // ---- generateBezier
                    double s00 = 0.0, s01 = 0.0, s11 = 0.0, sx0 = 0.0, sx1 = 0.0;
                    for (int i = lane; i <= n; i += 64) {
                        const double ui = get_u(i);
                        const double t = 1.0 - ui;
                        const double b = (3.0 * ui) * t;
                        const double b0 = (t * t) * t, b1 = b * t, b2 = b * ui, b3 = (ui * ui) * ui;
                        const double a1x = t1x * b1, a1y = t1y * b1, a2x = t2x * b2, a2y = t2y * b2;
                        const double tx = (px(first + i) - p1x * (b0 + b1)) - p2x * (b2 + b3);
                        const double ty = (py(first + i) - p1y * (b0 + b1)) - p2y * (b2 + b3);
                        s00 = s00 + (a1x * a1x + a1y * a1y);
                        s01 = s01 + (a1x * a2x + a1y * a2y);
                        s11 = s11 + (a2x * a2x + a2y * a2y);
                        sx0 = sx0 + (a1x * tx + a1y * ty);
                        sx1 = sx1 + (a2x * tx + a2y * ty);
                    }
                    const double c00 = ps_wave_sum(s00), c01 = ps_wave_sum(s01), c11 = ps_wave_sum(s11);
                    const double x0 = ps_wave_sum(sx0), x1 = ps_wave_sum(sx1);
                    const double det = c00 * c11 - c01 * c01;
                    double al1, al2;
                    if (fabs(det) > PS_EPS) {
                        const double det_c0x = c00 * x1 - c01 * x0;
                        const double det_xc1 = x0 * c11 - x1 * c01;
                        al1 = det_xc1 / det; al2 = det_c0x / det;
                    } else {
                        const double s0 = c00 + c01, s1 = c01 + c11;
                        al1 = al2 = fabs(s0) > PS_EPS ? x0 / s0 : (fabs(s1) > PS_EPS ? x1 / s1 : 0.0);
                    }
                    const double seg = ps_norm(p2x - p1x, p2y - p1y);
                    const double cut = PS_EPS * seg;
                    if (al1 < cut || al2 < cut) al1 = al2 = seg / 3.0;
                    else {
                        const double lx = p2x - p1x, ly = p2y - p1y;
                        const double h1x = t1x * al1, h1y = t1y * al1, h2x = t2x * al2, h2y = t2y * al2;
                        if ((h1x * lx + h1y * ly) - (h2x * lx + h2y * ly) > seg * seg) al1 = al2 = seg / 3.0;
                    }
                    c1x = p1x + t1x * al1; c1y = p1y + t1y * al1; c2x = p2x + t2x * al2; c2y = p2y + t2y * al2;
                    // ---- computeMaxError
                    double err = 0.0;
                    int idx = -1;
                    for (int i = lane ? lane : 64; i < n; i += 64) {
                        const double ui = get_u(i);
                        const double qx = ps_bezier(p1x, c1x, c2x, p2x, ui), qy = ps_bezier(p1y, c1y, c2y, p2y, ui);
                        double d = ps_norm(qx - px(first + i), qy - py(first + i));
                        d = d * d;
                        if (d >= err) { err = d; idx = first + i; }
                    }
                    ps_wave_argmax(err, idx);
                    if (idx <= first || idx >= last) { *bad = 1; return; }      // every distance is a NaN
                    split = idx;
                    if (err < tol && ordered) { leaf = true; break; }
                    if (err >= limit) break;
                    // ---- reparametrize: one Newton step per point, then are the u still ascending
                    for (int i = lane; i <= n; i += 64) {
                        const double t = get_u(i);
                        const double qx = px(first + i), qy = py(first + i);
                        const double fx = ps_bezier(p1x, c1x, c2x, p2x, t) - qx, fy = ps_bezier(p1y, c1y, c2y, p2y, t) - qy;
                        const double ax = ps_d1(p1x, c1x, c2x, p2x, t), ay = ps_d1(p1y, c1y, c2y, p2y, t);
                        const double bx = ps_d2(p1x, c1x, c2x, p2x, t), by = ps_d2(p1y, c1y, c2y, p2y, t);
                        const double num = fx * ax + fy * ay;
                        const double den = (ax * ax + ay * ay) + (fx * bx + fy * by);
                        if (!(den >= -PS_MACHINE_EPS && den <= PS_MACHINE_EPS)) set_u(i, t - num / den);
                    }
                    bool unordered = false;
                    double carry = 0.0;
                    for (int base = 0; base <= n; base += 64) {
                        const int i = base + lane;
                        const double v = i <= n ? get_u(i) : 0.0;
                        double prev = __shfl_up(v, 1, 64);
                        if (lane == 0) prev = carry;
                        carry = __shfl(v, 63, 64);
                        if (i >= 1 && i <= n && v <= prev) unordered = true;
                    }
                    ordered = !__any(unordered);
                    limit = err;
                }
            }
            if (leaf) {
                if (emitted < jl - jf) emit(slot0 + emitted, PS_ROW_CUBIC, last, c1x, c1y, c2x, c2y);
                ++emitted;
                if (last == jl) return;
                first = last;
                last = nxt[last];
            } else {
                nxt[split] = (unsigned short)last;
                last = split;
            }
        }
    }
};

__global__ __launch_bounds__(PS_THREADS) void paths_simplify_kernel(
    const float* __restrict__ commands, const float* __restrict__ args, int G, int S, int S_out, double tolerance,
    double epsilon, double cos_threshold, int force_smooth, double unit, float4* __restrict__ ws_ctrl, int* __restrict__ ws_meta,
    float* __restrict__ out_cmd, float* __restrict__ out_args, int32_t* __restrict__ len_groups,
    int32_t* __restrict__ source_row, uint8_t* __restrict__ valid) {
    __shared__ float2 pts[PS_MAX_ROWS];             // end position of every row, as read
    __shared__ double Lc[PS_MAX_ROWS];              // chord to the row before; then the chord table of every run; then gslot
    __shared__ double us[PS_MAX_ROWS];              // u of the interior points of the fit in progress
    __shared__ int pre_raw[PS_MAX_ROWS + 2];        // int: EOS rows before t, then slots before row t; 16 bit: slots in use before s
    __shared__ unsigned short nxt[PS_MAX_ROWS];     // the pending right children of a job: the end of the interval that starts here
    __shared__ unsigned char cls[PS_MAX_ROWS];
    __shared__ int wtot[PS_MAX_SLOTS / 64];
    __shared__ int s_bad;

    const long long b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = G * S;
    const float* cmd = commands + b * R;
    const float* arg = args + b * R * N_ARGS;
    float4* ctrl = ws_ctrl + b * 2 * R;
    int* meta = ws_meta + b * 2 * R;
    int* pre = pre_raw;

    for (int t = tid; t < R; t += PS_THREADS) {
        const float c = cmd[t];
        cls[t] = (unsigned char)((c >= 0.f && c < (float)N_CMD) ? (int)c : PS_UNKNOWN);      // a NaN is never converted
        pts[t] = make_float2(arg[(long long)t * N_ARGS + ARG_END], arg[(long long)t * N_ARGS + ARG_END + 1]);
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();

    // ---- a group ends at its first EOS; row 0 is its frame -------------------------------------------------------------
    block_flag_scan<PS_MAX_ROWS>(R, pre, wtot, [&](int t) { return t < R && cls[t] == CMD_EOS; });
    for (int t = tid; t < R; t += PS_THREADS) {
        if (pre[t + 1] != pre[(t / S) * S]) cls[t] = PS_DEAD;
        else if (t % S == 0) cls[t] = PS_FRAME;
    }
    __syncthreads();

    // ---- one lane per row: its chord, the segment break before it, the jobs it owns ------------------------------------
    int flags[PS_MAX_ROWS / PS_THREADS];
#pragma unroll
    for (int k = 0; k < PS_MAX_ROWS / PS_THREADS; ++k) {
        const int t = k * PS_THREADS + tid;
        flags[k] = 0;
        if (t >= R) continue;
        const int c = cls[t];
        if (c == PS_UNKNOWN || c == CMD_A) s_bad = 1;
        if (c != CMD_L && c != CMD_C) continue;
        const float* a = arg + (long long)t * N_ARGS;
        const int cp = cls[t - 1];                                                     // t - 1 is in the group: row 0 is its frame
        const int cn = (t + 1) % S ? cls[t + 1] : PS_DEAD;
        const double x0 = (double)pts[t - 1].x / unit, y0 = (double)pts[t - 1].y / unit;
        const double x3 = (double)pts[t].x / unit, y3 = (double)pts[t].y / unit;
        bool fin = ps_finite(x0) && ps_finite(y0) && ps_finite(x3) && ps_finite(y3);
        if (c == CMD_C)
            fin = fin && ps_finite((double)a[ARG_CONTROL1]) && ps_finite((double)a[ARG_CONTROL1 + 1]) &&
                  ps_finite((double)a[ARG_CONTROL2]) && ps_finite((double)a[ARG_CONTROL2 + 1]);
        if (!fin) s_bad = 1;
        Lc[t] = ps_norm(x3 - x0, y3 - y0);
        if (force_smooth) {
            if (!ps_is_lc(cp)) flags[k] = PS_SEG;
        } else if (c == CMD_L) {
            if (cp != CMD_L) flags[k] = PS_LGAP;
        } else {
            bool brk = cp != CMD_C;
            if (!brk) {
                const float* ap = a - N_ARGS;
                const double t1x = 3.0 * (x0 - (double)ap[ARG_CONTROL2] / unit), t1y = 3.0 * (y0 - (double)ap[ARG_CONTROL2 + 1] / unit);
                const double t2x = -(3.0 * ((double)a[ARG_CONTROL1] / unit - x0)), t2y = -(3.0 * ((double)a[ARG_CONTROL1 + 1] / unit - y0));
                const double n1 = ps_norm(t1x, t1y), n2 = ps_norm(t2x, t2y);
                if (n1 <= 1e-8 || n2 <= 1e-8) brk = true;
                else {
                    double cs = (t1x / n1) * (t2x / n2) + (t1y / n1) * (t2y / n2);
                    cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
                    brk = cs > cos_threshold;
                }
            }
            if (brk) flags[k] = PS_SEG | (cp != CMD_L ? PS_GAP_BEFORE : 0);
            if (!ps_is_lc(cn)) flags[k] |= PS_GAP_AFTER;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PS_MAX_ROWS / PS_THREADS; ++k) {
        const int t = k * PS_THREADS + tid;
        if (t < R && flags[k]) cls[t] |= flags[k];
    }
    __syncthreads();
    const bool scan_ok = !s_bad;

    // the chord table: once per run, in ascending order, by the lane of the run's first row
    if (scan_ok)
        for (int t = tid; t < R; t += PS_THREADS) {
            if (!ps_is_lc(cls[t]) || ps_is_lc(cls[t - 1])) continue;
            const int gend = (t / S + 1) * S;
            double acc = 0.0;
            Lc[t - 1] = 0.0;
            for (int q = t; q < gend && ps_is_lc(cls[q]); ++q) {
                acc = acc + Lc[q];
                Lc[q] = acc;
            }
        }

    // ---- the slots: one per interval of a job, one per empty gap, one per row that passes through ----------------------
    block_count_sum<PS_MAX_ROWS>(R, pre, wtot, [&](int t) {
        if (t >= R) return 0;
        const int f = cls[t], c = f & PS_CLASS;
        if (c == PS_DEAD || c == PS_FRAME) return 0;
        return 1 + ((f & PS_GAP_BEFORE) ? 1 : 0) + ((f & PS_GAP_AFTER) ? 1 : 0);
    });
    const int n_slots = pre[R];
    if (scan_ok) {
        for (int s = tid; s < n_slots; s += PS_THREADS) meta[s] = -1;
        __syncthreads();
        for (int t = tid; t < R; t += PS_THREADS) {
            const int f = cls[t], c = f & PS_CLASS;
            if (c == PS_DEAD || c == PS_FRAME) continue;
            if (!ps_is_lc(f)) meta[pre[t]] = (PS_ROW_PASS << 16) | t;
            if (f & PS_GAP_BEFORE) meta[pre[t]] = (PS_ROW_LINE << 16) | (t - 1);
            if (f & PS_GAP_AFTER) meta[pre[t + 1] - 1] = (PS_ROW_LINE << 16) | t;
        }

        // ---- the jobs: every wave takes the owner rows of its chunks ---------------------------------------------------
        PsWave w{pts, Lc, us, nxt, ctrl, meta, &s_bad, unit, tolerance, epsilon, lane};
        for (int base = wave * 64; base < R; base += PS_THREADS) {
            const int f0 = base + lane < R ? cls[base + lane] : PS_DEAD;
            unsigned long long owners = __ballot((f0 & (PS_SEG | PS_LGAP)) != 0);
            while (owners) {
                const int t0 = base + __ffsll((long long)owners) - 1;
                owners &= owners - 1;
                const int f = cls[t0];
                const int gend = (t0 / S + 1) * S;
                int e = t0;                       // the last row of the job: rows behind t0 that continue it, 64 at a time
                for (;;) {
                    const int q = e + 1 + lane;
                    bool cont = false;
                    if (q < gend) {
                        const int fq = cls[q];
                        cont = (f & PS_LGAP) ? (fq & PS_CLASS) == CMD_L
                                             : (force_smooth ? ps_is_lc(fq) : ((fq & PS_CLASS) == CMD_C && !(fq & PS_SEG)));
                    }
                    const unsigned long long m = __ballot(cont);
                    if (m == ~0ull) { e += 64; continue; }
                    e += __ffsll((long long)~m) - 1;
                    break;
                }
                if (f & PS_LGAP) w.rdp(t0 - 1, e, pre[t0]);
                else w.fit(t0 - 1, e, pre[t0] + ((f & PS_GAP_BEFORE) ? 1 : 0));
            }
        }
    }
    __syncthreads();

    // ---- pack: the slots in use, compacted ------------------------------------------------------------------------------
    int* gslot = reinterpret_cast<int*>(Lc);        // slots before group g; the chord table is done with
    for (int g = tid; g <= G; g += PS_THREADS) gslot[g] = pre[g * S];
    __syncthreads();
    unsigned short* used = reinterpret_cast<unsigned short*>(pre_raw);
    const bool fit_ok = !s_bad;
    block_flag_scan<PS_MAX_SLOTS>(n_slots > 0 ? n_slots : 1, used, wtot,
                                  [&](int s) { return fit_ok && s < n_slots && meta[s] != -1; });
    for (int g = tid; g < G; g += PS_THREADS)
        if ((int)used[gslot[g + 1]] - (int)used[gslot[g]] > S_out - 2) s_bad = 1;
    __syncthreads();
    const bool ok = !s_bad;

    if (tid == 0) valid[b] = ok ? 1 : 0;
    for (int g = tid; g < G; g += PS_THREADS) len_groups[b * G + g] = ok ? (int)used[gslot[g + 1]] - (int)used[gslot[g]] : 0;

    const int rows_out = G * S_out;
    float* oc = out_cmd + b * rows_out;
    float* oa = out_args + b * rows_out * N_ARGS;
    int32_t* os = source_row + b * rows_out;
    for (int r = tid; r < rows_out; r += PS_THREADS) {
        const int g = r / S_out, pos = r % S_out;
        float v[N_ARGS];
#pragma unroll
        for (int q = 0; q < N_ARGS; ++q) v[q] = -1.f;
        int c_out = pos == 0 ? CMD_SOS : CMD_EOS, src = -1;
        if (ok && pos > 0 && pos - 1 < (int)used[gslot[g + 1]] - (int)used[gslot[g]]) {
            const int target = (int)used[gslot[g]] + pos - 1;
            int lo = gslot[g], hi = gslot[g + 1] - 1;      // the last slot of the group with used[s] <= target: it is in use
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((int)used[mid] <= target) lo = mid; else hi = mid - 1;
            }
            const int m = meta[lo], kind = m >> 16, t = m & 0xffff;
            const float* a = arg + (long long)t * N_ARGS;
            src = t - g * S;
            if (kind == PS_ROW_PASS) {
                c_out = cls[t] & PS_CLASS;
                if (c_out == CMD_M) { v[ARG_END] = a[ARG_END]; v[ARG_END + 1] = a[ARG_END + 1]; }
            } else {
                c_out = kind == PS_ROW_LINE ? CMD_L : CMD_C;
                v[ARG_END] = a[ARG_END]; v[ARG_END + 1] = a[ARG_END + 1];
                if (kind == PS_ROW_CUBIC) {
                    const float4 cc = ctrl[lo];
                    v[ARG_CONTROL1] = cc.x; v[ARG_CONTROL1 + 1] = cc.y; v[ARG_CONTROL2] = cc.z; v[ARG_CONTROL2 + 1] = cc.w;
                }
            }
        }
        oc[r] = (float)c_out;
        os[r] = src;
#pragma unroll
        for (int q = 0; q < N_ARGS; ++q) oa[(long long)r * N_ARGS + q] = v[q];
    }
}
}  // namespace

extern "C" int64_t dsvg_paths_simplify_workspace_bytes(int64_t N, int32_t G, int32_t S) {
    if (N <= 0 || G < 1 || S < 1) return 0;
    return N * 2 * (int64_t)G * S * (int64_t)(sizeof(float4) + sizeof(int));
}

extern "C" int dsvg_paths_simplify(const float* commands, const float* args, int64_t N, int32_t G, int32_t S, int32_t S_out,
                                   double tolerance, double epsilon, double cos_threshold, int32_t force_smooth, double unit,
                                   void* workspace, int64_t workspace_bytes, float* out_commands, float* out_args,
                                   int32_t* len_groups, int32_t* source_row, uint8_t* valid, void* stream) {
    DSVG_CHECK_ARG(commands && args && out_commands && out_args && len_groups && source_row && valid && workspace,
                   "paths_simplify: null pointer");
    DSVG_CHECK_ARG(N > 0 && N < (1ll << 31) && G >= 1 && S >= 2 && (int64_t)G * S <= PS_MAX_ROWS,
                   "paths_simplify: bad shape (N=%lld G=%d S=%d; S >= 2, G * S <= %d rows per icon)", (long long)N, G, S,
                   PS_MAX_ROWS);
    DSVG_CHECK_ARG(S_out >= 2 && (int64_t)G * S_out <= PS_MAX_ROWS,
                   "paths_simplify: bad output shape (G=%d S_out=%d; S_out >= 2, G * S_out <= %d rows per icon)", G, S_out,
                   PS_MAX_ROWS);
    const double big = 1.7976931348623157e308;      // finite: the comparisons are false for a NaN too
    DSVG_CHECK_ARG(tolerance > 0.0 && tolerance <= big && epsilon > 0.0 && epsilon <= big && unit > 0.0 && unit <= big,
                   "paths_simplify: tolerance, epsilon and unit are finite and > 0 (%g, %g, %g)", tolerance, epsilon, unit);
    DSVG_CHECK_ARG(cos_threshold >= -1.0 && cos_threshold <= 1.0, "paths_simplify: cos_threshold in [-1, 1] (%g)",
                   cos_threshold);
    DSVG_CHECK_ARG(workspace_bytes >= dsvg_paths_simplify_workspace_bytes(N, G, S) && ((uintptr_t)workspace & 15) == 0,
                   "paths_simplify: workspace of %lld bytes, 16-byte aligned (dsvg_paths_simplify_workspace_bytes)",
                   (long long)dsvg_paths_simplify_workspace_bytes(N, G, S));
    float4* ws_ctrl = (float4*)workspace;
    int* ws_meta = (int*)(ws_ctrl + N * 2 * (int64_t)G * S);
    hipLaunchKernelGGL(paths_simplify_kernel, dim3((unsigned)N), dim3(PS_THREADS), 0, (hipStream_t)stream, commands, args, G, S,
                       S_out, tolerance, epsilon, cos_threshold, force_smooth ? 1 : 0, unit, ws_ctrl, ws_meta, out_commands,
                       out_args, len_groups, source_row, valid);
    DSVG_LAUNCH_CHECK("paths_simplify");
    return 0;
}
