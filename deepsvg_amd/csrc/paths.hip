// Canonical path order of a batch: SVG.canonicalize() of the reference (deepsvg/svglib/svg.py:333-349: split_paths,
// filter_consecutives, filter_empty, reorder, sort, canonicalize, drop_z) on the tensors themselves, for every icon of a batch
// in one launch - what the reference does one icon at a time on the host, through Python objects.  The definition is in
// include/dsvg.h; tests/paths_ref.py restates it in float64 and tests/golden/paths/ holds the reference's own results.
//   dsvg_canonicalize   one workgroup per icon.  Four ballot prefix scans classify the rows: the rows before each group's
//                       first EOS, the markers (`m`, `z`) and with them the marker every row hangs on, the commands that
//                       survive the degeneracy test, the sub-paths that keep at least one command.  One lane per sub-path
//                       then walks its commands (end positions staged in LDS): the order-dependent scan for the top-left-most
//                       command of a closed sub-path, and the float64 determinant sum in the rotated order.  A stable rank
//                       sort over the (y, x) keys orders the sub-paths.  The output is a gather: every output row works out
//                       which input row it copies (its own controls swapped when reversed, its neighbour's end position).
// Every value written is a copy of an input value (or its rounded / clipped form with numericalize); no atomics, no workspace:
// bit-reproducible, and nothing is read back to the host.
#include "dsvg_common.h"
#include "svg_seq.h"             // vocabulary, block_flag_scan (here with 16-bit counts: LDS is short)
#include "../../include/dsvg.h"

// the closeness tests and the determinant sum are restated operation by operation in tests/paths_ref.py: no fused multiply-add
#pragma clang fp contract(off)

namespace {
constexpr int CP_THREADS = SP_THREADS;
constexpr int CP_MAX_ROWS = SP_MAX_TOK;   // G * S rows of one icon: the largest two-stage config, 8 groups of 256
constexpr int CP_DEAD = 255;              // class of a row at or behind its group's first EOS
constexpr int CP_CLOSED = 1, CP_REVERSED = 2;
typedef unsigned short cp_u16;

// fp32 norm of Point.norm() (np.linalg.norm of a float32 pair): products, sum and root rounded to fp32 one by one.  The root
// has to be the correctly rounded one: on the integer grid it alone decides the closeness test of two norms.  __fsqrt_rn is
// v_sqrt_f32 here (1 ulp, and 4 of the 13 golden icons built on such pairs came out rotated differently with it); the
// float64 root of an fp32 number rounded to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits).
__device__ __forceinline__ float cp_norm(float x, float y) {
    return (float)sqrt((double)__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
}
// np.allclose(s, e) of one coordinate: |s - e| <= atol + rtol |e|
__device__ __forceinline__ bool cp_close(float s, float e) {
    return fabs((double)s - (double)e) <= 1e-8 + 1e-5 * fabs((double)e);
}
// a key that orders like the float (-0 == +0, NaN last): the rank sort needs a total order to stay a permutation
__device__ __forceinline__ unsigned cp_key(float v) {
    const unsigned u = __float_as_uint(v + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cp_num(float v, int n) { return fminf(fmaxf(rintf(v), 0.f), (float)(n - 1)); }
__device__ __forceinline__ long long cp_num(long long v, int n) { return v < 0 ? 0 : (v > n - 1 ? (long long)(n - 1) : v); }

template <typename T, int MAXT>
__global__ __launch_bounds__(CP_THREADS) void canonicalize_kernel(
    const T* __restrict__ commands, const T* __restrict__ args, int G, int S, int G_out, int S_out, int layout, int num,
    T* __restrict__ out_cmd, T* __restrict__ out_args, int32_t* __restrict__ n_groups, int32_t* __restrict__ len_groups,
    int32_t* __restrict__ source_group, uint8_t* __restrict__ reversed, uint8_t* __restrict__ valid) {
    constexpr int MAXP = MAXT / 2;            // a sub-path needs its `m` and one command
    __shared__ float ex[MAXT], ey[MAXT];      // end position of every row (the start point of the next)
    __shared__ unsigned char cls[MAXT];       // command of a live row, CP_DEAD behind the group's first EOS
    __shared__ cp_u16 pa[MAXT + 1];           // scan 1: EOS rows before t; scan 4: surviving sub-paths before marker k
    __shared__ cp_u16 pm[MAXT + 1];           // scan 2: markers (live m / z) before row t
    __shared__ cp_u16 pk[MAXT + 1];           // scan 3: kept commands before row t
    __shared__ cp_u16 markpos[MAXT];          // row of the k-th marker
    __shared__ cp_u16 krow[MAXT];             // row of the j-th kept command
    __shared__ cp_u16 sp_j0[MAXP], sp_cnt[MAXP], sp_best[MAXP], sp_grp[MAXP], order[MAXP], off[MAXP + 1];
    __shared__ unsigned char sp_flag[MAXP];
    __shared__ unsigned kx[MAXP], ky[MAXP];
    __shared__ int wtot[MAXT / 64];
    __shared__ int s_bad;

    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int R = G * S;
    const T* cmd = commands + b * R;
    const T* arg = args + b * R * N_ARGS;

    // ---- rows in: class and end position -------------------------------------------------------------------------------
    for (int t = tid; t < R; t += CP_THREADS) {
        const int c = (int)cmd[t];
        cls[t] = (unsigned char)((c >= 0 && c <= 6) ? c : 7);
        ex[t] = (float)arg[(long long)t * N_ARGS + ARG_END];
        ey[t] = (float)arg[(long long)t * N_ARGS + ARG_END + 1];
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();

    // ---- scan 1: a group ends at its first EOS -------------------------------------------------------------------------------
    block_flag_scan<MAXT>(R, pa, wtot, [&](int t) { return t < R && cls[t] == CMD_EOS; });
    for (int t = tid; t < R; t += CP_THREADS) {
        if (pa[t + 1] != pa[(t / S) * S]) cls[t] = CP_DEAD;
        else if (cls[t] == CMD_A) s_bad = 1;                                   // arcs are out of scope: the icon is invalid
    }
    __syncthreads();

    // ---- scan 2: markers; a row hangs on the last marker at or before it in its group -------------------------------
    block_flag_scan<MAXT>(R, pm, wtot, [&](int t) { return t < R && (cls[t] == CMD_M || cls[t] == CMD_Z); });
    for (int t = tid; t < R; t += CP_THREADS)
        if (pm[t + 1] > pm[t]) markpos[pm[t]] = (cp_u16)t;
    __syncthreads();
    const int n_mark = pm[R];

    // ---- scan 3: the commands that stay: `l` / `c` under an `m`, not degenerate -------------------------------------
    block_flag_scan<MAXT>(R, pk, wtot, [&](int t) {
        if (t >= R || (cls[t] != CMD_L && cls[t] != CMD_C)) return false;
        const int nm = pm[t + 1];
        if (nm == pm[(t / S) * S] || cls[markpos[nm - 1]] != CMD_M) return false;      // before the first m, or behind a z
        return !(cp_close(ex[t - 1], ex[t]) && cp_close(ey[t - 1], ey[t]));           // (t - 1 is in the group: the m is)
    });
    for (int t = tid; t < R; t += CP_THREADS)
        if (pk[t + 1] > pk[t]) krow[pk[t]] = (cp_u16)t;
    __syncthreads();

    // ---- scan 4: the sub-paths that stay: an `m` with at least one kept command before the group's next marker ----------
    auto mark_end = [&](int k) {              // first row behind the rows of marker k
        const int g = markpos[k] / S;
        return (k + 1 < n_mark && markpos[k + 1] / S == g) ? (int)markpos[k + 1] : (g + 1) * S;
    };
    block_flag_scan<MAXT>(R, pa, wtot, [&](int k) {
        if (k >= n_mark) return false;
        const int mr = markpos[k];
        return cls[mr] == CMD_M && pk[mark_end(k)] > pk[mr];
    });
    const int P = pa[R];
    for (int k = tid; k < n_mark; k += CP_THREADS)
        if (pa[k + 1] > pa[k]) {
            const int p = pa[k], mr = markpos[k], e = mark_end(k);
            sp_j0[p] = pk[mr];
            sp_cnt[p] = (cp_u16)(pk[e] - pk[mr]);
            sp_grp[p] = (cp_u16)(mr / S);
            sp_flag[p] = (e < (mr / S + 1) * S && cls[e] == CMD_Z) ? CP_CLOSED : 0;
        }
    __syncthreads();

    // ---- one lane per sub-path: rotation, sort key, orientation ----------------------------------------------------
    for (int p = tid; p < P; p += CP_THREADS) {
        const int j0 = sp_j0[p], cnt = sp_cnt[p];
        int best = 0;
        int t = krow[j0];
        float qx = ex[t - 1], qy = ey[t - 1];
        if (sp_flag[p] & CP_CLOSED) {
            float nq = cp_norm(qx, qy);
            for (int i = 1; i < cnt; ++i) {
                t = krow[j0 + i];
                const float px = ex[t - 1], py = ey[t - 1];
                bool left;
                float np = 0.f;
                bool have_np = false;
                if (py == qy) left = px < qx;
                else {
                    left = py < qy;
                    if (!left && px < qx) {
                        np = cp_norm(px, py);
                        have_np = true;
                        const float d = fabsf(__fsub_rn(np, nq));
                        left = (double)d <= 1e-8 + 1e-5 * fabs((double)nq);
                    }
                }
                if (left) {
                    best = i; qx = px; qy = py;
                    nq = have_np ? np : cp_norm(px, py);
                }
            }
        }
        sp_best[p] = (cp_u16)best;
        kx[p] = cp_key(qx);
        ky[p] = cp_key(qy);
        bool cw;
        if (cnt == 1) {
            t = krow[j0];
            const float sx = ex[t - 1], sy = ey[t - 1], fx = ex[t], fy = ey[t];
            cw = single_command_clockwise(sx, sy, fx, fy);
        } else {
            double det = 0.0;
            int j = best;
            for (int i = 0; i < cnt; ++i) {
                t = krow[j0 + j];
                det += orientation_term(ex[t - 1], ey[t - 1], ex[t], ey[t]);
                if (++j == cnt) j = 0;
            }
            cw = det >= 0.0;
        }
        if (!cw) sp_flag[p] |= CP_REVERSED;
        if (layout == DSVG_PATHS_GROUPED && cnt + 1 > S_out - 2) s_bad = 1;
    }
    __syncthreads();

    // ---- stable rank sort by (y, x) of the first command's start ------------------------------------------------------
    for (int p = tid; p < P; p += CP_THREADS) {
        const unsigned y = ky[p], x = kx[p];
        int rank = 0;
        for (int q = 0; q < P; ++q) {
            const unsigned yq = ky[q], xq = kx[q];
            rank += (yq < y || (yq == y && (xq < x || (xq == x && q < p)))) ? 1 : 0;
        }
        order[rank] = (cp_u16)p;
    }
    __syncthreads();
    const bool ok = !s_bad && P <= G_out && (layout == DSVG_PATHS_GROUPED || (int)pk[R] + P <= S_out - 2);
    if (layout == DSVG_PATHS_CONCAT && ok) {
        if (tid == 0) {
            int o = 0;
            for (int k = 0; k < P; ++k) { off[k] = (cp_u16)o; o += sp_cnt[order[k]] + 1; }
            off[P] = (cp_u16)o;
        }
        __syncthreads();
    }

    // ---- per-icon and per-group results ---------------------------------------------------------------------------------
    if (tid == 0) { n_groups[b] = ok ? P : 0; valid[b] = ok ? 1 : 0; }
    for (int k = tid; k < G_out; k += CP_THREADS) {
        const bool used = ok && k < P;
        const int p = used ? order[k] : 0;
        const long long o = b * G_out + k;
        len_groups[o] = used ? sp_cnt[p] + 1 : 0;
        source_group[o] = used ? (int)sp_grp[p] : -1;
        reversed[o] = (used && (sp_flag[p] & CP_REVERSED)) ? 1 : 0;
    }

    // ---- rows out: a gather ---------------------------------------------------------------------------------------
    const int rows_out = layout == DSVG_PATHS_GROUPED ? G_out * S_out : S_out;
    const int n_used = ok ? P : 0;
    T* oc = out_cmd + b * rows_out;
    T* oa = out_args + b * rows_out * N_ARGS;
    for (int r = tid; r < rows_out; r += CP_THREADS) {
        int k = -1, i = 0;                    // output group and row inside it (0 = its m); k < 0: SOS / EOS
        int pos;
        if (layout == DSVG_PATHS_GROUPED) {
            pos = r % S_out;
            const int kk = r / S_out;
            if (pos > 0 && kk < n_used && pos - 1 <= (int)sp_cnt[order[kk]]) { k = kk; i = pos - 1; }
        } else {
            pos = r;
            if (pos > 0 && n_used > 0 && pos - 1 < (int)off[n_used]) {
                int lo = 0, hi = n_used - 1;  // the last k with off[k] <= pos - 1
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if ((int)off[mid] <= pos - 1) lo = mid; else hi = mid - 1;
                }
                k = lo; i = pos - 1 - off[lo];
            }
        }
        T v[N_ARGS];
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) v[a] = (T)-1;
        int c_out = pos == 0 ? CMD_SOS : CMD_EOS;
        if (k >= 0) {
            const int p = order[k];
            const int j0 = sp_j0[p], cnt = sp_cnt[p], best = sp_best[p];
            const bool rev = sp_flag[p] & CP_REVERSED;
            int first = ARG_END;              // first enabled argument column
            if (i == 0) {
                c_out = CMD_M;
                // the first command's start; reversed: the end of the command that was last
                const int t = rev ? krow[j0 + (best + cnt - 1) % cnt] : krow[j0 + best] - 1;
                v[ARG_END] = arg[(long long)t * N_ARGS + ARG_END];
                v[ARG_END + 1] = arg[(long long)t * N_ARGS + ARG_END + 1];
            } else {
                const int ci = rev ? cnt - i : i - 1;
                const int t = krow[j0 + (best + ci) % cnt];
                const T* a = arg + (long long)t * N_ARGS;
                c_out = cls[t];
                const T* e = rev ? a - N_ARGS : a;          // reversed: the command ends where it started
                v[ARG_END] = e[ARG_END];
                v[ARG_END + 1] = e[ARG_END + 1];
                if (c_out == CMD_C) {
                    first = ARG_CONTROL1;
                    constexpr int C1 = ARG_CONTROL1, C2 = ARG_CONTROL2;
                    v[C1] = rev ? a[C2] : a[C1]; v[C1 + 1] = rev ? a[C2 + 1] : a[C1 + 1];
                    v[C2] = rev ? a[C1] : a[C2]; v[C2 + 1] = rev ? a[C1 + 1] : a[C2 + 1];
                }
            }
            if (num > 0) {
#pragma unroll
                for (int a = ARG_CONTROL1; a < N_ARGS; ++a)
                    if (a >= first) v[a] = cp_num(v[a], num);
            }
        }
        oc[r] = (T)c_out;
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) oa[(long long)r * N_ARGS + a] = v[a];
    }
}

template <typename T>
void canonicalize_launch(const void* commands, const void* args, int64_t N, int G, int S, int G_out, int S_out, int layout,
                         int num, void* out_commands, void* out_args, int32_t* n_groups, int32_t* len_groups,
                         int32_t* source_group, uint8_t* reversed, uint8_t* valid, hipStream_t st) {
    // icons of at most 256 rows (every one-stage config, two-stage up to 8 x 32) take the image with a quarter of the LDS
    if (G * S <= 256)
        hipLaunchKernelGGL((canonicalize_kernel<T, 256>), dim3((unsigned)N), dim3(CP_THREADS), 0, st, (const T*)commands,
                           (const T*)args, G, S, G_out, S_out, layout, num, (T*)out_commands, (T*)out_args, n_groups, len_groups,
                           source_group, reversed, valid);
    else
        hipLaunchKernelGGL((canonicalize_kernel<T, CP_MAX_ROWS>), dim3((unsigned)N), dim3(CP_THREADS), 0, st,
                           (const T*)commands, (const T*)args, G, S, G_out, S_out, layout, num, (T*)out_commands, (T*)out_args,
                           n_groups, len_groups, source_group, reversed, valid);
}
}  // namespace

extern "C" int dsvg_canonicalize(int32_t itype, const void* commands, const void* args, int64_t N, int32_t G, int32_t S,
                                 int32_t G_out, int32_t S_out, int32_t layout, int32_t numericalize, void* out_commands,
                                 void* out_args, int32_t* n_groups, int32_t* len_groups, int32_t* source_group,
                                 uint8_t* reversed, uint8_t* valid, void* stream) {
    DSVG_CHECK_ARG(commands && args && out_commands && out_args && n_groups && len_groups && source_group && reversed && valid,
                   "canonicalize: null pointer");
    DSVG_CHECK_ARG(itype == DSVG_F32 || itype == DSVG_I64, "canonicalize: itype %d is neither DSVG_F32 nor DSVG_I64", itype);
    DSVG_CHECK_ARG(layout == DSVG_PATHS_GROUPED || layout == DSVG_PATHS_CONCAT, "canonicalize: unknown layout %d", layout);
    DSVG_CHECK_ARG(N > 0 && N < (1ll << 31) && G >= 1 && S >= 1 && (int64_t)G * S <= CP_MAX_ROWS,
                   "canonicalize: bad shape (N=%lld G=%d S=%d; G * S <= %d rows per icon)", (long long)N, G, S, CP_MAX_ROWS);
    DSVG_CHECK_ARG(G_out >= 1 && S_out >= 2 && (int64_t)G_out * S_out <= (1ll << 24),
                   "canonicalize: bad output shape (G_out=%d S_out=%d; G_out >= 1, S_out >= 2, G_out * S_out <= 2^24)", G_out, S_out);
    DSVG_CHECK_ARG(numericalize >= 0 && numericalize <= (1 << 24), "canonicalize: numericalize = %d, need 0 (off) .. 2^24",
                   numericalize);
    hipStream_t st = (hipStream_t)stream;
    if (itype == DSVG_I64)
        canonicalize_launch<long long>(commands, args, N, G, S, G_out, S_out, layout, numericalize, out_commands, out_args,
                                       n_groups, len_groups, source_group, reversed, valid, st);
    else
        canonicalize_launch<float>(commands, args, N, G, S, G_out, S_out, layout, numericalize, out_commands, out_args, n_groups,
                                   len_groups, source_group, reversed, valid, st);
    DSVG_LAUNCH_CHECK("canonicalize");
    return 0;
}
