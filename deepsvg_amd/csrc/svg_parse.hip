// SVG path text -> the padded rows of the model, for a whole batch of strings: the reference's SVGPath.from_str(s).to_tensor()
// (deepsvg/svglib/svg_path.py:79-157, svg_command.py:51-120) and the `points` lists of its polylines and polygons
// (svg_primitive.py:196-207).  The definition is in include/dsvg.h; tests/svgio_ref.py restates it in plain Python, table by
// table, and tests/golden/svgio/parse.npz holds the reference's own results.
//   dsvg_svg_parse   five launches on one stream, no atomics, nothing read back:
//     slots_init / slots_claim / slots_mark   who fills which output group.  Every string stores its index at its slot (plain
//                      stores: one of them stays), then every string that does not find itself there marks the slot shared.
//                      Which index stayed is never read when the slot is shared, so the result does not depend on it.
//     svg_parse_kernel one wave (a workgroup of 64) per string.  The string is read in tiles of 64 bytes, one byte per lane.
//                      The number pattern is a nine-state automaton; a byte is a map of states, 9 x 4 bits in one 64-bit
//                      word, and an inclusive wave scan over the composition of these maps gives every lane the state in
//                      front of its byte; the state behind lane 63 is carried into the next tile.  From its state and its
//                      byte a lane knows whether a number ends in front of it and where (the pattern backtracks at most two
//                      bytes); a max-scan of the start flags gives it the start.  Ballots number the tokens (numbers and
//                      command letters) of the tile, the lane a number ends at converts it (exact integer digits and one
//                      float64 multiply or divide by an exact power of ten) and the tokens go to LDS in reading order.  Lane 0
//                      walks them: positions are float32 values added one at a time (the reference's `Point` is a float32
//                      array), which is sequential by definition.  The rows it produces collect in LDS and all lanes write
//                      them out, 44 contiguous bytes per row.
//                      dsvg_svg_parse_exact launches the kernel's other instantiation: a number the fast rule above refuses goes
//                      through the exact rule (decimal_exact.h: integers only) before it is called slow.
//     svg_finish_kernel  one workgroup per icon: the icon is valid when every string with a slot in it is OK or EMPTY; every
//                      group that no OK string of a valid icon wrote is written here as SOS, EOS...
// Every read of text is bounded by the string's offsets clamped to the buffer, every row write by S - 2 rows per group.
#include "dsvg_common.h"
#include "svg_seq.h"             // vocabulary, N_ARGS and the argument columns
#include "decimal_exact.h"       // the exact rule, integers only
#include "../../include/dsvg.h"

// positions are sums of float32 values, each add rounded once; nothing here may be contracted into a fused multiply-add
#pragma clang fp contract(off)

namespace {
constexpr int SV_TILE = DSVG_SVG_TILE;    // bytes per tile = lanes of the wave
constexpr int SV_ROWS = 64;               // rows that collect in LDS before all lanes write them out
constexpr int SV_TOK = 2 * SV_TILE;       // at most a number and a letter per byte

// byte classes and states of the number pattern [-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)? (tests/svgio_ref.py: NEXT, BEHIND, GOES_ON)
enum { K_DIGIT = 0, K_DOT = 1, K_SIGN = 2, K_EXP = 3, K_OTHER = 4 };
enum { Q_IDLE = 0, Q_SIGN = 1, Q_DOT0 = 2, Q_INT = 3, Q_INTDOT = 4, Q_FRAC = 5, Q_EXP0 = 6, Q_EXPSIGN = 7, Q_EXPD = 8, N_Q = 9 };

// the map of one byte class: nibble s = the state behind the byte when s is the state in front of it
constexpr uint64_t sv_map(int q0, int q1, int q2, int q3, int q4, int q5, int q6, int q7, int q8) {
    return (uint64_t)q0 | (uint64_t)q1 << 4 | (uint64_t)q2 << 8 | (uint64_t)q3 << 12 | (uint64_t)q4 << 16 | (uint64_t)q5 << 20 |
           (uint64_t)q6 << 24 | (uint64_t)q7 << 28 | (uint64_t)q8 << 32;
}
//                                        IDLE     SIGN     DOT0     INT        INTDOT   FRAC     EXP0        EXPSIGN  EXPD
constexpr uint64_t MAP_DIGIT = sv_map(Q_INT,   Q_INT,   Q_FRAC,  Q_INT,     Q_FRAC,  Q_FRAC,  Q_EXPD,     Q_EXPD,  Q_EXPD);
constexpr uint64_t MAP_DOT   = sv_map(Q_DOT0,  Q_DOT0,  Q_DOT0,  Q_INTDOT,  Q_DOT0,  Q_DOT0,  Q_DOT0,     Q_DOT0,  Q_DOT0);
constexpr uint64_t MAP_SIGN  = sv_map(Q_SIGN,  Q_SIGN,  Q_SIGN,  Q_SIGN,    Q_SIGN,  Q_SIGN,  Q_EXPSIGN,  Q_SIGN,  Q_SIGN);
constexpr uint64_t MAP_EXP   = sv_map(Q_IDLE,  Q_IDLE,  Q_IDLE,  Q_EXP0,    Q_IDLE,  Q_EXP0,  Q_IDLE,     Q_IDLE,  Q_IDLE);
constexpr uint64_t MAP_OTHER = 0;         // everything to IDLE
constexpr uint64_t MAP_ID = sv_map(0, 1, 2, 3, 4, 5, 6, 7, 8);

__device__ __forceinline__ uint64_t class_map(int k) {
    return k == K_DIGIT ? MAP_DIGIT : k == K_DOT ? MAP_DOT : k == K_SIGN ? MAP_SIGN : k == K_EXP ? MAP_EXP : MAP_OTHER;
}
__device__ __forceinline__ int map_at(uint64_t m, int s) { return (int)((m >> (4 * s)) & 15u); }
// first a, then b
__device__ __forceinline__ uint64_t map_then(uint64_t a, uint64_t b) {
    uint64_t r = 0;
#pragma unroll
    for (int s = 0; s < N_Q; ++s) r |= (uint64_t)map_at(b, map_at(a, s)) << (4 * s);
    return r;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ int byte_class(int b) {
    if (b >= '0' && b <= '9') return K_DIGIT;
    if (b == '.') return K_DOT;
    if (b == '+' || b == '-') return K_SIGN;
    if (b == 'e' || b == 'E') return K_EXP;
    return K_OTHER;
}
// MmZzLlHhVvCcSsQqTtAa
__device__ __forceinline__ bool is_letter(int b) {
    const int c = b | 0x20;
    return c == 'm' || c == 'z' || c == 'l' || c == 'h' || c == 'v' || c == 'c' || c == 's' || c == 'q' || c == 't' || c == 'a';
}
__device__ __forceinline__ int letter_arity(int lower) {
    switch (lower) {
        case 'm': case 'l': case 't': return 2;
        case 'h': case 'v': return 1;
        case 'c': return 6;
        case 's': case 'q': return 4;
        case 'a': return 7;
        default: return 0;
    }
}
// does the number that state q belongs to go on with a byte of class k
__device__ __forceinline__ bool goes_on(int q, int k) {
    switch (q) {
        case Q_INT: return k == K_DIGIT || k == K_DOT || k == K_EXP;
        case Q_FRAC: return k == K_DIGIT || k == K_EXP;
        case Q_EXP0: return k == K_DIGIT || k == K_SIGN;
        case Q_INTDOT: case Q_EXPSIGN: case Q_EXPD: return k == K_DIGIT;
        default: return false;
    }
}
__device__ __forceinline__ int behind(int q) { return q == Q_EXPSIGN ? 2 : (q == Q_INTDOT || q == Q_EXP0) ? 1 : 0; }

// the bytes [lo, hi) of one match -> its float64 value; false outside the fast path.  A template, like Walk below, only so that
// each instantiation of the kernel has a copy of its own with one caller, which the compiler inlines as it did before there were two
template <bool EXACT>
__device__ bool decimal(const uint8_t* __restrict__ t, long long lo, long long hi, double& out) {
    constexpr double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                   1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};     // exact in float64
    long long i = lo;
    bool neg = false;
    if (t[i] == '+' || t[i] == '-') {
        neg = t[i] == '-';
        ++i;
    }
    uint64_t w = 0;
    int kept = 0, zeros = 0;
    bool slow = false, frac = false;
    for (; i < hi; ++i) {
        const int b = t[i];
        if (b == 'e' || b == 'E') break;
        if (b == '.') {
            frac = true;
            continue;
        }
        const int d = b - '0';
        if (frac && d == 0) {
            ++zeros;                      // kept only when a digit follows
            continue;
        }
        const int times = frac ? zeros + 1 : 1;
        for (int z = 0; z < times; ++z) {
            if (w > (0xFFFFFFFFFFFFFFFFull - 9ull) / 10ull) slow = true;
            else w *= 10ull;
        }
        if (frac) {
            kept += zeros + 1;
            zeros = 0;
        }
        w += (uint64_t)d;
    }
    int ex = 0;
    bool eneg = false;
    if (i < hi) {
        ++i;
        if (i < hi && (t[i] == '+' || t[i] == '-')) {
            eneg = t[i] == '-';
            ++i;
        }
        for (; i < hi; ++i) ex = ex < 10000 ? ex * 10 + (t[i] - '0') : 100000;
    }
    const int e10 = (eneg ? -ex : ex) - kept;
    if (slow || w >= (1ull << 53) || e10 > 22 || e10 < -22) return false;
    const double v = e10 >= 0 ? (double)w * kPow10[e10] : (double)w / kPow10[-e10];
    out = neg ? -v : v;
    return true;
}

// tags of the token list a tile leaves in LDS
constexpr int TAG_NUMBER = 0, TAG_SLOW = 1;          // anything else: the command letter itself

struct WaveLds {
    double tok_val[SV_TOK];
    double num[8];                        // the numbers of the command that is forming
    float row_args[SV_ROWS * N_ARGS];
    float row_cmd[SV_ROWS];
    uint8_t tok_tag[SV_TOK];
};

// SVGCommand.from_str over the tokens and SVGPath.from_commands(allow_empty=False, add_closing=False) over its commands, row
// by row: lane 0 only
template <bool EXACT>
struct Walk {
    float px = 0.f, py = 0.f, ix = 0.f, iy = 0.f;    // position, initial position of the sub-path
    float bx = 0.f, by = 0.f, mx = 0.f, my = 0.f;    // control2 of the previous Bezier; the target of the open move
    bool bez = false, open = false, drawn = false;
    int letter = 0, have = 0, cmds = 0;              // the segment: its letter, numbers waiting, commands formed
    int kind = 0, npts = 0;
    float p0x = 0.f, p0y = 0.f;
    int err = DSVG_SVG_OK;                           // the first ARG_COUNT / SLOW_NUMBER in reading order
    bool overflow = false, range = false;
    int rows = 0, buffered = 0, cap = 0;             // rows so far, rows waiting in LDS, S - 2

    __device__ __forceinline__ void put(WaveLds& w, int cmd, float v0, float v1, float v2, float v3, float v4, float c1x,
                                        float c1y, float c2x, float c2y, float ex, float ey) {
        if (rows >= cap) {
            overflow = true;
            return;
        }
        const float v[N_ARGS] = {v0, v1, v2, v3, v4, c1x, c1y, c2x, c2y, ex, ey};
        const uint32_t mask = kCmdArgsMask[cmd];
#pragma unroll
        for (int q = 0; q < N_ARGS; ++q) {
            const bool on = (mask >> q) & 1u;
            if (on && !__builtin_isfinite(v[q])) range = true;
            w.row_args[buffered * N_ARGS + q] = on ? v[q] : -1.f;
        }
        w.row_cmd[buffered] = (float)cmd;
        ++buffered;
        ++rows;
    }
    __device__ __forceinline__ void emit(WaveLds& w, int cmd, float v0, float v1, float v2, float v3, float v4, float c1x,
                                         float c1y, float c2x, float c2y, float ex, float ey) {
        if (open) {
            if (!drawn) {
                put(w, CMD_M, 0, 0, 0, 0, 0, 0, 0, 0, 0, mx, my);
                drawn = true;
            }
            put(w, cmd, v0, v1, v2, v3, v4, c1x, c1y, c2x, c2y, ex, ey);
        }
        px = ex;
        py = ey;
        bez = cmd == CMD_C;
        bx = c2x;
        by = c2y;
    }
    __device__ __forceinline__ void close(WaveLds& w) {
        if (open && drawn) put(w, CMD_Z, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
        open = false;
        px = ix;
        py = iy;
        bez = false;
    }
    __device__ __forceinline__ void end_segment() {
        if (letter != 0 && (letter | 0x20) != 'z' && err == DSVG_SVG_OK && (cmds == 0 || have != 0)) err = DSVG_SVG_ARG_COUNT;
    }
    __device__ void command(WaveLds& w) {
        const double* a = w.num;
        const bool rel = (letter & 0x20) != 0;
        const int c = letter | 0x20;
        const float ox = rel ? px : 0.f, oy = rel ? py : 0.f;
        // a number becomes a float32 first, then the position is added in float32
        auto X = [&](int q) { const float v = (float)a[q]; return rel ? v + ox : v; };
        auto Y = [&](int q) { const float v = (float)a[q]; return rel ? v + oy : v; };
        const float rx = bez ? 2.f * px - bx : px, ry = bez ? 2.f * py - by : py;      // the reflected control point
        if (c == 'm' && cmds == 0) {
            const float x = X(0), y = Y(1);
            px = ix = mx = x;
            py = iy = my = y;
            bez = false;
            open = true;
            drawn = false;
        } else if (c == 'm' || c == 'l') {
            const float x = X(0), y = Y(1);
            emit(w, CMD_L, 0, 0, 0, 0, 0, 0, 0, 0, 0, x, y);
        } else if (c == 'h') {
            emit(w, CMD_L, 0, 0, 0, 0, 0, 0, 0, 0, 0, X(0), py);
        } else if (c == 'v') {
            emit(w, CMD_L, 0, 0, 0, 0, 0, 0, 0, 0, 0, px, Y(0));
        } else if (c == 'c') {
            const float c1x = X(0), c1y = Y(1), c2x = X(2), c2y = Y(3), ex = X(4), ey = Y(5);
            emit(w, CMD_C, 0, 0, 0, 0, 0, c1x, c1y, c2x, c2y, ex, ey);
        } else if (c == 's') {
            const float c2x = X(0), c2y = Y(1), ex = X(2), ey = Y(3);
            emit(w, CMD_C, 0, 0, 0, 0, 0, rx, ry, c2x, c2y, ex, ey);
        } else if (c == 'q') {
            const float cx = X(0), cy = Y(1), ex = X(2), ey = Y(3);
            emit(w, CMD_C, 0, 0, 0, 0, 0, cx, cy, cx, cy, ex, ey);
        } else if (c == 't') {
            const float ex = X(0), ey = Y(1);
            emit(w, CMD_C, 0, 0, 0, 0, 0, rx, ry, rx, ry, ex, ey);
        } else {                          // radii, angle and flags are not translated; a flag is int(value): no -0
            const float ex = X(5), ey = Y(6);
            const float fa = (float)(__builtin_trunc(a[3]) + 0.0), fs = (float)(__builtin_trunc(a[4]) + 0.0);
            emit(w, CMD_A, (float)a[0], (float)a[1], (float)a[2], fa, fs, 0, 0, 0, 0, ex, ey);
        }
        ++cmds;
    }
    __device__ void token(WaveLds& w, int tag, double val) {
        if (tag != TAG_NUMBER && tag != TAG_SLOW) {
            end_segment();
            letter = tag;
            have = 0;
            cmds = 0;
            if ((letter | 0x20) == 'z' && err == DSVG_SVG_OK) close(w);
            return;
        }
        if (kind == DSVG_SVG_PATH && letter == 0) return;         // numbers before the first letter are never converted
        if (err != DSVG_SVG_OK) return;
        if (tag == TAG_SLOW) {
            err = DSVG_SVG_SLOW_NUMBER;
            return;
        }
        if (kind != DSVG_SVG_PATH) {
            w.num[have++] = val;
            if (have == 2) {
                have = 0;
                const float x = (float)w.num[0], y = (float)w.num[1];
                if (npts == 0) {
                    p0x = x;
                    p0y = y;
                } else {
                    if (npts == 1) put(w, CMD_M, 0, 0, 0, 0, 0, 0, 0, 0, 0, p0x, p0y);
                    put(w, CMD_L, 0, 0, 0, 0, 0, 0, 0, 0, 0, x, y);
                }
                ++npts;
            }
            return;
        }
        if ((letter | 0x20) == 'z') {
            err = DSVG_SVG_ARG_COUNT;
            return;
        }
        w.num[have++] = val;
        if (have == letter_arity(letter | 0x20)) {
            have = 0;
            command(w);
        }
    }
    __device__ void finish(WaveLds& w) {
        if (kind == DSVG_SVG_PATH) {
            end_segment();
        } else {
            if (have != 0 && err == DSVG_SVG_OK) err = DSVG_SVG_ARG_COUNT;
            if (kind == DSVG_SVG_POLYGON && npts >= 2) put(w, CMD_Z, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ int status() const {
        return err != DSVG_SVG_OK ? err : overflow ? DSVG_SVG_ROWS_OVERFLOW : range ? DSVG_SVG_RANGE
                                        : rows == 0 ? DSVG_SVG_EMPTY : DSVG_SVG_OK;
    }
};

// ---- who fills which group ---------------------------------------------------------------------------------------------------
__global__ void slots_init_kernel(int32_t* __restrict__ owner, int32_t* __restrict__ shared, long long NG) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < NG) {
        owner[i] = -1;
        shared[i] = 0;
    }
}
__global__ void slots_claim_kernel(const int32_t* __restrict__ slot, long long P, long long NG, int32_t* __restrict__ owner) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) {
        const long long s = slot[p];
        if (s >= 0 && s < NG) owner[s] = (int32_t)p;
    }
}
__global__ void slots_mark_kernel(const int32_t* __restrict__ slot, long long P, long long NG, const int32_t* __restrict__ owner,
                                  int32_t* __restrict__ shared) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) {
        const long long s = slot[p];
        if (s >= 0 && s < NG && owner[s] != (int32_t)p) shared[s] = 1;
    }
}

// ---- one wave per string -------------------------------------------------------------------------------------------------------
// EXACT = false is the fast rule alone.  EXACT = true: a number the fast rule refuses goes through the exact rule before it is
// tagged TAG_SLOW - in a branch of its own behind the fast stores, so that the wave runs the long conversion once, with the
// lanes that need it active, however they are scattered over the tile.
template <bool EXACT>
__global__ __launch_bounds__(SV_TILE) void svg_parse_kernel(const uint8_t* __restrict__ data, long long B,
                                                            const int64_t* __restrict__ offsets, const uint8_t* __restrict__ kinds,
                                                            const int32_t* __restrict__ slot, long long P, long long NG, int S,
                                                            const int32_t* __restrict__ shared, float* __restrict__ out_cmd,
                                                            float* __restrict__ out_args, int32_t* __restrict__ len_groups,
                                                            int32_t* __restrict__ status) {
    __shared__ WaveLds w;
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const long long s = slot[p];
    if (s < -1 || s >= NG || (s >= 0 && shared[s] != 0)) {
        if (lane == 0) status[p] = DSVG_SVG_BAD_SLOT;
        return;
    }
    long long lo = offsets[p], hi = offsets[p + 1];
    lo = min(max(lo, 0ll), B);
    hi = min(max(hi, lo), B);
    const uint8_t* text = data + lo;
    const long long len = hi - lo;
    const int kind = kinds[p];
    float* g_cmd = s >= 0 ? out_cmd + s * S : nullptr;
    float* g_args = s >= 0 ? out_args + s * S * N_ARGS : nullptr;

    Walk<EXACT> walk;                     // lane 0's copy is the one that counts
    walk.kind = kind == DSVG_SVG_POLYLINE || kind == DSVG_SVG_POLYGON ? kind : DSVG_SVG_PATH;
    walk.cap = S - 2;
    int state = Q_IDLE;                   // behind the last byte of the tile before
    long long start = -1;                 // start of the number that is open there
    int written = 0;                      // rows already in global memory

    // all lanes: the rows waiting in LDS go out, 11 contiguous floats each
    auto flush = [&](int n) {
        __syncthreads();
        if (g_cmd != nullptr) {
            if (lane < n) g_cmd[1 + written + lane] = w.row_cmd[lane];
            for (int j = lane; j < n * N_ARGS; j += SV_TILE) g_args[(long long)(1 + written) * N_ARGS + j] = w.row_args[j];
        }
        written += n;
        __syncthreads();
    };
    // lane 0 walks the tokens [0, total) of the tile; whenever the row buffer fills, everybody writes it out
    auto consume = [&](int total, bool last) {
        int ti = 0;
        for (;;) {
            if (lane == 0) {
                while (ti < total && walk.buffered <= SV_ROWS - 3) {       // a token leaves at most two rows
                    walk.token(w, w.tok_tag[ti], w.tok_val[ti]);
                    ++ti;
                }
                if (last && ti >= total && walk.buffered <= SV_ROWS - 3) {
                    walk.finish(w);
                    ti = total + 1;
                }
            }
            const int n = __shfl(walk.buffered, 0, 64);
            const int at = __shfl(ti, 0, 64);
            flush(n);
            walk.buffered = 0;
            if (at >= total + (last ? 1 : 0)) break;
        }
    };

    for (long long base = 0; base <= len; base += SV_TILE) {     // one separator is read behind the last byte
        const long long i = base + lane;
        const int b = i < len ? (int)text[i] : ' ';
        const int k = byte_class(b);
        const bool letter = walk.kind == DSVG_SVG_PATH && is_letter(b);
        // the state in front of every byte: an inclusive scan of the maps, shifted by one lane, applied to the carried state
        uint64_t m = class_map(k);
#pragma unroll
        for (int d = 1; d < SV_TILE; d <<= 1) {
            const uint64_t up = shfl_up64(m, d);
            if (lane >= d) m = map_then(up, m);
        }
        uint64_t before = shfl_up64(m, 1);
        if (lane == 0) before = MAP_ID;
        const int q = map_at(before, state);
        const int nq = map_at(class_map(k), q);
        // what this byte ends and what it starts (tests/svgio_ref.py: step)
        const bool ends = q >= Q_INT && !goes_on(q, k);
        const long long end = i - behind(q);
        long long starts = -1;
        if (nq == Q_SIGN || (nq == Q_INT && q == Q_IDLE) || (nq == Q_DOT0 && q != Q_SIGN))
            starts = q == Q_EXPSIGN && nq == Q_DOT0 ? i - 1 : i;          // `4e+.5`: the sign starts the second number
        long long open = starts;            // inclusive max-scan: the last start at or in front of this byte
#pragma unroll
        for (int d = 1; d < SV_TILE; d <<= 1) {
            const long long up = (long long)shfl_up64((uint64_t)open, d);
            if (lane >= d) open = max(open, up);
        }
        long long mine = (long long)shfl_up64((uint64_t)open, 1);          // ... strictly in front of it
        if (lane == 0) mine = -1;
        mine = max(mine, start);
        // the tokens of the tile in reading order: a number that ends at a byte comes before the letter that byte is
        const unsigned long long nb = __ballot(ends), lb = __ballot(letter);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int at = __popcll(nb & below) + __popcll(lb & below);
        bool refused = false;               // EXACT only: a number inside the string that the fast rule did not take
        if (ends) {
            double v = 0.0;
            const bool fast = mine >= 0 && mine < end && end <= len && decimal<EXACT>(text, mine, end, v);
            w.tok_val[at] = v;
            w.tok_tag[at] = fast ? TAG_NUMBER : TAG_SLOW;
            if constexpr (EXACT) refused = !fast && mine >= 0 && mine < end && end <= len;
        }
        if constexpr (EXACT) {
            if (refused) {
                double v = 0.0;
                if (dsvg_exact::decimal_exact(text, mine, end, v)) {
                    w.tok_val[at] = v;
                    w.tok_tag[at] = TAG_NUMBER;
                }
            }
        }
        if (letter) w.tok_tag[at + (ends ? 1 : 0)] = (uint8_t)b;
        const int total = __popcll(nb) + __popcll(lb);
        state = __shfl(nq, SV_TILE - 1, 64);
        start = max(start, (long long)shfl64((uint64_t)open, SV_TILE - 1));
        __syncthreads();
        consume(total, base + SV_TILE > len);
    }

    const int st = __shfl(walk.status(), 0, 64);
    const int rows = __shfl(walk.rows, 0, 64);
    if (lane == 0) status[p] = st;
    if (st == DSVG_SVG_OK && g_cmd != nullptr) {
        // the frame and the padding; every other case is svg_finish_kernel's
        if (lane == 0) {
            g_cmd[0] = (float)CMD_SOS;
            len_groups[s] = rows;
        }
        for (int r = 1 + rows + lane; r < S; r += SV_TILE) g_cmd[r] = (float)CMD_EOS;
        for (int j = lane; j < N_ARGS; j += SV_TILE) g_args[j] = -1.f;
        for (long long j = (long long)(1 + rows) * N_ARGS + lane; j < (long long)S * N_ARGS; j += SV_TILE) g_args[j] = -1.f;
    }
}

// ---- one workgroup per icon ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void svg_finish_kernel(const int32_t* __restrict__ owner, const int32_t* __restrict__ shared,
                                                                const int32_t* __restrict__ status, long long P, int G, int S,
                                                                float* __restrict__ out_cmd, float* __restrict__ out_args,
                                                                int32_t* __restrict__ len_groups, uint8_t* __restrict__ valid) {
    const long long n = blockIdx.x;
    const int tid = threadIdx.x;
    auto state_of = [&](int g) -> int {      // -1: nobody fills the group
        const long long s = n * G + g;
        if (shared[s] != 0) return DSVG_SVG_BAD_SLOT;
        const long long o = owner[s];
        return o >= 0 && o < P ? status[o] : -1;
    };
    int good = 1;
    for (int g = tid; g < G; g += SP_THREADS) {
        const int st = state_of(g);
        if (st > DSVG_SVG_EMPTY) good = 0;
    }
    const int ok = __syncthreads_and(good);
    if (tid == 0) valid[n] = (uint8_t)(ok != 0);
    for (int g = tid; g < G; g += SP_THREADS)
        if (!ok || state_of(g) != DSVG_SVG_OK) len_groups[n * G + g] = 0;
    const long long R = (long long)G * S;
    for (long long t = tid; t < R; t += SP_THREADS) {
        const int g = (int)(t / S), r = (int)(t % S);
        if (ok && state_of(g) == DSVG_SVG_OK) continue;
        out_cmd[n * R + t] = r == 0 ? (float)CMD_SOS : (float)CMD_EOS;
    }
    for (long long j = tid; j < R * N_ARGS; j += SP_THREADS) {
        const int g = (int)(j / ((long long)S * N_ARGS));
        if (ok && state_of(g) == DSVG_SVG_OK) continue;
        out_args[n * R * N_ARGS + j] = -1.f;
    }
}
}  // namespace

template <bool EXACT>
static int svg_parse_launch(const uint8_t* data, int64_t B, const int64_t* offsets, const uint8_t* kind, const int32_t* slot,
                            int64_t P, int64_t N, int32_t G, int32_t S, int32_t* workspace, float* commands, float* args,
                            int32_t* len_groups, int32_t* status, uint8_t* valid, void* stream) {
    DSVG_CHECK_ARG(data && offsets && kind && slot && workspace && commands && args && len_groups && status && valid,
                   "svg_parse: null pointer");
    DSVG_CHECK_ARG(B >= 0 && B < (1ll << 31) && P >= 1 && P < (1ll << 31), "svg_parse: B = %lld bytes and P = %lld strings, need "
                   "0 <= B < 2^31 and 1 <= P < 2^31", (long long)B, (long long)P);
    DSVG_CHECK_ARG(N >= 1 && G >= 1 && S >= 2 && (int64_t)G * S <= SP_MAX_TOK && N * G < (1ll << 31),
                   "svg_parse: bad shape (N=%lld G=%d S=%d; S >= 2, G * S <= %d rows per icon, N * G < 2^31)", (long long)N, G, S,
                   SP_MAX_TOK);
    const long long NG = (long long)N * G;
    int32_t* owner = workspace;
    int32_t* shared = workspace + NG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(slots_init_kernel, dim3((unsigned)dsvg_cdiv(NG, 256)), dim3(256), 0, st, owner, shared, NG);
    hipLaunchKernelGGL(slots_claim_kernel, dim3((unsigned)dsvg_cdiv(P, 256)), dim3(256), 0, st, slot, (long long)P, NG, owner);
    hipLaunchKernelGGL(slots_mark_kernel, dim3((unsigned)dsvg_cdiv(P, 256)), dim3(256), 0, st, slot, (long long)P, NG, owner, shared);
    hipLaunchKernelGGL(svg_parse_kernel<EXACT>, dim3((unsigned)P), dim3(SV_TILE), 0, st, data, (long long)B, offsets, kind, slot,
                       (long long)P, NG, S, shared, commands, args, len_groups, status);
    hipLaunchKernelGGL(svg_finish_kernel, dim3((unsigned)N), dim3(SP_THREADS), 0, st, owner, shared, status, (long long)P, G, S,
                       commands, args, len_groups, valid);
    DSVG_LAUNCH_CHECK("svg_parse");
    return 0;
}

extern "C" int dsvg_svg_parse(const uint8_t* data, int64_t B, const int64_t* offsets, const uint8_t* kind, const int32_t* slot,
                              int64_t P, int64_t N, int32_t G, int32_t S, int32_t* workspace, float* commands, float* args,
                              int32_t* len_groups, int32_t* status, uint8_t* valid, void* stream) {
    return svg_parse_launch<false>(data, B, offsets, kind, slot, P, N, G, S, workspace, commands, args, len_groups, status, valid,
                                   stream);
}

extern "C" int dsvg_svg_parse_exact(const uint8_t* data, int64_t B, const int64_t* offsets, const uint8_t* kind,
                                    const int32_t* slot, int64_t P, int64_t N, int32_t G, int32_t S, int32_t* workspace,
                                    float* commands, float* args, int32_t* len_groups, int32_t* status, uint8_t* valid,
                                    void* stream) {
    return svg_parse_launch<true>(data, B, offsets, kind, slot, P, N, G, S, workspace, commands, args, len_groups, status, valid,
                                  stream);
}
