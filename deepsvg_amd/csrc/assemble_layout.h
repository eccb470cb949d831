// The token layout of an assembled batch, stated once for csrc/assemble.hip (the int16 store of numericalised rows) and
// csrc/paths_transform.hip (the float32 store, transformed and rounded as it is loaded): the SOS / rows / EOS / padding
// framing of SVGTensor.add_eos().add_sos().pad() (deepsvg/difflib/tensor.py:108-143), the per-group and the grouped
// addressing of a variant's slots, and the relative arguments of SVGTensor.get_relative_args (tensor.py:172-189).
//
// A row source `Src` is passed by value and gives
//   Row  load(long long r) const                         row r of the store as it is stored, as floats
//   void finish(Row& o, long long n) const               what item n does to a row it takes (nothing for the int16 store)
//   bool prev_end(long long j, long long n, float& px, float& py) const
//                                                        is row j a real command (m / l / c / a)?  then its end position as
//                                                        item n sees it, i.e. after finish
// One thread per output token, consecutive threads write consecutive tokens.
#pragma once
#include "dsvg_common.h"
#include "svg_seq.h"             // N_ARGS, the command ids, the argument mask

namespace {
struct Row {
    float cmd;
    float a[N_ARGS];
};

template <typename Src>
__global__ void assemble_kernel(const Src src, long long n_rows,
                                const int32_t* __restrict__ slot_off, long long n_slots,
                                const int32_t* __restrict__ variant, int G, int grouped, long long n_seq, int L,
                                float pad_val, float rel_shift,
                                float* __restrict__ commands, float* __restrict__ args,
                                float* __restrict__ args_rel) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_seq * L) return;
    const long long q = t / L;
    const int s = (int)(t % L);
    const long long n = grouped ? q : q / G;
    const int g = grouped ? 0 : (int)(q % G);
    const int span = grouped ? G : 1;
    long long slot = (long long)variant[n] * G + g;
    slot = min(max(slot, 0ll), n_slots - span);               // never read outside the store
    const long long begin = slot_off[slot];
    const int len = min((int)(slot_off[slot + span] - begin), L - 2);

    Row o;
    o.cmd = (s == 0) ? (float)CMD_SOS : (float)CMD_EOS;          // SOS, then EOS as end marker and as padding
#pragma unroll
    for (int a = 0; a < N_ARGS; ++a) o.a[a] = pad_val;
    const bool data = s >= 1 && s - 1 < len;
    const long long r = min(begin + max(s - 1, 0), n_rows - 1);
    const Row ld = src.load(r);                // unconditional load from a clamped address, selected afterwards
    if (data) {
        o = ld;
        src.finish(o, n);
    }

    commands[t] = o.cmd;
    if (args) {
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) args[t * N_ARGS + a] = o.a[a];
    }
    if (args_rel) {
        // SVGTensor.get_relative_args (tensor.py:172-189): positions of every real command (m/l/c/a) but the first
        // are taken relative to the end position of the previous real command; used slots are shifted by ARGS_DIM-1,
        // unused ones are PAD_VAL
        const int c = (int)o.cmd;
        float v[N_ARGS];
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) v[a] = o.a[a];
        if (data && c < CMD_EOS) {
            long long j = r - 1;
            bool found = false;
            float px = 0.f, py = 0.f;
            while (j >= begin) {                                 // previous real command (normally row r-1)
                if (src.prev_end(j, n, px, py)) {
                    found = true;
                    break;
                }
                --j;
            }
            if (found) {
#pragma unroll
                for (int q = ARG_CONTROL1; q < N_ARGS; q += 2) { v[q] -= px; v[q + 1] -= py; }
            }
        }
        const uint32_t m = (c >= 0 && c < N_CMD) ? kCmdArgsMask[c] : 0u;
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) args_rel[t * N_ARGS + a] = ((m >> a) & 1u) ? v[a] + rel_shift : pad_val;
    }
}

// host: the arguments dsvg_assemble_batch and dsvg_assemble_augmented share, refused under the name of the caller
inline int assemble_args_ok(const char* name, const void* rows, int64_t n_rows, const void* slot_off, int64_t n_slots,
                            const void* variant, int64_t n_items, int32_t G, int32_t grouped, int32_t L,
                            const void* commands, int align) {
    DSVG_CHECK_ARG(rows && slot_off && variant && commands, "%s: null pointer", name);
    DSVG_CHECK_ARG(n_rows > 0 && n_items > 0 && G > 0 && L >= 2 && n_slots >= G && n_slots % G == 0,
                   "%s: bad shape (n_rows=%lld n_items=%lld G=%d L=%d n_slots=%lld)", name, (long long)n_rows,
                   (long long)n_items, G, L, (long long)n_slots);
    DSVG_CHECK_ARG(((uintptr_t)rows & (uintptr_t)(align - 1)) == 0, "%s: rows must be %d-byte aligned", name, align);
    const long long n_seq = grouped ? n_items : n_items * G;
    DSVG_CHECK_ARG(n_seq * L < (1ll << 40), "%s: batch too large", name);
    return 0;
}
}  // namespace
