// Device-side batch assembly: the per-item cat / pad chain of SVGTensorDataset.get_data
// (deepsvg/svgtensor_dataset.py:164-205; SVGTensor.add_eos/add_sos/pad, deepsvg/difflib/tensor.py:108-143) and the
// DataLoader's default collate, as one gather over a packed icon store.
//
// Store layout (built once on the host, deepsvg_amd/dataset.py):
//   rows     int16 [R, 12]   one drawing command per row: (command, 11 arguments in SVGTensor.arg_keys order);
//                            the values are the numericalised integers -1..255 of the .pkl tensors
//   slot_off int32 [n_slots+1]  row range of slot (variant, group) = variant*G + group, a variant being one stored
//                               (icon, augmentation) pair; the groups of a variant are stored back to back, so the
//                               "grouped" sequence (all groups concatenated, svgtensor_dataset.py:175) is the span
//                               of its G slots
// Pure integer / byte movement: HBM-bound, 24 B read + 48..92 B written per output token; one thread per token,
// consecutive threads write consecutive tokens.
#include "dsvg_common.h"
#include "svg_seq.h"             // N_ARGS, the command ids
#include "assemble_layout.h"     // the token layout: assemble_kernel over a row source
#include "../../include/dsvg.h"

namespace {
constexpr int ROW_W = N_ARGS + 1;  // int16 per stored row

// the int16 store: rows are taken as they are stored
struct Int16Rows {
    const int16_t* __restrict__ rows;

    __device__ __forceinline__ Row load(long long r) const {
        // 24-byte rows: three 8-byte loads (the array base is at least 8-byte aligned)
        const uint2* p = reinterpret_cast<const uint2*>(rows + r * ROW_W);
        const uint2 q0 = p[0], q1 = p[1], q2 = p[2];
        const uint32_t w[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
        Row o;
        o.cmd = (float)(int16_t)(w[0] & 0xFFFFu);
#pragma unroll
        for (int a = 0; a < N_ARGS; ++a) {
            const int e = a + 1;
            o.a[a] = (float)(int16_t)((w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu);
        }
        return o;
    }
    __device__ __forceinline__ void finish(Row&, long long) const {}
    __device__ __forceinline__ bool prev_end(long long j, long long, float& px, float& py) const {
        const int16_t* pr = rows + j * ROW_W;
        if (pr[0] >= CMD_EOS) return false;
        px = (float)pr[1 + ARG_END];
        py = (float)pr[2 + ARG_END];
        return true;
    }
};
}  // namespace

extern "C" int dsvg_assemble_batch(const int16_t* rows, int64_t n_rows, const int32_t* slot_off, int64_t n_slots,
                                   const int32_t* variant, int64_t n_items, int32_t G, int32_t grouped,
                                   int32_t L, float pad_val, int32_t args_dim, float* commands, float* args,
                                   float* args_rel, void* stream) {
    if (assemble_args_ok("assemble_batch", rows, n_rows, slot_off, n_slots, variant, n_items, G, grouped, L, commands, 8))
        return -1;
    const long long n_seq = grouped ? n_items : n_items * G;
    hipLaunchKernelGGL(assemble_kernel<Int16Rows>, dim3((unsigned)dsvg_cdiv(n_seq * L, 256)), dim3(256), 0,
                       (hipStream_t)stream, Int16Rows{rows}, (long long)n_rows, slot_off, (long long)n_slots, variant, G,
                       grouped, n_seq, L, pad_val, (float)(args_dim - 1), commands, args, args_rel);
    DSVG_LAUNCH_CHECK("assemble_batch");
    return 0;
}
