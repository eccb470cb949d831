"""bf16 attention of 4,096 sequences x 8 heads at S = 66, 102, 130, 256 (lengths uniform in [S/4, S-2]): the matrix-core
long kernels (path_stage=True) against the VALU long kernels, forward and backward, time and algorithmic HBM bytes/s
(q|k|v + out; q|k|v + dO + dq|dk|dv).  usage: python scripts/long_attn_bench.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsvg_amd import ops
torch.manual_seed(0)
n, H = 4096, 8
res = []
for S in (66, 102, 130, 256):
    lens = torch.randint(max(2, S // 4), S - 1, (n,), dtype=torch.int32).cuda()
    qkv = (torch.randn(n * S, 768, device="cuda") * 0.7).to(torch.bfloat16)
    dout = torch.randn(n * S, 256, device="cuda").to(torch.bfloat16)
    row = {"S": S, "mean_len": lens.float().mean().item()}
    for name, ps in (("mfma", True), ("valu", False)):
        f = lambda: ops.attention_fwd(qkv, lens, n, S, H, 32 ** -0.5, path_stage=ps)
        b = lambda: ops.attention_bwd(qkv, lens, dout, n, S, H, 32 ** -0.5, path_stage=ps)
        for lab, fn, nbytes in (("fwd", f, (768 + 256) * 2 * n * S), ("bwd", b, (768 + 256 + 768) * 2 * n * S)):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 5
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            row[f"{name}_{lab}_us"] = round(ms * 1e3, 1)
            row[f"{name}_{lab}_GBps"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
    print(json.dumps(row), flush=True)
