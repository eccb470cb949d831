"""graph-replayed bf16 training step of Hierarchical with max_seq_len = 100: python scripts/long_step_bench.py BATCH STEPS
(DSVG_LONG_MFMA=0: the path-level attention on the VALU long kernels)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepsvg_amd
from deepsvg_amd import ops
from deepsvg_amd.synthetic import make_batch, det_state_dict
from deepsvg_amd.trainer import TrainStep
B, steps = int(sys.argv[1]), int(sys.argv[2])
cfg = deepsvg_amd.Hierarchical()
cfg.use_vae = False
cfg.max_seq_len = 100
m = deepsvg_amd.SVGTransformer(cfg)
m.load_state_dict(det_state_dict(m, seed=3))
m = m.cuda().set_compute_dtype(torch.bfloat16).train()
ts = TrainStep(m, deepsvg_amd.SVGLoss(cfg).cuda(), use_graph=True)
c, a = make_batch(B, 8, 100, seed=1)
c, a = c.cuda(), a.cuda()
for _ in range(3):
    ld = ts.step(c, a)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    ld = ts.step(c, a)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
print(json.dumps({"batch": B, "long_mfma": ops.LONG_MFMA, "step_ms": round(dt * 1e3, 3), "loss": ld["loss"].item(),
                  "tokens": int(c.numel())}), flush=True)
