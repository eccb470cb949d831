#!/usr/bin/env python
"""Benchmark of the hot path: one full training step (deepsvg/train.py:92-106 = forward + SVGLoss + backward +
clip_grad_norm_ + AdamW) of hierarchical_ordered (G=8, S=30, d_model=256) at 512 icons per GPU, synthetic data,
on N MI355X (one process per GPU, RCCL gradient all-reduce).

    python bench.py --gpus 1 --steps 20 --warmup 5 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line: `value` icons/s and `ms_per_step` of the K timed steps.  The timed loop rotates 8 distinct
device-resident batches (different layout buckets included; `graphs` reports how many hipGraphs that took).  A plain run sets
up, warms up, times the K steps and prints the line; `--dump-outputs DIR` also writes what the last timed step computed
(dump_outputs).  The extra objects below are measured with `--full` only (null in a plain run):
  roofline     the FFN sub-block of the 16 layers (fused forward kernel on the large stages, its share of the fused per-layer
               kernels on the 4096-row stages, the backward launches: dropout replay, gated dX GEMM, fused dx + LayerNorm-
               backward kernel, the weight-gradient GEMMs, the finishing kernel, and its share of the batched gradient
               reductions), timed live with HIP events around the launches of the timed step's own sequence (issued eagerly
               behind a short queue of GPU work: events cannot be recorded inside a replayed hipGraph on this runtime; the
               graph-mode durations of the same kernels are the committed rocprofv3 trace, `graph_mode_check`).  bound =
               "mfma": `frac` = ALGORITHMIC FLOPs the launches executed (524,288 FLOP per token-layer
               forward, x3 trained; skipped padding and recomputation are not counted) / that time / 2.5 PFLOP/s.
               `fused_fwd_kernel` is the dominant kernel alone; `traffic` is a committed rocprofv3 --pmc measurement.
  fp32         the parity path (fp32 storage, exact-fp32 MFMA): ms/step and icons/s of the same step, same batch
  dense_layout the same bf16 step with every exact work-skipping layout OFF (padded encoder, all decoder groups, dense head):
               like for like with the padded work `torch_rocm_reference` does
  secondary    BASELINE configs[3] / [4] as short legs: C4 one-stage train step, C5 one-shot and autoregressive decode of 8192
  in_kernel_clock / config.clock_mhz   the shader clock: sysfs sclk sampled during the timed loop, and s_memtime ticks per
               s_memrealtime microsecond inside ffn_fwd (the chip clocks to its power budget: `fused_fwd_kernel` also
               carries its fraction of the MFMA peak at the clock it actually ran at)
  torch_rocm_reference   the reference's step as stock PyTorch ops (the oracle module: aten / rocBLAS / MIOpen kernels,
               fp32, dropout on) on the SAME MI355X and batch: what the hand-written kernels buy over aten on this chip
  cpu_baseline the CPU restatement of the reference step (oracle/, kind "port": /root/reference does not exist on the GPU
               box), dropout ON like the reference's train mode, at batch 60 (the reference's per-GPU default) and at
               batch 2 (BASELINE configs[0]), each on a bounded sample, on a thread count that finishes
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "6")     # before the HIP runtime comes up (deepsvg_amd/trainer.py HW_QUEUES_NOTE)

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FFN_FLOP_PER_ICON_TRAIN = 3.2716e9      # 2080 token-layers x 524,288 FLOP x 3
STEP_FLOP_PER_ICON_TRAIN = 8.115e9      # whole step
PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}   # MI355X dense MFMA peaks (MI355X_MICROARCH.md)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512, help="icons per GPU")
    ap.add_argument("--dtype", default=os.environ.get("DSVG_BENCH_DTYPE", "bf16"), choices=["bf16", "fp32"])
    ap.add_argument("--graph", type=int, default=int(os.environ.get("DSVG_BENCH_GRAPH", "-1")),
                    help="1: replay the step as a hipGraph (one graph per layout bucket, the layout plan runs eagerly "
                         "before each replay), 0: eager launches, -1 (default): time both during the warm-up and keep "
                         "the faster (eager wins when the host dispatches ~650 launches faster than the GPU runs them)")
    ap.add_argument("--pack-encoder", type=int, default=int(os.environ.get("DSVG_PACK_ENCODER", "1")),
                    help="1: first encoder stage on the valid tokens only (exact, SURVEY.md 7.3-12); 0: padded layout")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--ffn-replay", type=int, default=0,
                    help="N > 0: after the roofline leg replay ONLY the step's FFN GEMM launches N times on random "
                         "operands of the recorded shapes (for a rocprofv3 --pmc pass, scripts/gpu_ffn_traffic.sh)")
    ap.add_argument("--cpu-batch", type=int, default=60)
    ap.add_argument("--batches", type=int, default=8, help="distinct device-resident batches rotated through the loop")
    ap.add_argument("--no-torch-ref", action="store_true", help="skip the stock-PyTorch-on-this-GPU sub-record")
    ap.add_argument("--no-fp32", action="store_true", help="skip the fp32 parity-path sub-record")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip the dense_layout / secondary / in-kernel clock legs")
    ap.add_argument("--cpu-leg", type=int, default=0, help="internal: run one CPU-baseline leg on this many threads and exit")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline (sysfs clock sampling, roofline, fp32, dense layout, secondary "
                         "workloads, in-kernel clock, one-rank RCCL, stock-PyTorch reference, CPU baseline; the --no-* options "
                         "above switch single legs off again).  Without it the run times the train step and prints its line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step to DIR/<name>.npy (float32, < 64 MB): the loss "
                         "dict, the flat gradient, a fixed sample of the updated parameters")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.ffn_replay > 0 and not a.full:
        ap.error("--ffn-replay runs after the roofline leg: it needs --full")
    return a


def _oracle_step_fn(cfg, sd, batch, device, dropout, seed=4242):
    """one train step of the reference restated with stock PyTorch ops (oracle/svg_transformer_oracle.py): forward +
    SVGLoss + backward + clip_grad_norm_ + AdamW (deepsvg/train.py:92-106), fp32, dropout as in the reference's train mode"""
    from oracle import svg_transformer_oracle as O
    from deepsvg_amd.synthetic import make_batch
    commands, args = make_batch(batch, seed=seed)
    commands, args = commands.to(device), args.to(device)
    leaves = {k: v.detach().clone().to(device).requires_grad_(torch.is_floating_point(v)) for k, v in sd.items()}
    params = [v for v in leaves.values() if v.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3)

    def one():
        O.TRAIN_DROPOUT = float(dropout)
        try:
            opt.zero_grad()
            out = O.forward(leaves, cfg, commands, args, commands, args)
            ld = O.svg_loss(cfg, out, O.DEFAULT_WEIGHTS)
            ld["loss"].backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        finally:
            O.TRAIN_DROPOUT = 0.0
        return ld["loss"]

    return one


def _cpu_leg(cfg, sd, batch, threads, box, dropout, max_steps=40):
    """-> (icons/s, threads used, steps timed, s/step) on a bounded sample: at most `box` seconds of CPU work"""
    torch.set_num_threads(max(1, threads))
    one = _oracle_step_fn(cfg, sd, batch, torch.device("cpu"), dropout)
    t0 = time.perf_counter()
    one()                               # warm-up (also the fallback sample when the host is very slow)
    first = time.perf_counter() - t0
    done, t0 = 0, time.perf_counter()
    while done < max_steps and (time.perf_counter() - t0) + first < box:
        one()
        done += 1
    dt = (time.perf_counter() - t0) / done if done else first
    return batch / dt, torch.get_num_threads(), max(done, 1), dt


def cpu_baseline(cfg, sd, batch, dropout):
    """The reference's CPU path beside the GPU number, as the oracle port (kind "port": the reference
    itself is not on the GPU box), dropout ON: (ii) a direct step loop at batch 60, the reference's per-GPU default, on 16
    threads and - in a child process with a hard time limit, because PyTorch's small CPU ops crawl when every core of a
    256-core host joins each parallel region - on 64 threads; (i) BASELINE configs[0]: batch 2, 16 threads.  `value` /
    `cores` = the best batch-60 leg that finished."""
    import subprocess
    ncores = os.cpu_count() or 1
    t16 = min(ncores, int(os.environ.get("DSVG_CPU_THREADS", "16")))
    v16, c16, n16, dt16 = _cpu_leg(cfg, sd, batch, t16, 10.0, dropout)
    legs = {str(c16): {"value": round(v16, 2), "steps": n16, "ms_per_step": round(dt16 * 1e3, 1)}}
    best = (v16, c16, n16, dt16)
    more = min(ncores, 64)
    if more > c16:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-leg", str(more), "--cpu-batch", str(batch),
                                "--dropout", str(dropout)], capture_output=True, text=True, timeout=30)
            leg = json.loads(r.stdout.strip().splitlines()[-1])
            legs[str(more)] = leg
            if leg.get("value") and leg["value"] > best[0]:
                best = (leg["value"], leg["cores"], leg["steps"], leg["ms_per_step"] / 1e3)
        except Exception as e:      # TimeoutExpired: not one step in the time box
            legs[str(more)] = {"value": None, "note": f"did not finish in 30 s ({type(e).__name__})"}
    v2, c2, n2, dt2 = _cpu_leg(cfg, sd, 2, t16, 4.0, dropout)
    ref_c1 = None       # the same configuration through the reference's own train.py, measured where the reference is mounted
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r03_cpu_c1_reference_train.log")) as f:
            for line in f:
                if line.startswith("{"):
                    ref_c1 = json.loads(line)
                    ref_c1["source"] = ("committed: profiles/r03_cpu_c1_reference_train.log (scripts/cpu_c1_reference_train.py in "
                                        "the build container; the port on that host and batch: 195.9 ms/step)")
    except Exception:
        pass
    # kind "reference" would need the reference's own deepsvg package on this host: it is mounted in the build container only
    # (the bench may not read /root/reference at run time, and no copy of its sources travels); the port is bit-identical to it
    # (tests/golden/make_golden.py: logits, losses and gradients of the real reference == the port's, distance 0)
    have_ref = os.path.isdir("/root/reference/deepsvg")
    return {"value": round(best[0], 2), "unit": "icons/s", "cores": best[1], "host_cores": ncores, "kind": "port",
            "note": ("kind is 'port': the unmodified reference is not on this host (" +
                     ("/root/reference exists here but the bench contract forbids reading it at run time" if have_ref
                      else "/root/reference does not exist on the GPU box") +
                     "); the port is pinned bit-for-bit to the reference by the golden fixtures, and the reference's own "
                     "train.py at BASELINE configs[0] was timed in the build container: c1_batch2.reference_train_py"),
            "dropout": dropout, "by_threads": legs,
            "c1_batch2": {"value": round(v2, 2), "unit": "icons/s", "cores": c2, "steps": n2,
                          "ms_per_step": round(dt2 * 1e3, 1),
                          "reference_train_py": ref_c1,
                          "note": "BASELINE configs[0] (batch 2): direct step loop of the port on this host; "
                                  "reference_train_py = the unmodified deepsvg/train.py on the build container's cores "
                                  "(/root/reference does not exist on the GPU box)"},
            "sample": f"{best[2]} train step(s) of batch {batch} (fwd+SVGLoss+bwd+clip+AdamW, dropout {dropout}, fp32, "
                      f"oracle/svg_transformer_oracle.py = stock PyTorch CPU ops), {best[3] * 1e3:.0f} ms/step on "
                      f"{best[1]} threads"}


def cpu_leg_main(threads, batch, dropout):
    """child process of cpu_baseline: one leg on `threads` threads, prints one JSON line"""
    import deepsvg_amd
    from deepsvg_amd.synthetic import det_state_dict
    cfg = deepsvg_amd.HierarchicalOrdered()
    sd = det_state_dict(deepsvg_amd.SVGTransformer(cfg), seed=42)
    v, c, n, dt = _cpu_leg(cfg, sd, batch, threads, 10.0, dropout)
    print(json.dumps({"value": round(v, 2), "cores": c, "steps": n, "ms_per_step": round(dt * 1e3, 1)}), flush=True)


def torch_rocm_reference(cfg, sd, batch, device, dropout, steps=5):
    """SURVEY.md 8(d), last line: the reference's step through stock torch-ROCm fp32 on the same MI355X and the same
    batch size - the oracle module on the device, i.e. aten / rocBLAS / MIOpen kernels, eager launches, dropout on"""
    one = _oracle_step_fn(cfg, sd, batch, device, dropout, seed=1000)
    for _ in range(2):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"ms_per_step": round(dt * 1e3, 2), "icons_per_s": round(batch / dt, 1), "steps": steps, "batch": batch,
            "dtype": "fp32", "dropout": dropout, "loss": round(float(loss), 4),
            "what": "oracle/svg_transformer_oracle.py (line-by-line restatement of the reference model + SVGLoss, pinned to "
                    "it by tests/golden) with torch.optim.AdamW and clip_grad_norm_, stock aten kernels on this GPU"}


def kernel_source_hash(path):
    """SHA-256 (16 hex digits) of a kernel source with comments and whitespace removed: what a committed PMC measurement names
    as the code it was taken on (an edited comment does not make it stale, an edited kernel does)"""
    import hashlib
    import re
    t = open(path).read()
    t = re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    t = re.sub(r"//[^\n]*", "", t)
    t = re.sub(r"\s+", " ", t)
    return hashlib.sha256(t.encode()).hexdigest()[:16]


def dense_layout_leg(cfg, sd_cpu, batches, device, steps=5):
    """the same train step with every exact work-skipping layout switched OFF (padded encoder rows, all 8 groups of the
    second decoder stage forward and backward, dense argument head): the like-for-like number against the reference's padded
    work (`torch_rocm_reference` does exactly that work), hipGraph replay, same batches"""
    import deepsvg_amd
    from deepsvg_amd.trainer import TrainStep
    m = deepsvg_amd.SVGTransformer(cfg)
    m.load_state_dict(sd_cpu)
    m.to(device).set_compute_dtype(torch.bfloat16)
    m.pack_encoder = False
    m.skip_invisible_backward = False
    m.skip_invisible_forward = False
    m.compact_head_backward = False
    m.train()
    ts = TrainStep(m, deepsvg_amd.SVGLoss(cfg).to(device), lr=1e-3, grad_clip=1.0, use_graph=True)
    ts.inputs_resident = True
    nb = min(len(batches), 4)
    for i in range(nb + 2):
        ts.step(*batches[i % nb])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ld = ts.step(*batches[i % nb])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    n = batches[0][0].shape[0]
    return {"ms_per_step": round(dt * 1e3, 3), "icons_per_s": round(n / dt, 1), "steps": steps, "loss": round(float(ld["loss"]), 4),
            "switches": "pack_encoder=0 skip_invisible_backward=0 skip_invisible_forward=0 compact_head_backward=0 "
                        "(= DSVG_PACK_ENCODER=0 DSVG_SKIP_INVISIBLE=0 DSVG_SKIP_INVISIBLE_FWD=0 DSVG_COMPACT_HEAD=0)",
            "what": "every row of the reference's padded (N, G, S) layout is computed, forward and backward"}


def ddp_one_rank_leg(cfg, sd_cpu, batches, device, a, use_graph, steps=20):
    """TrainStep's data-parallel path over a one-rank RCCL process group on this GPU: ms/step and the exposed time of the
    gradient all-reduce (HIP events, deepsvg_amd/trainer.py `time_allreduce`)"""
    import socket
    import deepsvg_amd
    from deepsvg_amd.trainer import TrainStep
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    import datetime
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=device,
                            timeout=datetime.timedelta(seconds=90))       # (a leg of the default run must never hang it)
    try:
        m = deepsvg_amd.SVGTransformer(cfg)
        m.load_state_dict(sd_cpu)
        m.to(device).set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
        m.pack_encoder = bool(a.pack_encoder)
        m.train()
        t = TrainStep(m, deepsvg_amd.SVGLoss(cfg).to(device), lr=1e-3, grad_clip=1.0, use_graph=use_graph, force_ddp=True)
        t.inputs_resident = True
        t.time_allreduce = True
        n_b = len(batches)
        for k in range(n_b):
            t.step(*batches[k])
        for i in range(3):
            t.step(*batches[i % n_b])
        torch.cuda.synchronize()
        t.allreduce_events.clear()
        t0 = time.perf_counter()
        for i in range(steps):
            t.step(*batches[(3 + i) % n_b])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        evs = t.allreduce_events[-steps:]
        ar = sum(e0.elapsed_time(e1) for e0, e1 in evs) / max(len(evs), 1)
        return {"ranks": t.rccl_ranks(), "allreduce_ms": round(ar, 4), "ms_per_step": round(dt * 1e3, 3), "steps": steps,
                "gradient_bytes": int(m.store.grad_buffer(0).numel()) * (2 if t.allreduce_bf16 else 4),
                "launch": "hipGraph replay, collectives outside the graph" if use_graph else "eager, overlapped decoder bucket",
                "measured_on": "one-rank RCCL group on this GPU (the data-parallel code path of an N-GPU rank, without the wire); "
                               "allreduce_ms = HIP events around the gradient all-reduce, mean of the timed steps"}
    finally:
        dist.destroy_process_group()


def secondary_legs(device):
    """BASELINE configs[3] and [4] as short legs (scripts/secondary_bench.py has the long form): C4 one-stage train step
    (OneStageOneShot, max_total_len 50, 512 icons), C5 decode-only of 8192 latents - one-shot arg-max (hierarchical_ordered)
    and autoregressive command sampling over the q|k|v cache (Sketchformer, max_total_len 50)"""
    import deepsvg_amd
    from deepsvg_amd import config as C
    from deepsvg_amd.synthetic import make_batch_onestage, det_state_dict
    from deepsvg_amd.trainer import TrainStep

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    def model_for(cfg):
        m = deepsvg_amd.SVGTransformer(cfg)
        m.load_state_dict(det_state_dict(m, seed=1))
        return m.to(device).set_compute_dtype(torch.bfloat16)
    out = {}
    cfg = C.OneStageOneShot()
    cfg.max_total_len = 50
    cfg.use_vae = False
    m = model_for(cfg).train()
    c, a = make_batch_onestage(512, total_len=50, seed=1)
    c, a = c.to(device), a.to(device)
    ts = TrainStep(m, deepsvg_amd.SVGLoss(cfg).to(device), lr=1e-3, use_graph=True)
    for _ in range(4):
        ts.step(c, a)
    sec = timed(lambda: ts.step(c, a), 20)
    # algorithmic FLOPs of the step in the dense (padded) layout, forward x 3 (backward = input + weight gradients): per token-layer
    # in_proj 3 d^2 + out_proj d^2 + FFN 2 d ff (MACs x 2) + scores / context 2 S d; encoder on 512 x 52 rows, decoder on
    # 512 x 51 rows + the heads (d x (n_args x args_dim + n_commands) per decoder token).  The step skips padding exactly
    # (packed encoder, loss-carrying head rows), so the EXECUTED FLOPs are fewer: this fraction is an upper bound
    d4, ff4 = cfg.d_model, cfg.dim_feedforward
    S_e, S_d = cfg.max_total_len + 2, cfg.max_total_len + 1
    ptl4 = 2.0 * (4 * d4 * d4 + 2 * d4 * ff4)
    fwd4 = (cfg.n_layers * 512 * S_e * (ptl4 + 2.0 * 2 * S_e * d4) + cfg.n_layers_decode * 512 * S_d * (ptl4 + 2.0 * 2 * S_d * d4)
            + 512 * S_d * 2.0 * d4 * (cfg.n_args * (cfg.args_dim + 1) + cfg.n_commands))
    flop_c4 = 3.0 * fwd4
    out["c4_one_stage_train"] = {"ms_per_step": round(sec * 1e3, 3), "icons_per_s": round(512 / sec, 1),
                                 "roofline": {"bound": "mfma", "algorithmic_TFLOP_dense_layout": round(flop_c4 / 1e12, 3),
                                              "achieved_TFLOPs": round(flop_c4 / sec / 1e12, 1), "peak_TFLOPs": 2500.0,
                                              "frac": round(flop_c4 / sec / 2.5e15, 4),
                                              "note": "dense-layout FLOPs / measured time: an upper bound of the executed fraction "
                                                      "(padding is skipped exactly); 26,624 + 26,112 rows are one round of 104 "
                                                      "256-row workgroups: launch-latency-bound, not MFMA-bound"},
                                 "workload": "OneStageOneShot max_total_len=50, 512 icons x 52 tokens, bf16, hipGraph"}
    del ts, m
    cfg = C.HierarchicalOrdered()
    m = model_for(cfg).eval()
    z = (torch.randn(8192, 1, 1, cfg.dim_z, generator=torch.Generator().manual_seed(0)) * 0.3).to(device)
    sec = timed(lambda: m.greedy_sample(z=z, concat_groups=False, temperature=0), 3)
    # algorithmic FLOPs of the one-shot decode (MACs x 2): group decoder on 8192 x 8 rows, path decoder on 8192 x 8 x S rows -
    # per token-layer in_proj 3 d^2 + scores / context 2 S d + out_proj d^2 + FFN 2 d ff - plus the heads (d x (n_args x args_dim
    # + n_commands)); the fused head never stores its logits, so its FLOPs are all the traffic it has
    d_, ff_, S_ = cfg.d_model, cfg.dim_feedforward, cfg.max_seq_len + 1
    per_tok_layer = 2.0 * (4 * d_ * d_ + 2 * d_ * ff_)
    rows2, rows1 = 8192 * cfg.max_num_groups * S_, 8192 * cfg.max_num_groups
    flop_c5 = (cfg.n_layers_decode * (rows2 * (per_tok_layer + 2.0 * 2 * S_ * d_) + rows1 * (per_tok_layer + 2.0 * 2 * cfg.max_num_groups * d_))
               + rows2 * 2.0 * d_ * (cfg.n_args * (cfg.args_dim + 1) + cfg.n_commands))
    def c5_roof(sec_):
        return {"bound": "mfma", "algorithmic_TFLOP": round(flop_c5 / 1e12, 2), "achieved_TFLOPs": round(flop_c5 / sec_ / 1e12, 1),
                "peak_TFLOPs": 2500.0, "frac": round(flop_c5 / sec_ / 2.5e15, 4)}
    out["c5_one_shot_decode"] = {"ms": round(sec * 1e3, 2), "icons_per_s": round(8192 / sec, 1), "roofline": c5_roof(sec),
                                 "workload": "hierarchical_ordered greedy_sample from 8192 latents, temperature 0 (head + arg-max fused)"}
    # the reference's default temperature (1e-4, deepsvg/model/model.py:414): the categorical draw as a Gumbel arg-max fused
    # into the argument head - the 8192 x 8 x 30 x 11 x 257 logits (23 GB in fp32) are never built
    sec = timed(lambda: m.greedy_sample(z=z, concat_groups=False), 3)
    out["c5_one_shot_decode_default_temperature"] = {
        "ms": round(sec * 1e3, 2), "icons_per_s": round(8192 / sec, 1), "roofline": c5_roof(sec),
        "workload": "the same at temperature 1e-4 (reference default): categorical draw on the device (head + Gumbel arg-max fused)"}
    del m
    cfg = C.Sketchformer()
    cfg.max_total_len = 50
    cfg.use_vae = False
    m = model_for(cfg).eval()
    z = torch.randn(8192, 1, 1, cfg.dim_z, generator=torch.Generator().manual_seed(1)).to(device)
    sec = timed(lambda: m.greedy_sample(z=z, concat_groups=False), 2)
    out["c5_autoregressive_decode"] = {"ms": round(sec * 1e3, 1), "icons_per_s": round(8192 / sec, 1),
                                       "tokens_per_s": round(8192 * 50 / sec, 1),
                                       "workload": "Sketchformer max_total_len=50, 8192 icons x 50 tokens, batched sampling over the q|k|v cache"}
    del m
    torch.cuda.empty_cache()
    return out


class SclkSampler:
    """sysfs sclk of this GPU (hwmon freq1_input), sampled every 5 ms by a thread while the timed loop runs.  What it reports
    is the power-management TARGET clock; the clock the waves of a kernel actually see is lower under full-chip load (see
    `in_kernel_clock_probe`: s_memtime ticks per s_memrealtime microsecond inside ffn_fwd)."""

    def __init__(self, index):
        import glob
        import threading
        # the drm card of torch's device `index`, by PCI address; every GPU's file otherwise (then the one whose clock MOVES most
        # is reported: an idle neighbour sits at a constant clock)
        self.paths = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input"))
        try:
            pr = torch.cuda.get_device_properties(index)
            addr = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}."
            mine = [p for p in self.paths if addr in os.path.realpath(p.split("/hwmon/")[0])]
            if mine:
                self.paths = mine[:1]
        except Exception:       # noqa: BLE001  (older torch: no PCI fields)
            pass
        self.samples, self.stop = {p: [] for p in self.paths}, False
        self.thread = threading.Thread(target=self._run, daemon=True) if self.paths else None

    def _run(self):
        while not self.stop:
            for p in self.paths:
                try:
                    self.samples[p].append(float(open(p).read()) / 1e6)
                except (OSError, ValueError):
                    pass
            time.sleep(0.005)

    def __enter__(self):
        if self.thread:
            self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        if self.thread:
            self.thread.join(timeout=1.0)

    def summary(self):
        best = None
        for p, vals in self.samples.items():
            v = sorted(vals)
            if v and (best is None or (v[-1] - v[0]) > (best[1][-1] - best[1][0])):
                best = (p, v)
        if best is None:
            return None
        p, v = best
        return {"source": p, "gpus_sampled": len(self.paths), "samples": len(v), "min_mhz": round(v[0]),
                "median_mhz": round(v[len(v) // 2]), "max_mhz": round(v[-1])}


def in_kernel_clock_probe(rows, device):
    """shader clock INSIDE ffn_fwd's training variant at the step's largest launch: one launch stamped with s_memtime (shader
    cycles) and one with s_memrealtime (the constant 100 MHz counter) at wave start, LayerNorm done, chunk loop done, stores
    issued (development hook dsvg_ffn_debug_clock); ticks / microseconds per phase = the clock the waves ran at.  The chip
    clocks to its power budget: 2.4 GHz with a few workgroups, 1.45-1.65 GHz in the chunk loop with all 256 CUs busy
    (profiles/r04_ffn_timeline_probe.log)."""
    from deepsvg_amd import ops, lib
    g = torch.Generator(device="cpu").manual_seed(0)
    flat = torch.zeros(8 + 131072 + 512 + 131072 + 256 + 256 + 8)
    o = 8
    offs = [[o, o + 131072, o + 131072 + 512, o + 262144 + 512, o + 262144 + 768]]
    flat[o:o + 131072] = torch.randn(131072, generator=g) * 0.06
    flat[o + 131072 + 512:o + 262144 + 512] = torch.randn(131072, generator=g) * 0.06
    flat[o + 262144 + 512:o + 262144 + 768] = 1.0
    flat = flat.to(device)
    pf, _pb, b1f = ops.ffn_pack(flat, torch.tensor(offs, dtype=torch.int64, device=device), 1)
    pl = pf[:ops.FFN_FWD_LAYER_ELEMS]
    b2 = torch.zeros(256, device=device)
    seed = torch.tensor([1234567], dtype=torch.int64, device=device)
    x = torch.randn(rows, 256, generator=g).to(device).to(torch.bfloat16)
    nwg = (rows + 255) // 256
    L = lib.load()
    run = lambda: ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, 0.1, 3, 4, seed, train=True, stages=4)
    for _ in range(20):
        run()
    ph = {}
    for mode in (1, 0):
        buf = torch.zeros(nwg * 8 * 4, dtype=torch.int64, device=device)
        lib.check(L.dsvg_ffn_debug_clock(buf.data_ptr() | mode), "dsvg_ffn_debug_clock")
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        lib.check(L.dsvg_ffn_debug_clock(None), "dsvg_ffn_debug_clock")
        t = buf.view(nwg * 8, 4).double().cpu()
        t = t[(t > 0).all(1)]
        ph[mode] = torch.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 3] - t[:, 2], t[:, 3] - t[:, 0]], -1).median(0).values
    us = ph[1] * 0.01          # 100 MHz ticks -> microseconds
    mhz = [float(ph[0][i] / max(us[i].item(), 1e-9)) for i in range(4)]
    return {"kernel": "ffn_fwd_kernel<4, true>", "rows": rows, "workgroups": nwg,
            "wave_life_us": round(us[3].item(), 1), "prologue_us": round(us[0].item(), 1), "chunk_loop_us": round(us[1].item(), 1),
            "epilogue_us": round(us[2].item(), 1),
            "shader_clock_mhz": {"prologue": round(mhz[0]), "chunk_loop": round(mhz[1]), "epilogue": round(mhz[2]),
                                 "whole_wave": round(mhz[3])},
            "cycles_per_chunk": round(float(ph[0][1]) / 16),
            "method": "s_memtime ticks / s_memrealtime (100 MHz) microseconds, median over the launch's waves"}


def replay_ffn(specs, n, device):
    """the FFN GEMM launches of one step, again, on random operands of the recorded shapes (PMC pass only)"""
    from deepsvg_amd import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    seed = torch.tensor([1234], dtype=torch.int64, device=device)
    calls = []
    for sp in specs:
        dt = torch.bfloat16 if "bfloat16" in sp["dtype"] else torch.float32
        A = (torch.randn(sp["a"], generator=g) * 0.5).to(device).to(dt)
        B = (torch.randn(sp["b"], generator=g) * 0.1).to(device).to(dt)
        M = sp["a"][0] if sp["a_kc"] else sp["a"][1]
        N = sp["b"][0] if sp["b_kc"] else sp["b"][1]
        kw = dict(a_kc=sp["a_kc"], b_kc=sp["b_kc"], act=sp["act"], drop_p=sp["drop_p"], drop_site=3, seed=seed,
                  split_k=sp["split_k"])
        if sp["bias"]:
            kw["bias"] = torch.randn(N, device=device)
        if sp["res"]:
            kw["res"] = (torch.randn(M, N, generator=g) * 0.5).to(device).to(dt)
        if sp["gate"]:
            kw["gate"] = (torch.randn(M, N, generator=g)).to(device).to(dt)
            kw["gate_scale"] = sp["gate_scale"]
        if sp["split_k"] > 1:
            flat = torch.empty(M * N + M, device=device, dtype=torch.float32)
            kw["out"] = flat[:M * N].view(M, N)
            if sp["rowsum"]:
                kw["rowsum"] = flat[M * N:]
        elif sp["out_f32"]:
            kw["out_dtype"] = torch.float32
        calls.append((A, B, kw))
    torch.cuda.synchronize()
    for _ in range(n):
        for A, B, kw in calls:
            ops.gemm(A, B, **kw)
    torch.cuda.synchronize()
    log(f"replayed {len(calls)} FFN launches x {n}")


def self_launch(n):
    """re-run this script under torch.distributed.run with n ranks on this node; returns the launcher's exit code"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on these hosts (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log(f"--gpus {n} without WORLD_SIZE: launching {n} ranks: {' '.join(cmd)}")
    return subprocess.run(cmd, env=env).returncode


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


DUMP_PARAM_SAMPLE = 1 << 21     # parameters in the --dump-outputs sample: the whole fp32 image is 41 MB, the gradient beside it


def dump_outputs(out_dir, ld, model):
    """--dump-outputs DIR: what the timed path computed in its LAST step, as float32 .npy files (~50 MB in all) - the loss dict
    TrainStep.step returned (<key>.npy), the flat gradient of that step (grad.npy, padding slots included) and the parameters
    after its AdamW update at a fixed, seeded sample of positions of the flat fp32 buffer (params_sample.npy)"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    out = {k: v.detach().float().reshape(-1).cpu().numpy() for k, v in ld.items()}
    store = model.store
    if store.flat is not None:
        out["grad"] = store.grad_buffer(0).detach().float().cpu().numpy()
        flat = store.flat.detach().float().cpu().numpy()
        n = min(DUMP_PARAM_SAMPLE, flat.size)
        idx = np.sort(np.random.default_rng(20240611).choice(flat.size, size=n, replace=False))
        out["params_sample"] = flat[idx]
    for name, arr in out.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(arr, dtype=np.float32))
    log(f"outputs of the last timed step -> {out_dir}: " + ", ".join(f"{k} {v.size}" for k, v in out.items()))


def main():
    a = parse()
    if a.cpu_leg > 0:
        cpu_leg_main(a.cpu_leg, a.cpu_batch, a.dropout)
        return
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, rendezvous on
        # 127.0.0.1) - the same command line the driver's torchrun form runs, so both forms report the same line
        # (replaces the single-process nn.DataParallel of /root/reference/deepsvg/train.py:74)
        sys.exit(self_launch(a.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # DSVG_BENCH_EMULATE=1: CPU dry run of THIS script's launch / timing / reporting logic under torch.distributed.run
    # with the gloo backend and the plain-torch restatements of the ops (tests/test_bench_ddp_cpu.py): it proves the
    # multi-process path is launchable where no multi-GPU node is available; it measures nothing
    emulate = os.environ.get("DSVG_BENCH_EMULATE") == "1"
    if emulate:
        from tests.conftest import install_emulated_ops
        install_emulated_ops()
        device = torch.device("cpu")
        if world > 1:
            dist.init_process_group("gloo")
    else:
        assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        if world > 1 or (os.environ.get("DSVG_FORCE_DDP") == "1" and "MASTER_ADDR" in os.environ):
            dist.init_process_group("nccl", device_id=device)
    assert world == a.gpus or world == 1, f"--gpus {a.gpus} but WORLD_SIZE={world}"

    def sync():
        if not emulate:
            torch.cuda.synchronize()

    import deepsvg_amd
    from deepsvg_amd import lib, ops
    from deepsvg_amd.synthetic import make_batch, det_state_dict
    from deepsvg_amd.trainer import TrainStep
    if not emulate:
        lib.load()   # no fallback: fail loudly when the HIP extension is missing

    torch.manual_seed(42)                                   # deepsvg/train.py:15
    cfg = deepsvg_amd.HierarchicalOrdered()
    cfg.dropout = a.dropout
    model = deepsvg_amd.SVGTransformer(cfg)
    sd_cpu = det_state_dict(model, seed=42)                 # same weights on every rank (and for the CPU leg)
    model.load_state_dict(sd_cpu)
    torch.manual_seed(42 + rank)                            # per-rank dropout streams (weights are already fixed)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    model.to(device).set_compute_dtype(dtype)
    model.pack_encoder = bool(a.pack_encoder)
    model.train()
    loss_fn = deepsvg_amd.SVGLoss(cfg).to(device)
    # distinct device-resident batches, rotated through warm-up and the timed loop: their packed-row / visible-sequence /
    # loss-row counts differ, so the loop also pays the per-step layout plan on changing data and the switches between
    # the hipGraphs of different layout buckets
    n_b = max(1, a.batches)
    batches = []
    for k in range(n_b):
        c_k, a_k = make_batch(a.batch, G=8, S=30, seed=1000 + rank + 97 * k)
        batches.append((c_k.to(device), a_k.to(device)))
    commands, args = batches[0]

    log(f"model on {device}, dtype={a.dtype}, batch={a.batch}, world={world}, {n_b} batches")
    # N > 1: the hipGraph holds forward + backward only; the loss-count all-reduce runs before it, the gradient all-reduce
    # and clip + AdamW eagerly behind it (TrainStep.step) - no collective is captured.  DSVG_BENCH_GRAPH_DDP=0: eager
    graph_ok = (world == 1 or os.environ.get("DSVG_BENCH_GRAPH_DDP", "1") != "0") and not emulate
    use_graph = a.graph != 0 and graph_ok
    # DSVG_FORCE_DDP=1 under a one-rank launch: the data-parallel path (RCCL collectives included) on a single GPU
    force_ddp = os.environ.get("DSVG_FORCE_DDP") == "1" and dist.is_available() and dist.is_initialized()
    ts = TrainStep(model, loss_fn, lr=1e-3 * world, grad_clip=1.0, use_graph=use_graph, force_ddp=force_ddp)
    ts.inputs_resident = True       # the synthetic batches sit in HBM before the timed region (bench contract)
    ts.time_allreduce = not emulate
    try:
        ts.step(commands, args)
    except Exception as e:          # graph capture can fail (e.g. collective not capturable): fall back to eager
        if not use_graph:
            raise
        if rank == 0:
            print(f"[bench] hipGraph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
        use_graph = False
        model = deepsvg_amd.SVGTransformer(cfg)
        model.load_state_dict(sd_cpu)
        model.to(device).set_compute_dtype(dtype)
        model.pack_encoder = bool(a.pack_encoder)
        model.train()
        ts = TrainStep(model, loss_fn, lr=1e-3 * world, grad_clip=1.0, use_graph=False)
        ts.step(commands, args)
    rccl_ranks = ts.rccl_ranks() if not emulate or world > 1 else 1

    sync()
    # set-up pass (untimed, before the W warm-up steps): every batch once, so that the hipGraph of every layout bucket the
    # rotation visits exists before the timed region (a capture is a one-off ~0.3 s per bucket in a training run)
    for k in range(1, n_b):
        ts.step(*batches[k])
    sync()
    log(f"set-up pass done (graph={use_graph}, {ts.graphs_captured} graph(s) for {n_b} batches); warmup {a.warmup}")
    if a.graph < 0 and use_graph:
        # launch-mode calibration inside the (untimed) warm-up: same TrainStep, same state, both launch paths
        t_mode = {}
        for mode in (True, False):
            ts.use_graph = mode
            ts.step(commands, args)
            sync()
            t1 = time.perf_counter()
            for i in range(max(a.warmup, 3)):
                ts.step(*batches[i % n_b])
            sync()
            t_mode[mode] = (time.perf_counter() - t1) / max(a.warmup, 3)
        if world > 1:       # every rank must take the same decision: compare the slowest rank's times
            tm = torch.tensor([t_mode[True], t_mode[False]], device=device, dtype=torch.float64)
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
            t_mode = {True: tm[0].item(), False: tm[1].item()}
        use_graph = t_mode[True] <= t_mode[False]
        ts.use_graph = use_graph
        log(f"calibration: graph {t_mode[True] * 1e3:.3f} ms/step, eager {t_mode[False] * 1e3:.3f} ms/step")
    for i in range(a.warmup):
        ts.step(*batches[i % n_b])
    if world > 1:
        dist.barrier()
    sync()
    captured_before = ts.graphs_captured
    keys_seen, switches, last_key = set(), 0, None
    sclk = SclkSampler(local_rank) if (rank == 0 and a.full and not emulate) else None
    if sclk is not None:
        sclk.__enter__()
    t0 = time.perf_counter()
    for i in range(a.steps):
        ld = ts.step(*batches[(a.warmup + i) % n_b])
        if use_graph and ts._graphs:
            k_now = next(reversed(ts._graphs))      # the most recently used bucket = this step's
            keys_seen.add(k_now)
            switches += int(last_key is not None and k_now != last_key)
            last_key = k_now
    sync()
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if sclk is not None:
        sclk.__exit__()
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    loss_val = float(ld["loss"])
    assert loss_val == loss_val and abs(loss_val) < 1e4, f"loss diverged: {loss_val}"
    log(f"timed {a.steps} steps in {elapsed:.3f}s, loss {loss_val:.4f}")
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, ld, model)       # before any leg below runs another step on the same model
    if ts.host_trace:       # DSVG_TRACE_STEP=1: where the host spends a step (ms): plan + its one read, copies + graph launch
        tr = ts.host_trace[-a.steps:]
        plan_ms = sum(t[1] - t[0] for t in tr) / len(tr) * 1e3
        launch_ms = sum(t[2] - t[1] for t in tr) / len(tr) * 1e3
        period_ms = (tr[-1][0] - tr[0][0]) / max(len(tr) - 1, 1) * 1e3
        only_plan_ms = sum(t[3] - t[0] for t in tr) / len(tr) * 1e3 if len(tr[0]) > 3 else float("nan")
        log(f"host trace: plan + read {plan_ms:.3f} ms (of which the layout plan and its read {only_plan_ms:.3f}), copies + graph "
            f"launch {launch_ms:.3f} ms, step period {period_ms:.3f} ms")
    ms_per_step = elapsed / a.steps * 1e3
    icons_per_s = a.batch * world / (elapsed / a.steps)
    graphs = {"launch_mode": "hipGraph replay" if use_graph else "eager", "batches_rotated": n_b,
              "graphs_captured_total": ts.graphs_captured, "graphs_cached": len(ts._graphs),
              "graphs_captured_inside_timed_region": ts.graphs_captured - captured_before,
              "distinct_buckets_in_timed_region": len(keys_seen), "bucket_switches_in_timed_region": switches,
              "graphs_evicted": ts.graphs_evicted, "cache_limit": ts.max_graphs}

    def allreduce_ms(tstep, last_n):
        evs = tstep.allreduce_events[-last_n:]
        return round(sum(e0.elapsed_time(e1) for e0, e1 in evs) / len(evs), 4) if evs else None
    ddp = None
    if ts.ddp and rank == 0:
        ddp = {"ranks": rccl_ranks, "allreduce_ms": allreduce_ms(ts, a.steps) if not emulate else None,
               "gradient_bytes": int(model.store.grad_buffer(0).numel()) * (2 if ts.allreduce_bf16 else 4),
               "measured_on": "this run: HIP events around the gradient all-reduce behind the replayed graph, rank 0, mean of the "
                              "timed steps (exposed time: nothing overlaps it in hipGraph mode)",
               "ms_per_step": round(ms_per_step, 3)}

    roofline = None
    if rank == 0 and a.full and not a.no_roofline and not emulate:
        # Per-launch times of the FFN sub-block, live: HIP events (torch.cuda.Event on the launch stream) around every tagged
        # launch of the SAME launch sequence the timed step replays - same kernels, same order, deferred + batched gradient
        # reductions - issued eagerly behind a short queue of other GPU work, so that the host has enqueued the step before
        # the GPU reaches it and an interval is kernel time, not launch latency.  Events cannot be recorded INSIDE the
        # replayed hipGraph on this runtime (torch: "External events are disallowed in rocm"; hipEventRecordWithFlags(...,
        # hipEventRecordExternal) during a capture breaks the next launch - scripts/graph_event_probe.py): the graph-mode
        # durations of the same kernels come from rocprofv3 --kernel-trace of the timed command, committed under profiles/
        # and cross-checked below (`graph_mode_check`).
        ts_prof = None
        if world == 1:
            ts_prof = TrainStep(model, loss_fn, lr=0.0, grad_clip=1.0, use_graph=False)
            ts_prof.inputs_resident = True
        prof_mode = None
        if ts_prof is not None:
            n_prof = 3
            ts_prof.step(commands, args)
            ops.PROFILE.clear()
            ops.PROFILE_KEEP_DEFER, ops.PROFILE_ON = True, True
            queue = torch.randn(8192, 8192, device=device)
            for _ in range(n_prof):
                sync()
                for _b in range(3):
                    queue @ queue
                ts_prof.step(commands, args)
            sync()
            del queue
            ops.PROFILE_KEEP_DEFER, ops.PROFILE_ON = False, False
            per = len(ops.PROFILE) // n_prof
            recs = []
            for i in range(per):
                rs = [ops.PROFILE[i + j * per] for j in range(n_prof)]
                recs.append((rs[0][0], sum(r[1].elapsed_time(r[2]) for r in rs) / n_prof, rs[0][3], rs[0][4], rs[0][5]))
            ops.PROFILE.clear()
            prof_mode = ("HIP events around the launches of the timed step's sequence (deferred reductions included), "
                         "issued eagerly behind a short queue of other GPU work; mean of 3 steps")
            # recs: (tag, ms, flops, algorithmic bytes, spec) per launch of ONE step
            n_prof = 1
            red = [r for r in recs if r[0] == "reduce"]
            red_ms = sum(r[1] for r in red)
            red_by = {}
            for r in red:
                for k, v in r[4]["by_tag"].items():
                    red_by[k] = red_by.get(k, 0) + v
            red_total = float(sum(red_by.values())) or 1.0
            ffn_red_ms = red_ms * red_by.get("ffn", 0) / red_total
            wg_red_ms = red_ms * (red_by.get("ffn", 0) + red_by.get("wgrad", 0)) / red_total
            # grouped weight-gradient launches of the 4096-row stages: one record per launch, members' FLOPs / bytes by tag
            grp = [r for r in recs if r[0] == "group"]
            grp_ms = sum(r[1] for r in grp)
            grp_ffn_ms = sum(r[1] * r[4]["by_tag"].get("ffn", 0.0) / max(r[2], 1.0) for r in grp)
            grp_ffn_flop = sum(r[4]["by_tag"].get("ffn", 0.0) for r in grp)
            grp_bytes = sum(r[3] for r in grp)

            class _Ms:              # stands in for the (start event, end event) pair of a record: the averaged duration
                def __init__(self, ms):
                    self.ms = ms

                def elapsed_time(self, _other):
                    return self.ms
            allr = [(r[0], _Ms(r[1]), None, r[2], r[3], r[4]) for r in recs]
            ffn = [r for r in allr if r[0] == "ffn"]
            n_ffn = len(ffn)
            # the fused per-layer kernels of the 4096-row group stages contain the FFN sub-block: it is charged with the
            # share of their time that its FLOPs have in the launch (about half: the rest is in_proj / attention / out_proj)
            gsr = [r for r in allr if r[0] == "gs" and r[3] > 0]
            gs_ffn_ms = sum(r[1].elapsed_time(r[2]) * r[5]["ffn_flops"] / r[3] for r in gsr)
            gs_ffn_flop = sum(r[5]["ffn_flops"] for r in gsr)
            # the FFN sub-block's time = its launches + its share (by queued workspace bytes) of the batched reductions
            ffn_ms = sum(r[1].elapsed_time(r[2]) for r in ffn) + ffn_red_ms + gs_ffn_ms + grp_ffn_ms
            n_ffn += len(gsr) + len(grp)
            # algorithmic FLOPs of the FFN sub-block = linear1 + linear2 forward, dX and dW; recomputed or
            # auxiliary launches (dropout replay, reductions, finishing kernel) carry 0 FLOPs but their time counts
            flop_exec = sum(r[3] for r in ffn) / n_prof + gs_ffn_flop + grp_ffn_flop
            flop_padded = a.batch * FFN_FLOP_PER_ICON_TRAIN         # the reference's padded layout
            tf = flop_exec / (ffn_ms * 1e-3) / 1e12
            peak_tf = PEAK_TFLOPS[a.dtype]
            # SURVEY.md 8(d) fused byte count: 512 B in + 512 B out per token-layer forward; the backward pass in the same
            # spirit: dy and x in, dx out (weights and their gradients are O(1) per token)
            fwd_rows = sum(r[5].get("rows", 0) for r in ffn if r[5].get("op") == "ffn_fwd") / n_prof
            unf_fwd_rows = sum(r[5]["a"][0] for r in ffn if r[5].get("act") == 1) / n_prof      # linear1 of an unfused layer
            bwd_rows = sum(r[5].get("rows", 0) for r in ffn if r[5].get("op") in ("ffn_bwd_dx", "ffn_bwd")) / n_prof
            unf_bwd_rows = sum(r[5]["a"][0] for r in ffn if r[5].get("gate")) / n_prof - bwd_rows   # gated dX GEMM: all layers
            # (a stack launch, round 6, carries its rows through `layers` layers)
            gs_fwd_rows = sum(r[5]["rows"] * r[5].get("layers", 1) for r in gsr if r[5]["op"] in ("gs_layer_fwd", "gs_stack_fwd"))
            gs_bwd_rows = sum(r[5]["rows"] * r[5].get("layers", 1) for r in gsr if r[5]["op"] in ("gs_layer_bwd", "gs_stack_bwd"))
            fused_bytes = 1024.0 * (fwd_rows + unf_fwd_rows + gs_fwd_rows) + 1536.0 * (bwd_rows + max(unf_bwd_rows, 0.0) + gs_bwd_rows)
            gbs = fused_bytes / (ffn_ms * 1e-3) / 1e9
            # like-for-like with round 1's definition (matrix launches only: norm2, dropout replay, finishing kernel left out)
            mm_ms = sum(r[1].elapsed_time(r[2]) for r in ffn if r[3] > 0) / n_prof
            fk = [r for r in ffn if r[5].get("op") == "ffn_fwd"]
            fk_ms = sum(r[1].elapsed_time(r[2]) for r in fk) / n_prof
            fk_flop = sum(r[3] for r in fk) / n_prof
            fused_fwd = None
            if fk:
                big = max(r[5]["rows"] for r in fk)
                bigs = [r for r in fk if r[5]["rows"] == big]
                big_us = sum(r[1].elapsed_time(r[2]) for r in bigs) / len(bigs) * 1e3
                fused_fwd = {"kernel": "ffn_fwd_kernel (LayerNorm + linear1 + ReLU + dropout + linear2 + dropout + residual, "
                                       "training variant: also stores h and xh for the backward pass)",
                             "launches_per_step": len(fk) // n_prof, "ms_per_step": round(fk_ms, 3),
                             "achieved_TFLOPs": round(fk_flop / (fk_ms * 1e-3) / 1e12, 1),
                             "frac": round(fk_flop / (fk_ms * 1e-3) / 1e12 / peak_tf, 4),
                             "largest_launch": {"rows": big, "avg_us": round(big_us, 1),
                                                "TFLOPs": round(4.0 * 256 * 512 * big / big_us * 1e-6, 1),
                                                "frac": round(4.0 * 256 * 512 * big / big_us * 1e-6 / peak_tf, 4)}}
            # the second fused kernel of the step: the attention sub-block of the layers with >= 16384 rows (forward)
            ak = [r for r in allr if r[0] == "attn" and r[5].get("op") == "attn_block_fwd"]
            fused_attn = None
            if ak:
                ak_ms = sum(r[1].elapsed_time(r[2]) for r in ak) / n_prof
                ak_flop = sum(r[3] for r in ak) / n_prof
                big = max(r[5]["rows"] for r in ak)
                bigs = [r for r in ak if r[5]["rows"] == big]
                big_us = sum(r[1].elapsed_time(r[2]) for r in bigs) / len(bigs) * 1e3
                big_flop = bigs[0][3]
                fused_attn = {"kernel": "attn_block_fwd_kernel (LayerNorm + in_proj + 8-head attention + out_proj + dropout "
                                        "+ residual, training variant: also stores LN(x), q|k|v and the head outputs)",
                              "launches_per_step": len(ak) // n_prof, "ms_per_step": round(ak_ms, 3),
                              "achieved_TFLOPs": round(ak_flop / (ak_ms * 1e-3) / 1e12, 1),
                              "frac": round(ak_flop / (ak_ms * 1e-3) / 1e12 / peak_tf, 4),
                              "largest_launch": {"rows": big, "avg_us": round(big_us, 1),
                                                 "TFLOPs": round(big_flop / big_us * 1e-6, 1),
                                                 "frac": round(big_flop / big_us * 1e-6 / peak_tf, 4)}}
            # the launches that take the most time in the step are not MFMA-bound: the weight-gradient GEMMs (token-major
            # operands of 0.5-1.5 KB per token read once, a 256 x 256 .. 768 x 256 result) are HBM-bound.  Timed with their
            # share of the batched split-K reductions
            wg = [r for r in allr if len(r[5]) and r[5].get("split_k", 1) > 1 and r[0] in ("wgrad", "ffn")]
            wgrad = None
            if wg:
                wg_ms = sum(r[1].elapsed_time(r[2]) for r in wg) / n_prof + wg_red_ms + grp_ms
                wg_bytes = sum(r[4] for r in wg) / n_prof + grp_bytes
                wgrad = {"kernel": "weight-gradient GEMMs (dW = dY^T X over all tokens, split-K) incl. their reductions",
                         "bound": "hbm", "launches_per_step": len(wg) // n_prof + len(grp), "ms_per_step": round(wg_ms, 3),
                         "algorithmic_GB_per_step": round(wg_bytes / 1e9, 3),
                         "achieved_GBps": round(wg_bytes / (wg_ms * 1e-3) / 1e9, 1), "peak_GBps": 8000.0,
                         "frac": round(wg_bytes / (wg_ms * 1e-3) / 1e9 / 8000.0, 4)}
            roofline = {"bound": "mfma",
                        "kernel": "FFN sub-block of the 16 layers (fused forward kernel / linear1+linear2 GEMMs, dX, dW), "
                                  "%d launches per step" % n_ffn,
                        "achieved": round(tf, 2), "peak": peak_tf, "unit": "TFLOP/s", "frac": round(tf / peak_tf, 4),
                        "traffic": None, "traffic_source": None,
                        "timed_in": prof_mode,
                        "launches_per_step": n_ffn, "ffn_ms_per_step": round(ffn_ms, 3),
                        "batched_reductions": {"ms_per_step": round(red_ms, 3), "ffn_share_ms": round(ffn_red_ms, 3),
                                               "weight_grad_share_ms": round(wg_red_ms, 3)},
                        "avg_launch_us": round(ffn_ms * 1e3 / n_ffn, 2),
                        "executed_gflop_per_step": round(flop_exec / 1e9, 1),
                        "padded_layout_gflop_per_step": round(flop_padded / 1e9, 1),
                        "padding_skipped_frac": round(1.0 - flop_exec / flop_padded, 4),
                        "matrix_launches_only": {"ms_per_step": round(mm_ms, 3),
                                                 "frac": round(flop_exec / (mm_ms * 1e-3) / 1e12 / peak_tf, 4),
                                                 "note": "round 1's accounting: launches that execute FLOPs only"},
                        "group_stage_layers": {"kernel": "gs_stack_fwd / gs_stack_bwd (ONE launch per 4-layer stack and direction for the "
                                                         "4096-row stages) + gs_layer_fwd (the remainder rows of the second decoder "
                                                         "stage, one launch per layer): LN + in_proj + attention + out_proj + LN + FFN",
                                               "launches_per_step": len(gsr),
                                               "layers_per_step": sum(r[5].get("layers", 1) for r in gsr),
                                               "ms_per_step": round(sum(r[1].elapsed_time(r[2]) for r in gsr), 3),
                                               "ffn_share_ms": round(gs_ffn_ms, 3)} if gsr else None,
                        "fused_fwd_kernel": fused_fwd,
                        "fused_attn_fwd_kernel": fused_attn,
                        "weight_grad_gemms": wgrad,
                        "hbm_view": {"achieved_GBps": round(gbs, 1), "peak_GBps": 8000.0, "frac": round(gbs / 8000.0, 4),
                                     "fused_algorithmic_GB_per_step": round(fused_bytes / 1e9, 3),
                                     "definition": "SURVEY.md 8(d) fused byte count: 1024 B per token-layer forward; "
                                                   "1536 B per token-layer backward (dy, x in; dx out)"}}
            # HBM traffic of the dominant kernel, measured by rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (scripts/
            # gpu_step_pmc.sh; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for 16-byte streaming reads on
            # gfx950): a COMMITTED measurement (profiles/ffn_traffic.json), not taken in this run
            tj = os.path.join(ROOT, "profiles", "ffn_traffic.json")
            if os.path.exists(tj):
                t = json.load(open(tj))
                if t.get("dtype") == a.dtype and "MB_per_launch" in t:
                    sha = kernel_source_hash(os.path.join(ROOT, "deepsvg_amd", "csrc", "ffn_fused.hip"))
                    roofline["traffic"] = t["MB_per_launch"]
                    roofline["traffic_source"] = "committed: " + t["source"]
                    roofline["traffic_over_fused_algorithmic"] = t.get("over_fused_algorithmic")
                    # the committed measurement names the commit and the kernel source it was taken on; a kernel edited since
                    # then makes the number stale (tests/test_bench_gpu.py fails on it)
                    roofline["traffic_collected_at"] = {"commit": t.get("commit"), "ffn_fused_hip_code_sha256_16": t.get("ffn_fused_hip_code_sha256_16"),
                                                        "current_ffn_fused_hip_code_sha256_16": sha,
                                                        "kernel_source_unchanged": t.get("ffn_fused_hip_code_sha256_16") == sha}
            gcsv = next((q for q in (os.path.join(ROOT, "profiles", f"r0{r}_graph_kernel_stats.csv") for r in (6, 5, 4, 3))
                         if os.path.exists(q)), "")       # the newest committed trace of the replayed graph
            if os.path.exists(gcsv) and fused_fwd is not None:
                for line in open(gcsv):
                    if "ffn_fwd_kernel" in line:
                        f = line.strip().split(",")
                        roofline["graph_mode_check"] = {
                            "kernel": "ffn_fwd_kernel", "source": "committed: profiles/" + os.path.basename(gcsv) + " (rocprofv3 "
                            "--kernel-trace of `bench.py --graph 1`, scripts/gpu_prof_graph.sh)",
                            "graph_replay_avg_us": float(f[3]), "launches_profiled": int(f[1]),
                            "live_event_avg_us": round(fk_ms * 1e3 / max(len(fk), 1), 1)}
                        break
            if os.path.exists(gcsv) and fused_fwd is not None and wgrad is not None:
                # the same family inside the replayed graph (the leg above times eager launches, each with its launch latency
                # exposed): per-step totals of the committed rocprofv3 trace of `bench.py --graph 1`, the deferred reductions
                # shared out as in the live leg
                tot = {}
                for line in open(gcsv):
                    f = line.strip().split(",")
                    if len(f) > 3 and f[1].isdigit():
                        tot[f[0]] = (int(f[1]), float(f[2]))
                steps_prof = sum(c for k, (c, _) in tot.items() if "ffn_fwd_kernel" in k) / max(fused_fwd["launches_per_step"], 1)
                if steps_prof > 0:
                    g_ms = sum(ms for k, (_, ms) in tot.items()
                               if ("gemm_bf16_glds_kernelILb0ELb0ELi5" in k or "gemm_bf16_wgrad_group_kernel" in k)) / steps_prof
                    g_red = sum(ms for k, (_, ms) in tot.items() if "reduce_deferred_kernel" in k) / steps_prof
                    g_ms += g_red * (wg_red_ms / red_ms if red_ms > 0 else 0.0)
                    wgrad["graph_replay"] = {"ms_per_step": round(g_ms, 3), "achieved_GBps": round(wg_bytes / (g_ms * 1e-3) / 1e9, 1),
                                             "frac": round(wg_bytes / (g_ms * 1e-3) / 1e9 / 8000.0, 4),
                                             "steps_profiled": round(steps_prof, 1),
                                             "source": "committed: profiles/" + os.path.basename(gcsv) + " (split-K products + grouped "
                                                       "launches + their share of reduce_deferred, rocprofv3 --kernel-trace of the "
                                                       "replayed graph)"}
            # HBM traffic of the WHOLE step from the committed per-kernel PMC summary (scripts/gpu_step_pmc.sh: rocprofv3 --pmc
            # FETCH_SIZE / WRITE_SIZE in separate passes over 3 eager steps; FETCH doubled as the micro-architecture guide
            # prescribes for gfx950): sum over kernels of (fetch + write) MB per launch x launches per step
            pcsv = next((q for q in (os.path.join(ROOT, "profiles", f"r0{r}_step_pmc_summary.csv") for r in (6, 5, 4, 3))
                         if os.path.exists(q)), "")
            if os.path.exists(pcsv):
                tot_mb, n_ffn_launches = 0.0, 0
                for line in open(pcsv):
                    f = line.strip().rsplit(",", 8)         # (kernel names contain commas: the 8 numeric columns from the right)
                    if len(f) != 9 or not f[1].isdigit():
                        continue
                    tot_mb += (float(f[3]) + float(f[4])) * int(f[1])
                    if "ffn_fwd_kernel" in f[0]:
                        n_ffn_launches += int(f[1])
                # (`launches` counts every step of the profiled command - set-up pass, warm-up, timed: 8 ffn_fwd launches per step)
                steps_pmc = n_ffn_launches / 8.0
                if steps_pmc > 0:
                    roofline["step_traffic_GB"] = round(tot_mb / steps_pmc / 1e3, 2)
                    roofline["step_traffic_source"] = ("committed: profiles/" + os.path.basename(pcsv) + " (sum over the 60 kernels "
                                                       "with the most time of (fetch x 2 + write) MB per launch x launches, / "
                                                       f"{steps_pmc:.0f} profiled steps; eager launches, scripts/gpu_step_pmc.sh)")
            if a.ffn_replay > 0:
                specs = [r[5] for r in ffn[:n_ffn] if "a" in r[5]]
                replay_ffn(specs, a.ffn_replay, device)

    if a.full:
        log(f"roofline leg done: {roofline}")
    fp32 = None
    if rank == 0 and world == 1 and a.full and a.dtype == "bf16" and not a.no_fp32 and not emulate:
        # the parity path (what the 1e-3 tolerance of the north star is tested on): the same step over the same rotating batches,
        # timed by the same loop as the headline (round 6: hipGraph replay like the bf16 step; eager if a capture fails)
        m32 = deepsvg_amd.SVGTransformer(cfg)
        m32.load_state_dict(sd_cpu)
        m32.to(device).set_compute_dtype(torch.float32)
        m32.pack_encoder = bool(a.pack_encoder)
        m32.train()
        g32 = bool(use_graph)
        t32 = TrainStep(m32, deepsvg_amd.SVGLoss(cfg).to(device), lr=1e-3, grad_clip=1.0, use_graph=g32)
        t32.inputs_resident = True
        try:
            for k in range(n_b):
                ld32 = t32.step(*batches[k])
        except Exception as e:
            if not g32:
                raise
            log(f"fp32 leg: hipGraph capture failed ({type(e).__name__}: {e}); eager")
            g32 = False
            m32 = deepsvg_amd.SVGTransformer(cfg)
            m32.load_state_dict(sd_cpu)
            m32.to(device).set_compute_dtype(torch.float32)
            m32.pack_encoder = bool(a.pack_encoder)
            m32.train()
            t32 = TrainStep(m32, deepsvg_amd.SVGLoss(cfg).to(device), lr=1e-3, grad_clip=1.0, use_graph=False)
            t32.inputs_resident = True
            for k in range(n_b):
                ld32 = t32.step(*batches[k])
        for i in range(3):
            ld32 = t32.step(*batches[i % n_b])
        sync()
        t1 = time.perf_counter()
        n32 = a.steps
        for i in range(n32):
            ld32 = t32.step(*batches[(3 + i) % n_b])
        sync()
        dt32 = (time.perf_counter() - t1) / n32
        fp32 = {"ms_per_step": round(dt32 * 1e3, 3), "icons_per_s": round(a.batch / dt32, 1), "steps": n32,
                "launch": "hipGraph replay" if g32 else "eager", "loss": round(float(ld32["loss"]), 4),
                "note": "fp32 storage, exact-fp32 MFMA (157.3 TFLOP/s peak): the path the 1e-3 parity tests run on"}
        # bf16 storage against this fp32 path on the SAME (trained-for-a-few-steps) weights, evaluation mode, one batch: how
        # far the timed dtype is from the parity dtype on the quantities the north star names
        try:
            mb = deepsvg_amd.SVGTransformer(cfg)
            mb.load_state_dict({k: v.detach().float().cpu() for k, v in m32.state_dict().items()})
            mb.to(device).set_compute_dtype(torch.bfloat16).eval()
            m32.eval()
            with torch.no_grad():
                o32 = m32(commands, args, commands, args, params={})
                o16 = mb(commands, args, commands, args, params={})
            c32, c16 = o32["command_logits"].float(), o16["command_logits"].float()
            fp32["bf16_vs_fp32"] = {"cmd_argmax_agreement": round((c32.argmax(-1) == c16.argmax(-1)).float().mean().item(), 5),
                                    "cmd_logit_max_abs_err": round((c32 - c16).abs().max().item(), 5)}
            del mb, o32, o16
        except Exception as e:      # reported, never fatal for the bench line
            fp32["bf16_vs_fp32"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        del m32, t32
        log(f"fp32 leg done: {fp32}")
    dense = secondary = clock = None
    if rank == 0 and world == 1 and a.full and a.dtype == "bf16" and not a.no_extra_legs and not emulate:
        try:
            dense = dense_layout_leg(cfg, sd_cpu, batches, device)
        except Exception as e:      # reported, never fatal for the bench line
            dense = {"error": f"{type(e).__name__}: {e}"[:300]}
        log(f"dense-layout leg done: {dense}")
        try:
            secondary = secondary_legs(device)
        except Exception as e:
            secondary = {"error": f"{type(e).__name__}: {e}"[:300]}
        log(f"secondary legs done: {secondary}")
        try:
            big = 63488
            if roofline and roofline.get("fused_fwd_kernel"):
                big = int(roofline["fused_fwd_kernel"]["largest_launch"]["rows"])
            clock = in_kernel_clock_probe(big, device)
        except Exception as e:
            clock = {"error": f"{type(e).__name__}: {e}"[:300]}
        log(f"in-kernel clock probe done: {clock}")
        if roofline and clock and "shader_clock_mhz" in clock and roofline.get("fused_fwd_kernel"):
            # the same fractions against the MFMA peak AT THE CLOCK THE KERNEL RAN AT (2.5 PFLOP/s is the peak at 2.4 GHz; the
            # chip clocks to its power budget): what the kernel's schedule leaves on the table, apart from the clock
            mhz = clock["shader_clock_mhz"]["whole_wave"]
            scale = 2400.0 / max(mhz, 1.0)
            ff = roofline["fused_fwd_kernel"]
            ff["frac_at_measured_clock"] = round(ff["largest_launch"]["frac"] * scale, 4)
            ff["measured_clock_mhz"] = mhz
            ff["chunk_loop_frac_at_its_clock"] = round(
                2 * 32 * 32.0 / max(clock["cycles_per_chunk"], 1.0), 4)     # matrix-pipe cycles of a SIMD's two waves (2 x 32 MFMAs x 32) / cycles per chunk
    if ddp is None and rank == 0 and world == 1 and a.full and not a.no_extra_legs and not emulate and not (dist.is_available() and dist.is_initialized()):
        # the data-parallel path on a ONE-rank RCCL group (no multi-GPU lease is available to the builder): the same step with the
        # 3-count loss all-reduce in front of the graph and the 41 MB gradient all-reduce behind it - what a rank of an N-GPU
        # run executes, minus the wire.  `allreduce_ms` = the exposed time of that exchange on one GPU (RCCL's local copy path);
        # on N GPUs add 2 (N - 1) / N x bytes / link bandwidth (ring, xGMI: ~0.1-0.5 ms for 41 MB at N = 8)
        try:
            ddp = ddp_one_rank_leg(cfg, sd_cpu, batches, device, a, use_graph)
        except Exception as e:      # reported, never fatal for the bench line
            ddp = {"error": f"{type(e).__name__}: {e}"[:300]}
        log(f"one-rank RCCL leg done: {ddp}")
    torch_ref = None
    if rank == 0 and world == 1 and a.full and not a.no_torch_ref and not emulate:
        try:
            torch_ref = torch_rocm_reference(cfg, sd_cpu, a.batch, device, a.dropout)
        except Exception as e:          # (e.g. out of memory on a shared box): reported, never fatal for the bench line
            torch_ref = {"error": f"{type(e).__name__}: {e}"[:300]}
        torch.cuda.empty_cache()
        log(f"torch-ROCm reference leg done: {torch_ref}")
    cpu = None
    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline and not emulate:
        cpu = cpu_baseline(cfg, sd_cpu, a.cpu_batch, a.dropout)
        log(f"cpu baseline done: {cpu}")

    if rank == 0:
        rec = {
            "metric": "SVG icons/sec (train step) hierarchical_ordered d=256",
            "value": round(icons_per_s, 1), "unit": "icons/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": "hierarchical_ordered (Hierarchical, use_vae=False) G=8 S=30 d_model=256 ff=512 "
                                   "H=8 L=4x4; full train step = forward + SVGLoss + backward + grad-clip 1.0 + AdamW; "
                                   f"dropout {a.dropout}", "global_batch": a.batch * world, "batch_per_gpu": a.batch,
                       "parallelism": f"dp{world}", "hip_graph": use_graph, "loss": round(loss_val, 4),
                       "encoder_layout": ("packed (valid tokens only, exact)" if model.last_packing else "padded"),
                       "encoder_valid_token_frac": (round(model.last_packing[0] / model.last_packing[1], 4)
                                                    if model.last_packing else 1.0),
                       # every DSVG_* environment switch that was set for this run (A/B knobs, opt-in kernels): a record taken
                       # with a non-default kernel selection says so
                       "env_overrides": {k: v for k, v in sorted(os.environ.items())
                                         if k.startswith("DSVG_") and not k.startswith("DSVG_BENCH_")},
                       # sysfs sclk while the timed loop ran (the power-management target; stationary from the first step on:
                       # profiles/r04_clock_probe.log) and the shader clock measured inside the dominant kernel
                       "clock_mhz": {"sclk_sysfs": (sclk.summary() if sclk is not None else None),
                                     "in_kernel": (clock or {}).get("shader_clock_mhz") if clock else None},
                       # the numbers that must be quoted beside `value` (round 6: short scalar keys the driver's parser keeps):
                       # the parity dtype's throughput, the like-for-like dense layout, bf16's arg-max agreement with fp32
                       "fp32_ms_per_step": (fp32 or {}).get("ms_per_step"),
                       "fp32_icons_per_s": (fp32 or {}).get("icons_per_s"),
                       "fp32_launch": (fp32 or {}).get("launch"),
                       "dense_ms_per_step": (dense or {}).get("ms_per_step") if isinstance(dense, dict) else None,
                       "bf16_cmd_argmax_agreement": ((fp32 or {}).get("bf16_vs_fp32") or {}).get("cmd_argmax_agreement"),
                       "bf16_cmd_logit_max_abs_err": ((fp32 or {}).get("bf16_vs_fp32") or {}).get("cmd_logit_max_abs_err")},
            "graphs": graphs, "rccl_ranks": rccl_ranks, "ddp": ddp,
            "roofline": roofline, "fp32": fp32, "dense_layout": dense, "secondary": secondary, "in_kernel_clock": clock,
            "torch_rocm_reference": torch_ref, "cpu_baseline": cpu,
        }
        print(json.dumps(rec), flush=True)
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
