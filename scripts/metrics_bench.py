"""Micro-timing of the reconstruction-error kernels (csrc/metrics.hip) at batch 512, hierarchical_ordered shapes (G = 8 groups
of S + 2 = 32 tokens), n = 10 points per command:

  ops.sample_points   float32 targets (as the dataset delivers them) and int64 sequences (as greedy_sample returns them)
  ops.chamfer         the clouds of two different seeded batches against each other: `typical` = make_batch (1..8 visible
                      groups, 2..30 commands each), `dense` = every group visible, `full` = every group 30 curves (2,168
                      points in every cloud: the most these shapes give, and equal work in every workgroup)
  the reference's way on the same GPU: a loop over icons of torch.cdist -> min -> mean (deepsvg/difflib/loss.py:5-7 restated)
                      over the kernel's points
  the backward legs   ops.chamfer_nn (next to ops.chamfer: the same sweep with the arg-min kept), ops.chamfer_bwd,
                      ops.sample_points_bwd, one step of metrics.refine's loop (sample_points -> chamfer -> backward -> Adam),
                      and the reference's way again: the per-icon torch.cdist loop with autograd through it
  the ordered loss    (`typical` clouds only) ops.emd, ops.emd_bwd and one step of metrics.refine(loss="emd"), against a
                      per-icon torch loop of the same definition (include/dsvg.h: float64 orientation and arc lengths,
                      searchsorted matching, all n shifts of an icon at once from an [n, n] gather - kinder to torch than the
                      reference's Python loop over the n shifts, deepsvg/difflib/loss.py:39), forward and with autograd

HIP events around `inner` back-to-back calls, median of 20 such runs after warm-up.  The VALU floor quoted for the Chamfer
launch is pairs * 4.5 vector instructions (2 subtractions, multiply, fused multiply-add, half a 3-way minimum: the kernel's inner
loop) over 256 CUs * 4 SIMDs * 32 lanes per clock at 2.4 GHz.  Writes nothing but stdout."""
import os
import socket
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsvg_amd import metrics, ops                 # noqa: E402
from deepsvg_amd.synthetic import make_batch         # noqa: E402

N, G, S, NPTS = 512, 8, 30, 10
RUNS, WARMUP = 20, 5
VALU_LANES_PER_S = 256 * 4 * 32 * 2.4e9


def timed(fn, inner, runs=RUNS, warmup=WARMUP):
    """-> (median, min, max) ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def chamfer_torch_loop(px, nx, py, ny):
    """the reference's way, one icon at a time (counts on the host)"""
    out = []
    for b in range(px.shape[0]):
        d = torch.cdist(px[b, :nx[b]], py[b, :ny[b]])
        out.append(d.min(dim=0).values.mean() + d.min(dim=1).values.mean())
    return torch.stack(out)


def emd_torch_loop(px, nx, py, ny):
    """the ordered loss of include/dsvg.h one icon at a time (counts on the host, both clouds non-empty)"""
    out = []
    for b in range(px.shape[0]):
        n, m = nx[b], ny[b]
        x, y = px[b, :n], py[b, :m].double()
        if not bool((y[:-1, 0] * y[1:, 1] - y[1:, 0] * y[:-1, 1]).sum() > 0):
            y = y.flip(0)
        cum = torch.cat([y.new_zeros(1), (y[1:] - y[:-1]).norm(dim=-1).cumsum(0)])
        if m == 1 or not bool(cum[-1] > 0):
            j = torch.zeros(n, dtype=torch.long, device=px.device)
        else:
            D = cum / cum[-1]
            u = torch.arange(n, dtype=torch.float64, device=px.device) / max(n - 1, 1)
            hi = torch.searchsorted(D, u).clamp(max=m - 1)
            lo = (hi - 1).clamp(min=0)
            j = torch.where((u - D[lo]).abs() <= (D[hi] - u).abs(), lo, hi)
        t = y[j].float()
        k = torch.arange(n, device=px.device)
        S = (x.unsqueeze(0) - t[(k.unsqueeze(0) + k.unsqueeze(1)) % n]).norm(dim=-1).sum(1)          # [shift, point]
        s = int(S.argmin())
        out.append((x - torch.cat([t[s:], t[:s]])).norm(dim=-1).mean())
    return torch.stack(out)


def full_batch(seed):
    """every group: SOS, 30 curves, EOS"""
    commands = torch.full((N, G, S + 2), 2.0)
    commands[:, :, 0], commands[:, :, -1] = 5.0, 4.0
    args = torch.randint(0, 256, (N, G, S + 2, 11), generator=torch.Generator().manual_seed(seed)).float()
    return commands.cuda(), args.cuda()


def main():
    assert torch.cuda.is_available(), "metrics_bench.py measures on a GPU"
    dev = "cuda"
    print(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
    print(f"batch {N}, G = {G}, S + 2 = {S + 2}, n = {NPTS}; median [min .. max] of {RUNS} runs")
    for tag, min_groups in (("typical", 1), ("dense", G), ("full", None)):
        if min_groups is None:
            (ca, aa), (cb, ab) = full_batch(1), full_batch(2)
        else:
            ca, aa = make_batch(N, G=G, S=S, seed=1, device=dev, min_groups=min_groups)
            cb, ab = make_batch(N, G=G, S=S, seed=2, device=dev, min_groups=min_groups)
        flat = lambda c, a: (c.reshape(N * G, S + 2).contiguous(), a.reshape(N * G, S + 2, 11).contiguous())     # noqa: E731
        (c32, a32), (c64, a64) = flat(ca, aa), flat(cb.long(), ab.long())
        in32 = c32.numel() * 4 * 12
        px, nx = ops.sample_points(c32, a32, n=NPTS, groups=G)
        py, ny = ops.sample_points(c64, a64, n=NPTS, groups=G)
        out_b = int(nx.sum()) * 8
        for name, c, a, inb in (("float32", c32, a32, in32), ("int64", c64, a64, 2 * in32)):
            med, lo, hi = timed(lambda: ops.sample_points(c, a, n=NPTS, groups=G), inner=20)
            print(f"[{tag}] sample_points {name}: {med * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  reads {inb / 1e6:.1f} MB, "
                  f"writes ~{out_b / 1e6:.1f} MB of points into a {px.numel() * 4 / 1e6:.1f} MB buffer "
                  f"({(inb + out_b) / med / 1e6:.0f} GB/s)")
        pairs = 2 * int((nx.long() * ny.long()).sum())
        floor_ms = pairs * 4.5 / VALU_LANES_PER_S * 1e3
        med, lo, hi = timed(lambda: ops.chamfer(px, nx, py, ny), inner=10)
        print(f"[{tag}] chamfer: {med * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  points per cloud mean {float(nx.float().mean()):.0f} / "
              f"max {int(nx.max())}, {pairs / 1e9:.2f} G point pairs (both directions), {pairs / med / 1e9:.1f} T pairs/s; "
              f"VALU floor {floor_ms * 1e3:.1f} us = {floor_ms / med * 100:.0f} % of the launch")
        got = ops.chamfer(px, nx, py, ny)
        nxl, nyl = nx.tolist(), ny.tolist()
        want = chamfer_torch_loop(px, nxl, py, nyl)
        med_t, lo_t, hi_t = timed(lambda: chamfer_torch_loop(px, nxl, py, nyl), inner=1, runs=5, warmup=1)
        print(f"[{tag}] torch.cdist loop over {N} icons (5 runs): {med_t:8.2f} ms [{lo_t:.2f} .. {hi_t:.2f}] = {med_t / med:.0f} x the "
              f"kernel; largest matrix {max(a * b for a, b in zip(nxl, nyl)) * 4 / 1e6:.1f} MB, all {N} at once would be "
              f"{sum(a * b for a, b in zip(nxl, nyl)) * 4 / 1e9:.2f} GB; max |kernel - fp32 cdist| {float((got - want).abs().max()):.2e}")
        print(f"[{tag}] mean Chamfer distance of the two batches {float(got.mean()):.4f}")
        # ---- the backward legs ----
        med_nn, lo, hi = timed(lambda: ops.chamfer_nn(px, nx, py, ny), inner=10)
        print(f"[{tag}] chamfer_nn: {med_nn * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {med_nn / med:.2f} x chamfer")
        out_nn, idx_x, idx_y = ops.chamfer_nn(px, nx, py, ny)
        assert torch.equal(out_nn.view(torch.int32), got.view(torch.int32)), "chamfer_nn and chamfer differ in bits"
        dout = torch.ones(N, device=dev)
        med_b, lo, hi = timed(lambda: ops.chamfer_bwd(px, nx, py, ny, idx_x, idx_y, dout), inner=10)
        print(f"[{tag}] chamfer_bwd: {med_b * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {med_b / med:.2f} x chamfer")
        dpx, _ = ops.chamfer_bwd(px, nx, py, ny, idx_x, idx_y, dout)
        med_s, lo, hi = timed(lambda: ops.sample_points_bwd(c32, dpx, n=NPTS, groups=G), inner=20)
        print(f"[{tag}] sample_points_bwd: {med_s * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  reads {dpx.numel() * 4 / 1e6:.1f} MB of "
              f"point gradients, writes {a32.numel() * 4 / 1e6:.1f} MB")
        ref = a32.view(N, G, S + 2, 11).clone().requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=0.1)

        def refine_step():
            opt.zero_grad(set_to_none=True)
            metrics.chamfer_loss(ca, ref, py, ny, NPTS)["loss"].backward()
            opt.step()
        med_r, lo, hi = timed(refine_step, inner=5)
        print(f"[{tag}] one refine step (sample_points, chamfer_nn, chamfer_bwd, sample_points_bwd, masked mean, Adam): "
              f"{med_r * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]")
        grown = []
        for _ in range(2):                              # (second pass: code objects and the allocator's pools are warm)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            o, ix, iy = ops.chamfer_nn(px, nx, py, ny)
            gx, gy = ops.chamfer_bwd(px, nx, py, ny, ix, iy, dout)
            torch.cuda.synchronize()
            grown.append(torch.cuda.max_memory_allocated() - before)
        print(f"[{tag}] chamfer_nn + chamfer_bwd allocate {grown[-1] / 1e6:.2f} MB: indices {(ix.numel() + iy.numel()) * 4 / 1e6:.2f} MB, "
              f"gradients {(gx.numel() + gy.numel()) * 4 / 1e6:.2f} MB, out + workspace the rest")
        pxl = px.clone().requires_grad_(True)

        def torch_loop_backward():
            pxl.grad = None
            chamfer_torch_loop(pxl, nxl, py, nyl).sum().backward()
        med_tb, lo_t, hi_t = timed(torch_loop_backward, inner=1, runs=5, warmup=1)
        torch_loop_backward()
        live = (torch.arange(px.shape[1], device=dev).unsqueeze(0) < nx.unsqueeze(1)).unsqueeze(-1)
        diff = torch.where(live, (pxl.grad - dpx).abs(), torch.zeros_like(dpx))
        print(f"[{tag}] torch.cdist loop, forward + autograd backward (5 runs): {med_tb:8.2f} ms [{lo_t:.2f} .. {hi_t:.2f}] = "
              f"{med_tb / (med_nn + med_b):.0f} x chamfer_nn + chamfer_bwd; max |kernel - fp32 cdist autograd| on d / d points "
              f"{float(diff.max()):.2e}, above 1e-5 in {int((diff > 1e-5).sum())} of {int(live.sum()) * 2} entries")
        if tag != "typical":
            continue
        # ---- the ordered loss ----
        terms = int((nx.long() * nx.long()).sum())
        med_e, lo, hi = timed(lambda: ops.emd(px, nx, py, ny), inner=5)
        print(f"[{tag}] emd: {med_e * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {med_e / med:.2f} x chamfer; {terms / 1e9:.2f} G "
              f"shift terms, {terms / med_e / 1e9:.1f} T terms/s")
        out_e, shift, _, t = ops.emd(px, nx, py, ny)
        med_eb, lo, hi = timed(lambda: ops.emd_bwd(px, nx, ny, t, shift, dout), inner=20)
        print(f"[{tag}] emd_bwd: {med_eb * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]")

        def refine_step_emd():
            opt.zero_grad(set_to_none=True)
            metrics.emd_loss(ca, ref, py, ny, NPTS)["loss"].backward()
            opt.step()
        med_re, lo, hi = timed(refine_step_emd, inner=5)
        print(f"[{tag}] one refine(loss='emd') step (sample_points, emd, emd_bwd, sample_points_bwd, masked mean, Adam): "
              f"{med_re * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {med_re / med_r:.2f} x the Chamfer step")
        want_e = emd_torch_loop(px, nxl, py, nyl)
        med_te, lo_t, hi_t = timed(lambda: emd_torch_loop(px, nxl, py, nyl), inner=1, runs=3, warmup=1)
        print(f"[{tag}] torch loop of the ordered loss over {N} icons (3 runs): {med_te:8.2f} ms [{lo_t:.2f} .. {hi_t:.2f}] = "
              f"{med_te / med_e:.0f} x the kernel; max |kernel - torch loop| {float((out_e - want_e).abs().max()):.2e}, mean loss "
              f"{float(out_e.mean()):.4f}")

        def emd_loop_backward():
            pxl.grad = None
            emd_torch_loop(pxl, nxl, py, nyl).sum().backward()
        med_teb, lo_t, hi_t = timed(emd_loop_backward, inner=1, runs=3, warmup=1)
        print(f"[{tag}] torch loop of the ordered loss, forward + autograd backward (3 runs): {med_teb:8.2f} ms [{lo_t:.2f} .. "
              f"{hi_t:.2f}] = {med_teb / (med_e + med_eb):.0f} x emd + emd_bwd")


if __name__ == "__main__":
    main()
