"""Reconstruction error of decoded icons, on the device: the Chamfer distance between points sampled on the decoded curves
and on the target curves (the RE of the DeepSVG paper).  Replaces a host loop over paths of the reference's
``SVGTensor.sample_points`` (deepsvg/difflib/tensor.py:191-230) and ``chamfer_loss`` (deepsvg/difflib/loss.py:5-7), whose
``torch.cdist`` matrix is 23 MB per icon (and as much again in its backward).  Units are argument units, 0..255.

Both functions are differentiable, as the reference's are (notebooks/svgtensor.ipynb optimises Bezier parameters through
them): float32 ``args`` that require grad receive ``d / d args`` through ``sample_points`` -> ``chamfer``; `chamfer_loss` is
the batch loss and `refine` the notebook's Adam loop on top.  The gradient is the arg-min gather of csrc/metrics.hip: of
equidistant nearest points the lowest index takes the term, a pair at distance zero contributes nothing (chamfer(x, x) has
a zero gradient), the start point of a drawing command is the end position of the row before it whatever that row holds,
and an icon with an empty cloud gets a zero gradient.  No distance matrix, no atomics: bit-reproducible.  int64 inputs,
calls under ``torch.no_grad()`` and inputs that do not require grad take the forward-only kernels, as before.
`reconstruction_error` stays an evaluation: no gradients.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["sample_points", "chamfer", "reconstruction_error", "chamfer_loss", "refine"]


class _SamplePoints(torch.autograd.Function):
    """ops.sample_points on flat float32 inputs; linear in args, so the backward needs the commands only"""

    @staticmethod
    def forward(ctx, args, commands, n, groups):
        points, counts = ops.sample_points(commands, args, n=n, groups=groups)
        ctx.save_for_backward(commands)
        ctx.n, ctx.groups = n, groups
        ctx.mark_non_differentiable(counts)
        return points, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, dpoints, _dcounts):
        commands, = ctx.saved_tensors
        return ops.sample_points_bwd(commands, dpoints.contiguous(), n=ctx.n, groups=ctx.groups), None, None, None


class _Chamfer(torch.autograd.Function):
    """ops.chamfer_nn (the bits of ops.chamfer, plus the arg-min indices) with ops.chamfer_bwd behind it"""

    @staticmethod
    def forward(ctx, px, nx, py, ny):
        out, idx_x, idx_y = ops.chamfer_nn(px, nx, py, ny)
        ctx.save_for_backward(px, nx, py, ny, idx_x, idx_y)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        dpx, dpy = ops.chamfer_bwd(*ctx.saved_tensors, dout.contiguous())
        return dpx if ctx.needs_input_grad[0] else None, None, dpy if ctx.needs_input_grad[2] else None, None


def sample_points(commands, args, n=10):
    """commands [N, S] -> one cloud per row; commands [N, G, S] -> one cloud per icon, its groups concatenated in order;
    args [..., S, 11].  float32 (as the dataset delivers them) and int64 (as greedy_sample returns them) are read as they
    are.  -> (points f32 [N, cap, 2], counts int32 [N]): every `l` / `c` command gives its points at z = k / (n - 1), the
    end point shared with the next command once; a sequence with k drawing commands gives k (n - 1) + 1 points, one
    with none (an invisible group, where the reference raises) gives 0.  Rows past counts[i] are unspecified.
    float32 args that require grad (grad mode on) get their gradient through `points`; `counts` carries none."""
    if commands.dim() not in (2, 3) or args.dim() != commands.dim() + 1 or args.shape[:-1] != commands.shape:
        raise ValueError(f"sample_points: commands (N, S) or (N, G, S) with args (..., S, 11); got {tuple(commands.shape)} "
                         f"and {tuple(args.shape)}")
    if commands.dtype != args.dtype or commands.dtype not in (torch.float32, torch.int64):
        commands, args = commands.float(), args.float()
    groups = commands.shape[1] if commands.dim() == 3 else 1
    S = commands.shape[-1]
    commands, args = commands.reshape(-1, S).contiguous(), args.reshape(-1, S, args.shape[-1]).contiguous()
    if args.dtype == torch.float32 and args.requires_grad and torch.is_grad_enabled():
        return _SamplePoints.apply(args, commands.detach(), n, groups)
    return ops.sample_points(commands, args, n=n, groups=groups)


def chamfer(points_x, counts_x, points_y, counts_y):
    """clouds as sample_points returns them -> f32 [N]: mean_i min_j |x_i - y_j| + mean_j min_i |x_i - y_j| (Euclidean);
    NaN where either cloud is empty.  Symmetric bit for bit, and bit-reproducible from run to run.  Differentiable with
    respect to either cloud (same bits as without): rows past the counts and icons with an empty cloud get zeros."""
    clouds = (points_x.contiguous(), counts_x.contiguous(), points_y.contiguous(), counts_y.contiguous())
    if torch.is_grad_enabled() and (points_x.requires_grad or points_y.requires_grad):
        return _Chamfer.apply(*clouds)
    return ops.chamfer(*clouds)


def reconstruction_error(model, commands, args, label=None, n=10, temperature=0.0):
    """Decode `commands` / `args` with ``model.greedy_sample`` and compare the decoded icons with the targets, taken exactly
    as passed (SOS, EOS and padding give no points).  -> {"re": f32 [N], "valid": bool [N], "mean": 0-d}: `valid` where both
    clouds are non-empty, `re` NaN elsewhere, `mean` over the valid icons.  Runs without gradients in eval mode; the
    model's train / eval state is restored."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            commands_y, args_y = model.greedy_sample(commands, args, commands, args, label=label, concat_groups=False,
                                                     temperature=temperature)
            px, nx = sample_points(commands_y, args_y, n)
            py, ny = sample_points(commands, args, n)
            re = chamfer(px, nx, py, ny)
            valid = (nx > 0) & (ny > 0)
            mean = torch.where(valid, re, torch.zeros_like(re)).sum() / valid.sum()
    finally:
        model.train(was_training)
    return {"re": re, "valid": valid, "mean": mean}


def chamfer_loss(commands, args, target_points, target_counts, n=10):
    """The reference's ``chamfer_loss`` (deepsvg/difflib/loss.py:5-7) of the curves of `commands` / `args` (as sample_points
    takes them) against target clouds (as sample_points returns them), for a whole batch.
    -> {"loss": 0-d, "per_icon": f32 [N], "valid": bool [N]}: `valid` where both clouds are non-empty, `per_icon` NaN
    elsewhere, `loss` the mean over the valid icons - the others are masked out before the mean, so they add nothing to the
    loss and a zero gradient to `args`.  With no valid icon at all `loss` is NaN (the mean of nothing, as `mean` of
    reconstruction_error); the gradient is still zero everywhere, so an optimizer step on it changes nothing."""
    points, counts = sample_points(commands, args, n)
    per_icon = chamfer(points, counts, target_points, target_counts)
    valid = (counts > 0) & (target_counts > 0)
    loss = torch.where(valid, per_icon, torch.zeros_like(per_icon)).sum() / valid.sum()
    return {"loss": loss, "per_icon": per_icon, "valid": valid}


def refine(commands, args, target_points, target_counts, steps=150, lr=0.1, n=10):
    """The loop of notebooks/svgtensor.ipynb ("Differentiable SVGTensor optimization") for a whole batch: Adam on a float32
    copy of `args`, minimising `chamfer_loss` against the target clouds.  -> (refined args f32, history f32 [steps]: the
    loss before each step, kept on the device - the loop reads nothing back).  Elements whose gradient is always zero
    (columns 0-4, padding, rows that neither draw nor precede a drawing row) come back as they went in."""
    refined = args.detach().float().clone().requires_grad_(True)
    opt = torch.optim.Adam([refined], lr=lr)
    history = torch.empty(steps, dtype=torch.float32, device=refined.device)
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = chamfer_loss(commands, refined, target_points, target_counts, n)["loss"]
        loss.backward()
        history[step] = loss.detach()
        opt.step()
    return refined.detach(), history
