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

The other losses of deepsvg/difflib/loss.py are here as well, batched in the same way.  `emd` is ``svg_emd_loss``
(loss.py:21-51), the ORDERED point loss that the notebook's optimisation cell actually minimises: the target is oriented
(``make_clockwise``), sampled at the pred cloud's uniform arc-length fractions, and the cyclic shift with the smallest mean
point-to-point distance is taken - a curve that visits the right places in the wrong order does not score well, as it does
under the order-free Chamfer distance.  Lengths and the shift sums are float64 on the device, so orientation, matching and
shift are properties of the input (the lowest index wins every tie); the gradient is with respect to the PRED cloud only,
the target is a constant, as in the notebook.  `polyline_length`, `svg_length_loss` (:15-18) and `continuity_loss` (:10-12)
complete the file; `emd_loss` is the batch loss and ``refine(loss="emd")`` the notebook's loop with the notebook's loss.
"""
import contextlib

import torch
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["sample_points", "chamfer", "reconstruction_error", "chamfer_loss", "refine", "emd", "emd_loss", "polyline_length",
           "svg_length_loss", "continuity_loss"]


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


class _Emd(torch.autograd.Function):
    """ops.emd with ops.emd_bwd behind it; the gradient is for the pred cloud only"""

    @staticmethod
    def forward(ctx, px, nx, py, ny, first_point_weight):
        out, shift, matched, t = ops.emd(px, nx, py, ny, first_point_weight)
        ctx.save_for_backward(px, nx, ny, t, shift)
        ctx.first_point_weight = first_point_weight
        ctx.mark_non_differentiable(shift, matched)
        return out, shift, matched

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dshift, _dmatched):
        return ops.emd_bwd(*ctx.saved_tensors, dout.contiguous(), ctx.first_point_weight), None, None, None, None


class _PolylineLength(torch.autograd.Function):
    """ops.polyline_length with ops.polyline_length_bwd behind it"""

    @staticmethod
    def forward(ctx, p, n):
        ctx.save_for_backward(p, n)
        return ops.polyline_length(p, n)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return ops.polyline_length_bwd(*ctx.saved_tensors, dout.contiguous()), None


def _flat_sequences(name, commands, args):
    """commands (N, S) or (N, G, S) with args (..., S, 11), refused under the caller's `name` -> (commands [N * G, S], args
    [N * G, S, 11], G): contiguous, and both float32 unless they are both float32 or both int64 already"""
    if commands.dim() not in (2, 3) or args.dim() != commands.dim() + 1 or args.shape[:-1] != commands.shape:
        raise ValueError(f"{name}: commands (N, S) or (N, G, S) with args (..., S, 11); got {tuple(commands.shape)} "
                         f"and {tuple(args.shape)}")
    if commands.dtype != args.dtype or commands.dtype not in (torch.float32, torch.int64):
        commands, args = commands.float(), args.float()
    groups = commands.shape[1] if commands.dim() == 3 else 1
    S = commands.shape[-1]
    return commands.reshape(-1, S).contiguous(), args.reshape(-1, S, args.shape[-1]).contiguous(), groups


@contextlib.contextmanager
def _evaluating(model):
    """eval mode and no gradients inside; the model's train / eval state is restored"""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)


def _masked_mean(per_icon, valid):
    """the mean of `per_icon` over the `valid` icons: the others are masked out before the sum; NaN when there is none"""
    return torch.where(valid, per_icon, torch.zeros_like(per_icon)).sum() / valid.sum()


def _adam_refine(args, steps, lr, batch_loss):
    """Adam on a float32 copy of `args`, minimising the 0-d batch_loss(refined) -> (refined args f32, history f32 [steps]:
    the loss before each step, kept on the device - the loop reads nothing back)"""
    refined = args.detach().float().clone().requires_grad_(True)
    opt = torch.optim.Adam([refined], lr=lr)
    history = torch.empty(steps, dtype=torch.float32, device=refined.device)
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        value = batch_loss(refined)
        value.backward()
        history[step] = value.detach()
        opt.step()
    return refined.detach(), history


def sample_points(commands, args, n=10):
    """commands [N, S] -> one cloud per row; commands [N, G, S] -> one cloud per icon, its groups concatenated in order;
    args [..., S, 11].  float32 (as the dataset delivers them) and int64 (as greedy_sample returns them) are read as they
    are.  -> (points f32 [N, cap, 2], counts int32 [N]): every `l` / `c` command gives its points at z = k / (n - 1), the
    end point shared with the next command once; a sequence with k drawing commands gives k (n - 1) + 1 points, one
    with none (an invisible group, where the reference raises) gives 0.  Rows past counts[i] are unspecified.
    float32 args that require grad (grad mode on) get their gradient through `points`; `counts` carries none."""
    commands, args, groups = _flat_sequences("sample_points", commands, args)
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
    with _evaluating(model):
        commands_y, args_y = model.greedy_sample(commands, args, commands, args, label=label, concat_groups=False,
                                                 temperature=temperature)
        px, nx = sample_points(commands_y, args_y, n)
        py, ny = sample_points(commands, args, n)
        re = chamfer(px, nx, py, ny)
        valid = (nx > 0) & (ny > 0)
        mean = _masked_mean(re, valid)
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
    return {"loss": _masked_mean(per_icon, valid), "per_icon": per_icon, "valid": valid}


def emd(points_x, counts_x, points_y, counts_y, first_point_weight=False, return_matched_indices=False):
    """The reference's ``svg_emd_loss`` (deepsvg/difflib/loss.py:21-51) of pred clouds x against target clouds y, both as
    sample_points returns them -> f32 [N]; with `return_matched_indices` -> (loss, matched int32 [N, cap_x], shift int32
    [N]): matched[i, k] is the index into points_y[i] AS PASSED (the orientation flip is undone) of the point paired with
    x_k, -1 past counts_x[i].  0 where x is empty, NaN where only y is.  `first_point_weight` counts the first pair 10
    times; it does not influence the shift.  Differentiable with respect to points_x ONLY (the target is a constant, as in
    the notebook); the same bits with and without gradients, bit-reproducible."""
    clouds = (points_x.contiguous(), counts_x.contiguous(), points_y.detach().contiguous(), counts_y.contiguous())
    if torch.is_grad_enabled() and points_x.requires_grad:
        loss, shift, matched = _Emd.apply(*clouds, bool(first_point_weight))
    else:
        loss, shift, matched, _ = ops.emd(*clouds, bool(first_point_weight))
    return (loss, matched, shift) if return_matched_indices else loss


def emd_loss(commands, args, target_points, target_counts, n=10, first_point_weight=False):
    """chamfer_loss with `emd` in the place of `chamfer`: -> {"loss": 0-d, "per_icon": f32 [N], "valid": bool [N]}, `valid`
    where both clouds are non-empty, `loss` the mean of `per_icon` over the valid icons (NaN when there is none; the
    gradient is zero on the others either way)."""
    points, counts = sample_points(commands, args, n)
    per_icon = emd(points, counts, target_points, target_counts, first_point_weight)
    valid = (counts > 0) & (target_counts > 0)
    return {"loss": _masked_mean(per_icon, valid), "per_icon": per_icon, "valid": valid}


def polyline_length(points, counts):
    """clouds as sample_points returns them -> f32 [N]: sum_i |p_{i+1} - p_i| over the points in use (``get_length``,
    deepsvg/difflib/utils.py:67-69), 0 for clouds of 0 or 1 point.  Differentiable with respect to `points`; a zero-length
    segment contributes no gradient."""
    points, counts = points.contiguous(), counts.contiguous()
    if torch.is_grad_enabled() and points.requires_grad:
        return _PolylineLength.apply(points, counts)
    return ops.polyline_length(points, counts)


def svg_length_loss(points_x, counts_x, points_y, counts_y):
    """The reference's ``svg_length_loss`` (loss.py:15-18): |L_y - L_x| / L_y -> f32 [N], NaN (and a zero gradient)
    where L_y == 0.  Differentiable with respect to points_x; the target is a constant."""
    target = polyline_length(points_y.detach(), counts_y)
    ratio = (target - polyline_length(points_x, counts_x)).abs() / torch.where(target > 0, target, torch.ones_like(target))
    return torch.where(target > 0, ratio, torch.full_like(ratio, float("nan")))


def continuity_loss(points, counts):
    """The reference's ``continuity_loss`` (loss.py:10-12): the mean segment length L / (count - 1) -> f32 [N], NaN where
    count < 2 (the mean of nothing).  Differentiable with respect to `points`."""
    segments = (counts - 1).clamp(min=0).to(torch.float32)
    length = polyline_length(points, counts)
    return torch.where(segments > 0, length / segments.clamp(min=1), torch.full_like(length, float("nan")))


_REFINE_LOSSES = {"chamfer": chamfer_loss, "emd": emd_loss}


def refine(commands, args, target_points, target_counts, steps=150, lr=0.1, n=10, loss="chamfer"):
    """The loop of notebooks/svgtensor.ipynb ("Differentiable SVGTensor optimization") for a whole batch: Adam on a float32
    copy of `args`, minimising `chamfer_loss` (loss="chamfer", the default) or `emd_loss` (loss="emd") against the target
    clouds.  The notebook's own cell minimises ``svg_emd_loss``, i.e. loss="emd"; the order-free Chamfer distance also accepts
    a curve that visits the right places in another order.  -> (refined args f32, history f32 [steps]: the
    loss before each step, kept on the device - the loop reads nothing back).  Elements whose gradient is always zero
    (columns 0-4, padding, rows that neither draw nor precede a drawing row) come back as they went in."""
    if loss not in _REFINE_LOSSES:
        raise ValueError(f"refine: loss {loss!r}, need one of {sorted(_REFINE_LOSSES)}")
    batch_loss = _REFINE_LOSSES[loss]
    return _adam_refine(args, steps, lr, lambda refined: batch_loss(commands, refined, target_points, target_counts, n)["loss"])
