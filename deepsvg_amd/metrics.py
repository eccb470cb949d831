"""Reconstruction error of decoded icons, on the device: the Chamfer distance between points sampled on the decoded curves
and on the target curves (the RE of the DeepSVG paper).  Replaces a host loop over paths of the reference's
``SVGTensor.sample_points`` (deepsvg/difflib/tensor.py:191-230) and ``chamfer_loss`` (deepsvg/difflib/loss.py:5-7), whose
``torch.cdist`` matrix is 23 MB per icon.  Evaluation only: nothing here has a gradient.  Units are argument units, 0..255.
"""
import torch

from . import ops

__all__ = ["sample_points", "chamfer", "reconstruction_error"]


def sample_points(commands, args, n=10):
    """commands [N, S] -> one cloud per row; commands [N, G, S] -> one cloud per icon, its groups concatenated in order;
    args [..., S, 11].  float32 (as the dataset delivers them) and int64 (as greedy_sample returns them) are read as they
    are.  -> (points f32 [N, cap, 2], counts int32 [N]): every `l` / `c` command gives its points at z = k / (n - 1), the
    end point shared with the next command once; a sequence with k drawing commands gives k (n - 1) + 1 points, one
    with none (an invisible group, where the reference raises) gives 0.  Rows past counts[i] are unspecified."""
    if commands.dim() not in (2, 3) or args.dim() != commands.dim() + 1 or args.shape[:-1] != commands.shape:
        raise ValueError(f"sample_points: commands (N, S) or (N, G, S) with args (..., S, 11); got {tuple(commands.shape)} "
                         f"and {tuple(args.shape)}")
    if commands.dtype != args.dtype or commands.dtype not in (torch.float32, torch.int64):
        commands, args = commands.float(), args.float()
    groups = commands.shape[1] if commands.dim() == 3 else 1
    S = commands.shape[-1]
    return ops.sample_points(commands.reshape(-1, S).contiguous(), args.reshape(-1, S, args.shape[-1]).contiguous(), n=n,
                             groups=groups)


def chamfer(points_x, counts_x, points_y, counts_y):
    """clouds as sample_points returns them -> f32 [N]: mean_i min_j |x_i - y_j| + mean_j min_i |x_i - y_j| (Euclidean);
    NaN where either cloud is empty.  Symmetric bit for bit, and bit-reproducible from run to run."""
    return ops.chamfer(points_x.contiguous(), counts_x.contiguous(), points_y.contiguous(), counts_y.contiguous())


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
