"""Plain-torch restatements of ops.sample_points and ops.chamfer (deepsvg_amd/csrc/metrics.hip), batched, float64 inside.
install() puts them in place of the two ops, on top of the emulated_ops fixture, so that deepsvg_amd.metrics runs on CPU
(tests/long_ops_ref.py does the same for the long-path ops)."""
import torch

L_ID, C_ID = 1, 2


def sample_points(commands, args, n=10, groups=1):
    """same contract as ops.sample_points; rows past counts[b] are zero here"""
    assert commands.dim() == 2 and args.dim() == 3 and commands.shape[0] % groups == 0
    R, L = commands.shape
    B = R // groups
    cmd = commands.long()
    a = args.double()
    end = a[:, :, 9:11]
    start = torch.cat([torch.zeros_like(end[:, :1]), end[:, :-1]], dim=1)            # row i starts where row i - 1 ended
    p1, p2 = a[:, :, 5:7], a[:, :, 7:9]
    z = (torch.arange(n, dtype=torch.float64, device=a.device) / (n - 1)).view(1, 1, n, 1)
    s, c1, c2, e = (t.unsqueeze(2) for t in (start, p1, p2, end))
    line = s + z * (e - s)
    w = 1 - z
    cubic = w ** 3 * s + 3 * w ** 2 * z * c1 + 3 * w * z ** 2 * c2 + z ** 3 * e
    pts = torch.where((cmd == C_ID).view(R, L, 1, 1), cubic, line)                   # [R, L, n, 2]
    draw = (cmd == L_ID) | (cmd == C_ID)                                             # [R, L]
    k = draw.sum(1)
    is_last = draw & (draw.long().cumsum(1) == k.unsqueeze(1))                       # the sequence's last drawing command
    keep = draw.unsqueeze(2).expand(R, L, n).clone()
    keep[:, :, n - 1] &= is_last
    cap = groups * (L * (n - 1) + 1)
    keep = keep.reshape(B, groups * L * n)
    pts = pts.reshape(B, groups * L * n, 2)
    counts = keep.sum(1)
    dest = keep.long().cumsum(1) - 1
    out = torch.zeros(B, cap + 1, 2, dtype=torch.float64, device=a.device)           # slot `cap` takes what is dropped
    dest = torch.where(keep, dest, torch.full_like(dest, cap))
    out.scatter_(1, dest.unsqueeze(-1).expand(-1, -1, 2), pts)
    return out[:, :cap].float(), counts.to(torch.int32)


def chamfer(px, nx, py, ny, as_double=False):
    """same contract as ops.chamfer: brute force over the float64 distance matrix, one icon at a time"""
    out = torch.full((px.shape[0],), float("nan"), dtype=torch.float64, device=px.device)
    for b in range(px.shape[0]):
        cx, cy = int(nx[b]), int(ny[b])
        if cx == 0 or cy == 0:
            continue
        x, y = px[b, :cx].double(), py[b, :cy].double()
        d = (x.unsqueeze(1) - y.unsqueeze(0)).pow(2).sum(-1).sqrt()
        out[b] = d.min(1).values.mean() + d.min(0).values.mean()
    return out if as_double else out.float()


NAMES = ("sample_points", "chamfer")


def install():
    """on top of tests/conftest.py's emulated_ops: -> the replaced functions, for restore()"""
    import deepsvg_amd.ops as ops
    saved = {n: getattr(ops, n) for n in NAMES}
    g = globals()
    for n in NAMES:
        setattr(ops, n, g[n])
    return saved


def restore(saved):
    import deepsvg_amd.ops as ops
    for n, fn in saved.items():
        setattr(ops, n, fn)
