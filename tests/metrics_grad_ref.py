"""Plain-torch restatements of ops.chamfer_nn, ops.chamfer_bwd and ops.sample_points_bwd (deepsvg_amd/csrc/metrics.hip),
float64 inside.  chamfer_bwd TAKES the arg-min indices, as the kernel does: fed the kernel's own indices it follows the
kernel's choice of nearest point, so no arg-min flip can enter a comparison.  install() puts them, and the two forward
restatements of tests/metrics_ref.py, in place of the ops on top of the emulated_ops fixture, so that the autograd wiring
of deepsvg_amd.metrics runs on CPU."""
import torch

from tests import metrics_ref as MR

L_ID, C_ID = MR.L_ID, MR.C_ID


def sample_points64(commands, args, n=10, groups=1):
    """MR.sample_points with float64 points (the same counts): what the reference computes, without its fp32 rounding"""
    R, L = commands.shape
    B = R // groups
    cmd, a = commands.long(), args.double()
    end = a[:, :, 9:11]
    start = torch.cat([torch.zeros_like(end[:, :1]), end[:, :-1]], dim=1)
    z = (torch.arange(n, dtype=torch.float64) / (n - 1)).view(1, 1, n, 1)
    s, c1, c2, e = (t.unsqueeze(2) for t in (start, a[:, :, 5:7], a[:, :, 7:9], end))
    w = 1 - z
    pts = torch.where((cmd == C_ID).view(R, L, 1, 1), w ** 3 * s + 3 * w ** 2 * z * c1 + 3 * w * z ** 2 * c2 + z ** 3 * e,
                      s + z * (e - s))
    keep, dest, counts = _layout(cmd, n, groups)
    cap = groups * (L * (n - 1) + 1)
    out = torch.zeros(B, cap + 1, 2, dtype=torch.float64)
    dest = torch.where(keep, dest, torch.full_like(dest, cap))
    out.scatter_(1, dest.unsqueeze(-1).expand(-1, -1, 2), pts.reshape(B, groups * L * n, 2))
    return out[:, :cap], counts.to(torch.int32)


def _layout(cmd, n, groups):
    """-> keep bool [B, G * L * n]: sample k of token t is a point; dest: its row in the cloud; counts [B]"""
    R, L = cmd.shape
    draw = (cmd == L_ID) | (cmd == C_ID)
    is_last = draw & (draw.long().cumsum(1) == draw.sum(1, keepdim=True))           # the sequence's last drawing command
    keep = draw.unsqueeze(2).expand(R, L, n).clone()
    keep[:, :, n - 1] &= is_last
    keep = keep.reshape(R // groups, groups * L * n)
    return keep, keep.long().cumsum(1) - 1, keep.sum(1)


def sample_points_bwd(commands, dpoints, n=10, groups=1, as_double=False):
    """same contract as ops.sample_points_bwd"""
    assert commands.dim() == 2 and commands.dtype == torch.float32 and commands.shape[0] % groups == 0
    R, L = commands.shape
    B = R // groups
    assert dpoints.shape == (B, groups * (L * (n - 1) + 1), 2)
    cmd = commands.long()
    keep, dest, _ = _layout(cmd, n, groups)
    dP = dpoints.double().gather(1, dest.clamp(min=0).unsqueeze(-1).expand(-1, -1, 2))
    dP = torch.where(keep.unsqueeze(-1), dP, torch.zeros_like(dP)).reshape(R, L, n, 2)       # of sample k of token t
    z = (torch.arange(n, dtype=torch.float64) / (n - 1)).view(1, 1, n, 1)
    w = 1 - z
    cubic = (cmd == C_ID).view(R, L, 1, 1)
    dargs = torch.zeros(R, L, 11, dtype=torch.float64)
    dargs[:, :, 5:7] = torch.where(cubic, 3 * w ** 2 * z * dP, torch.zeros_like(dP)).sum(2)
    dargs[:, :, 7:9] = torch.where(cubic, 3 * w * z ** 2 * dP, torch.zeros_like(dP)).sum(2)
    dargs[:, :, 9:11] = torch.where(cubic, z ** 3 * dP, z * dP).sum(2)
    start = torch.where(cubic, w ** 3 * dP, w * dP).sum(2)              # to the end position of the row before, whatever it holds
    dargs[:, :-1, 9:11] += start[:, 1:]                                 # (row 0 starts at the constant (0, 0))
    return dargs if as_double else dargs.float()


def chamfer_nn(px, nx, py, ny):
    """same contract as ops.chamfer_nn: float64 brute force, the lowest index of equidistant candidates; entries past the
    counts are zero here"""
    B = px.shape[0]
    idx_x = torch.zeros(B, px.shape[1], dtype=torch.int32)
    idx_y = torch.zeros(B, py.shape[1], dtype=torch.int32)
    for b in range(B):
        cx, cy = int(nx[b]), int(ny[b])
        if cx == 0 or cy == 0:
            continue
        d2 = (px[b, :cx].double().unsqueeze(1) - py[b, :cy].double().unsqueeze(0)).pow(2).sum(-1)
        idx_x[b, :cx] = d2.argmin(1).to(torch.int32)
        idx_y[b, :cy] = d2.argmin(0).to(torch.int32)
    return MR.chamfer(px, nx, py, ny), idx_x, idx_y


def _unit(a, b):
    d = a - b
    r = d.norm(dim=-1, keepdim=True)
    return torch.where(r > 0, d / r, torch.zeros_like(d))


def chamfer_bwd(px, nx, py, ny, idx_x, idx_y, dout, as_double=False):
    """same contract as ops.chamfer_bwd, with the indices as given"""
    dpx = torch.zeros(px.shape, dtype=torch.float64)
    dpy = torch.zeros(py.shape, dtype=torch.float64)
    for b in range(px.shape[0]):
        cx, cy = int(nx[b]), int(ny[b])
        if cx == 0 or cy == 0:
            continue                                    # zero rows whatever dout[b] holds
        x, y = px[b, :cx].double(), py[b, :cy].double()
        jx, iy = idx_x[b, :cx].long(), idx_y[b, :cy].long()
        gx = _unit(x, y[jx]) / cx
        gx.index_add_(0, iy, -_unit(y, x[iy]) / cy)
        gy = _unit(y, x[iy]) / cy
        gy.index_add_(0, jx, -_unit(x, y[jx]) / cx)
        dpx[b, :cx], dpy[b, :cy] = dout[b].double() * gx, dout[b].double() * gy
    return (dpx, dpy) if as_double else (dpx.float(), dpy.float())


NAMES = ("chamfer_nn", "chamfer_bwd", "sample_points_bwd")


def install():
    """on top of tests/conftest.py's emulated_ops: the forward pair of metrics_ref and the three above -> what restore()
    needs"""
    import deepsvg_amd.ops as ops
    saved = MR.install()
    saved.update({n: getattr(ops, n) for n in NAMES})
    g = globals()
    for n in NAMES:
        setattr(ops, n, g[n])
    return saved


def restore(saved):
    MR.restore(saved)
