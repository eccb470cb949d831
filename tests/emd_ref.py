"""Plain-torch restatements of the ordered point loss and the polyline length of deepsvg_amd/csrc/metrics.hip (ops.emd,
ops.emd_bwd, ops.polyline_length, ops.polyline_length_bwd, and emd_match, the matching stage of ops.emd on its own), float64
inside, written from the definition in include/dsvg.h - one icon at a time, the [n] x [n] shift sums in the open.

`float_terms=True` forms each term |x_k - t_j| in float32 (difference, squares, sum, sqrt: the kernel's arithmetic up to its
fused multiply-add) and adds the terms in float64, which is what the kernel does; the default forms them in float64.  emd
takes an optional `t` (and `match`): fed the kernel's own gathered target points it follows the kernel's matching, so that
no near-tie of the arc-length match can enter a comparison of the later stages.  install() puts the four ops in place of
the ops functions on top of the emulated_ops fixture and metrics_grad_ref.install(), so that the autograd wiring of
deepsvg_amd.metrics runs on CPU."""
import torch

from tests import metrics_grad_ref as GR


def orientation(y):
    """y float64 [m, 2] -> A, the shoelace sum of the open polyline"""
    return (y[:-1, 0] * y[1:, 1] - y[1:, 0] * y[:-1, 1]).sum()


def emd_match(n, y):
    """n pred points against the target y [m, 2] (m >= 1) -> (match int64 [n]: indices into y AS PASSED, flip: bool, gap: the
    smallest difference between the nearest and the second-nearest |u_i - D_j| over the pred points, inf where m == 1, A)"""
    y = y.double()
    m = y.shape[0]
    A = orientation(y)
    flip = not bool(A > 0)
    yo = y.flip(0) if flip else y
    seg = (yo[1:] - yo[:-1]).norm(dim=-1)
    cum = torch.cat([seg.new_zeros(1), seg.cumsum(0)])
    total = cum[-1]
    if m == 1 or not bool(total > 0):
        j = torch.zeros(n, dtype=torch.int64)
        gap = float("inf")
    else:
        D = cum / total
        u = torch.arange(n, dtype=torch.float64) / max(n - 1, 1)
        d = (u.unsqueeze(1) - D.unsqueeze(0)).abs()
        j = d.argmin(1)                                  # torch's argmin returns the first of equal minima
        two = d.topk(2, dim=1, largest=False).values
        gap = float((two[:, 1] - two[:, 0]).min())
    return (m - 1 - j if flip else j), flip, gap, float(A)


def match_error(n, y, match):
    """how far each given matched index (into y as passed) is from the best: |u_i - D_j| - min_j |u_i - D_j|, float64 [n]"""
    y = y.double()
    m = y.shape[0]
    flip = not bool(orientation(y) > 0)
    yo = y.flip(0) if flip else y
    seg = (yo[1:] - yo[:-1]).norm(dim=-1)
    cum = torch.cat([seg.new_zeros(1), seg.cumsum(0)])
    if m == 1 or not bool(cum[-1] > 0):
        return ((m - 1 - match if flip else match) != 0).double()
    D = cum / cum[-1]
    u = torch.arange(n, dtype=torch.float64) / max(n - 1, 1)
    d = (u.unsqueeze(1) - D.unsqueeze(0)).abs()
    j = m - 1 - match.long() if flip else match.long()
    return d.gather(1, j.unsqueeze(1)).squeeze(1) - d.min(1).values


def terms(x, t, float_terms):
    """|x - t| per row -> float64"""
    if float_terms:
        d = x.float() - t.float()
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).sqrt().double()
    return (x.double() - t.double()).norm(dim=-1)


def shift_sums(x, t, float_terms=False):
    """S(s) = sum_k |x_k - t_{(k+s) mod n}| for s = 0 .. n - 1 -> float64 [n]"""
    n = x.shape[0]
    k = torch.arange(n)
    S = torch.empty(n, dtype=torch.float64)
    for s0 in range(0, n, 256):
        s = torch.arange(s0, min(s0 + 256, n))
        idx = (k.unsqueeze(0) + s.unsqueeze(1)) % n                     # [shifts, n]
        S[s0:s0 + len(s)] = terms(x.unsqueeze(0), t[idx], float_terms).sum(1)
    return S


def emd(px, nx, py, ny, first_point_weight=False, float_terms=False, as_double=False, t=None, match=None):
    """same contract as ops.emd -> (out, shift int32 [B], matched int32 [B, capx], t f32 [B, capx, 2]; rows of t past the
    counts are zero here).  With `t` (and optionally `match`, indices into py as passed BEFORE the shift) given, the matching
    stage is skipped and they are used as they are."""
    B, capx = px.shape[0], px.shape[1]
    out = torch.zeros(B, dtype=torch.float64)
    shift = torch.zeros(B, dtype=torch.int32)
    matched = torch.full((B, capx), -1, dtype=torch.int32)
    t_out = torch.zeros(B, capx, 2, dtype=torch.float64)
    for b in range(B):
        n, m = int(nx[b]), int(ny[b])
        if n == 0:
            continue
        if m == 0:
            out[b] = float("nan")
            continue
        x = px[b, :n].double()
        if t is None:
            mt = emd_match(n, py[b, :m])[0]
            tb = py[b, :m].double()[mt]
        else:
            tb = t[b, :n].double()
            mt = match[b, :n].long() if match is not None else None
        S = shift_sums(x, tb, float_terms)
        s = int(S.argmin())                                             # the first of equal minima
        value = S[s]
        if first_point_weight:
            value = value + 9.0 * terms(x[0], tb[s], float_terms)
        out[b], shift[b], t_out[b, :n] = value / n, s, tb
        if mt is not None:
            matched[b, :n] = torch.cat([mt[s:], mt[:s]]).to(torch.int32)
    return (out, shift, matched, t_out) if as_double else (out.float(), shift, matched, t_out.float())


def emd_bwd(px, nx, ny, t, shift, dout, first_point_weight=False, as_double=False):
    """same contract as ops.emd_bwd"""
    dpx = torch.zeros(px.shape, dtype=torch.float64)
    for b in range(px.shape[0]):
        n = int(nx[b])
        if n == 0 or int(ny[b]) == 0:
            continue
        s = int(shift[b])
        tb = t[b, :n].double()
        g = GR._unit(px[b, :n].double(), torch.cat([tb[s:], tb[:s]])) / n
        if first_point_weight:
            g[0] = g[0] * 10.0
        dpx[b, :n] = dout[b].double() * g
    return dpx if as_double else dpx.float()


def polyline_length(p, n, as_double=False):
    """same contract as ops.polyline_length"""
    out = torch.zeros(p.shape[0], dtype=torch.float64)
    for b in range(p.shape[0]):
        x = p[b, :int(n[b])].double()
        if x.shape[0] > 1:
            out[b] = (x[1:] - x[:-1]).norm(dim=-1).sum()
    return out if as_double else out.float()


def polyline_length_bwd(p, n, dout, as_double=False):
    """same contract as ops.polyline_length_bwd"""
    dp = torch.zeros(p.shape, dtype=torch.float64)
    for b in range(p.shape[0]):
        c = int(n[b])
        if c < 2:
            continue
        x = p[b, :c].double()
        u = GR._unit(x[1:], x[:-1])                                     # of segment i: towards its end point
        g = torch.zeros_like(x)
        g[1:] += u
        g[:-1] -= u
        dp[b, :c] = dout[b].double() * g
    return dp if as_double else dp.float()


NAMES = ("emd", "emd_bwd", "polyline_length", "polyline_length_bwd")


def install():
    """on top of tests/conftest.py's emulated_ops: metrics_grad_ref.install() and the four above -> what restore() needs"""
    import deepsvg_amd.ops as ops
    saved = GR.install()
    saved.update({n: getattr(ops, n) for n in NAMES})
    g = globals()
    for n in NAMES:
        setattr(ops, n, g[n])
    return saved


def restore(saved):
    GR.restore(saved)
