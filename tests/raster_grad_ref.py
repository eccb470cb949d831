"""Float64 restatement of the gradient of an image (include/dsvg.h, "The gradient of an image"; deepsvg_amd/csrc/raster.hip:
dsvg_raster_sweep_nn, dsvg_raster_sweep_bwd, dsvg_raster_segments_bwd), written from the definition on top of the forward
restatement of tests/raster_ref.py.

A pixel's ink depends on the chords only through d, the distance to its nearest chord a -> b: with the closest point at the
clamped parameter t and q = p - (a + t (b - a)), d d / d a = -(1 - t) q / d and d d / d b = -t q / d; d ink / d d = -1 / s in
stroke mode and outside a filled shape, +1 / s inside one (ink > 0.5), 0 where the stored ink is 0 or 1.  Ties go to the
lowest chord index, a pixel with d == 0 contributes nothing.  raster_sweep_bwd TAKES the arg-min indices and the stored
image, as the kernel does: fed the kernel's own results it follows the kernel's choice of nearest chord and of live pixels,
so neither an arg-min flip nor a clamp decided by rounding can enter a comparison.

chord_vertices64 is the chord builder as differentiable torch: autograd through it is the oracle of raster_segments_bwd,
which is written out token by token here.  install() puts the restatements in place of the ops (with those of
tests/raster_ref.py), so that the autograd wiring of deepsvg_amd.render runs on CPU."""
import numpy as np
import torch

from tests import raster_ref as RR

L_ID, C_ID, VIEW = RR.L_ID, RR.C_ID, RR.VIEW


def chord_vertices64(commands, args, n=10, groups=1, fill=False):
    """RR.chord_list with `args` kept in the graph: commands [B*groups, L], args float64 [B*groups, L, 11] -> one dict per
    image: a, b float64 [C, 2] (functions of args), seq int64 [C]"""
    cmd = commands.detach().long().tolist()
    arg = args.double()
    R, L = len(cmd), len(cmd[0])
    z = (torch.arange(n, dtype=torch.float64) / (n - 1))[1:-1, None]
    w = 1 - z
    origin = torch.zeros(2, dtype=torch.float64)
    images = []
    for img in range(R // groups):
        a, b, seq = [], [], []
        for g in range(groups):
            row = img * groups + g
            sub_first = last = None
            for i in range(L):
                draws = cmd[row][i] in (L_ID, C_ID)
                if draws:
                    start = arg[row, i - 1, 9:11] if i else origin
                    end = arg[row, i, 9:11]
                    if cmd[row][i] == L_ID:
                        mid = w * start + z * end
                    else:
                        mid = w ** 3 * start + 3 * w ** 2 * z * arg[row, i, 5:7] + 3 * w * z ** 2 * arg[row, i, 7:9] + z ** 3 * end
                    v = torch.cat([start[None], mid, end[None]])
                    if sub_first is None:
                        sub_first = start
                    last = end
                    a.append(v[:-1])
                    b.append(v[1:])
                    seq += [g] * (n - 1)
                if sub_first is not None and (not draws or i == L - 1):
                    if fill:
                        a.append(last[None])
                        b.append(sub_first[None])
                        seq.append(g)
                    sub_first = None
        empty = torch.zeros(0, 2, dtype=torch.float64)
        images.append({"a": torch.cat(a) if a else empty, "b": torch.cat(b) if b else empty,
                       "seq": torch.tensor(seq, dtype=torch.int64)})
    return images


CHUNK = 256            # chords per [chords, H, W] broadcast


def _centres(size, dtype):
    s = VIEW / size
    centre = (torch.arange(size, dtype=dtype) + 0.5) * s
    return centre.view(1, size).expand(size, size), centre.view(size, 1).expand(size, size)          # x [H, W], y [H, W]


def _closest(a, d, px, py):
    """chords a + t d ([..., 2] each) against points (px, py), broadcast against a[..., 0] -> (t, qx, qy): the clamped
    parameter of the closest point (0 on a zero-length chord) and q = p - (a + t d)"""
    dx, dy = d[..., 0], d[..., 1]
    len2 = dx * dx + dy * dy
    rx, ry = px - a[..., 0], py - a[..., 1]
    t = torch.where(len2 > 0, (rx * dx + ry * dy) / torch.where(len2 > 0, len2, torch.ones_like(len2)),
                    torch.zeros_like(rx)).clamp(0, 1)
    return t, rx - t * dx, ry - t * dy


def nearest(a, b, size):
    """float64 chords a -> b ([C, 2]) -> (d float64 [size, size]: the distance to the nearest chord, inf without chords; idx
    int64 [size, size]: its index, the lowest of equidistant ones, -1 without chords)"""
    cx, cy = _centres(size, torch.float64)
    best = torch.full((size, size), float("inf"), dtype=torch.float64)
    idx = torch.full((size, size), -1, dtype=torch.int64)
    for j in range(0, a.shape[0], CHUNK):
        aj, dj = a[j:j + CHUNK].double().view(-1, 1, 1, 2), (b[j:j + CHUNK] - a[j:j + CHUNK]).double().view(-1, 1, 1, 2)
        _, qx, qy = _closest(aj, dj, cx, cy)
        d2 = qx * qx + qy * qy                              # [chords, size, size]
        m, arg = d2.min(0)                                  # (the first of equal minima)
        better = m < best                                   # strict: an earlier chunk keeps a tie
        best, idx = torch.where(better, m, best), torch.where(better, arg + j, idx)
    return best.sqrt(), idx


def distance_to(a, b, idx, size):
    """float64 distance of every pixel to the chord idx names ([size, size], idx < 0: inf)"""
    cx, cy = _centres(size, torch.float64)
    live = idx >= 0
    j = idx[live].long()
    _, qx, qy = _closest(a[j].double(), (b[j] - a[j]).double(), cx[live], cy[live])
    out = torch.full((size, size), float("inf"), dtype=torch.float64)
    out[live] = (qx * qx + qy * qy).sqrt()
    return out


def chords_bwd(a, b, ink, idx, dout, fill, dtype=torch.float64):
    """chords a -> b ([C, 2]), the stored image `ink`, the arg-min `idx` and dL / d ink `dout` (all [size, size]) -> (da, db)
    [C, 2]: dL / d vertices, every step in `dtype`"""
    size = ink.shape[-1]
    s = VIEW / size
    cx, cy = _centres(size, dtype)
    live = (idx >= 0) & (ink > 0) & (ink < 1)
    j = idx[live].long()
    aj, dj = a[j].to(dtype), (b[j] - a[j]).to(dtype)
    t, qx, qy = _closest(aj, dj, cx[live], cy[live])
    d = (qx * qx + qy * qy).sqrt()
    sign = torch.where(ink[live] > 0.5, 1.0, -1.0).to(dtype) if fill else -torch.ones_like(d)
    g = torch.where(d > 0, dout[live].to(dtype) * sign / s / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
    q = torch.stack([qx, qy], 1)
    da = torch.zeros(a.shape[0], 2, dtype=dtype).index_add_(0, j, -((1 - t) * g).unsqueeze(1) * q)
    db = torch.zeros(a.shape[0], 2, dtype=dtype).index_add_(0, j, -(t * g).unsqueeze(1) * q)
    return da, db


def smallest_live_distance(a, b, ink, idx):
    """the smallest float64 distance to its own chord among the pixels that carry a gradient (inf when there is none)"""
    d = distance_to(a, b, idx, ink.shape[-1])
    live = (idx >= 0) & (ink > 0) & (ink < 1)
    return d[live].min().item() if bool(live.any()) else float("inf")


def _chords_of(segs_i, count):
    r = segs_i[:int(count)]
    a = r[:, :2].double()
    return a, a + r[:, 2:4].double()


def raster_sweep_nn(segs, seg_counts, size=64, stroke_width=3.2, fill=False, cull=None):
    """same contract as ops.raster_sweep_nn: the image of RR.raster_sweep, the float64 arg-min"""
    out = RR.raster_sweep(segs, seg_counts, size=size, stroke_width=stroke_width, fill=fill)
    idx = torch.full(out.shape, -1, dtype=torch.int32)
    for i in range(segs.shape[0]):
        _, nn = nearest(*_chords_of(segs[i], seg_counts[i]), size)
        idx[i] = torch.where((out[i] > 0) & (out[i] < 1), nn, torch.full_like(nn, -1)).to(torch.int32)
    return out, idx


def raster_sweep_bwd(segs, seg_counts, out, idx, dout, stroke_width=3.2, fill=False, wide=None, dtype=torch.float64,
                     as_double=False):
    """same contract as ops.raster_sweep_bwd, with the image and the indices as given; rows past the counts are zero here"""
    dsegs = torch.zeros(segs.shape[0], segs.shape[1], 4, dtype=dtype)
    for i in range(segs.shape[0]):
        k = int(seg_counts[i])
        a, b = _chords_of(segs[i], k)
        da, db = chords_bwd(a, b, out[i], idx[i], dout[i], fill, dtype)
        dsegs[i, :k, :2], dsegs[i, :k, 2:] = da, db
    return dsegs if as_double else dsegs.float()


def raster_segments_bwd(commands, dsegs, seg_counts, n=10, groups=1, fill=False, dtype=np.float64, as_double=False):
    """same contract as ops.raster_segments_bwd: a walk over the rows of every sequence, as RR.chord_list; vertex q of a
    command is the a of its chord q and the b of its chord q - 1"""
    cmd = commands.detach().long().numpy()
    ds = dsegs.detach().numpy().astype(dtype)
    R, L = cmd.shape
    z = (np.arange(n, dtype=dtype) / dtype(n - 1))[:, None]
    w = 1 - z
    dargs = np.zeros((R, L, 11), dtype=dtype)
    for img in range(R // groups):
        count = 0
        for g in range(groups):
            row = img * groups + g
            first = None                                    # first row of the open sub-path
            for i in range(L):
                draws = cmd[row, i] in (L_ID, C_ID)
                if draws:
                    V = np.zeros((n, 2), dtype=dtype)
                    V[:-1] += ds[img, count:count + n - 1, :2]
                    V[1:] += ds[img, count:count + n - 1, 2:]
                    cubic = cmd[row, i] == C_ID
                    if cubic:
                        dargs[row, i, 5:7] = (3 * w ** 2 * z * V).sum(0)
                        dargs[row, i, 7:9] = (3 * w * z ** 2 * V).sum(0)
                    dargs[row, i, 9:11] += ((z ** 3 if cubic else z) * V).sum(0)
                    if i:
                        dargs[row, i - 1, 9:11] += ((w ** 3 if cubic else w) * V).sum(0)
                    if first is None:
                        first = i
                    count += n - 1
                if first is not None and (not draws or i == L - 1):
                    if fill:
                        dargs[row, i if draws else i - 1, 9:11] += ds[img, count, :2]
                        if first:
                            dargs[row, first - 1, 9:11] += ds[img, count, 2:]
                        count += 1
                    first = None
        assert count == int(seg_counts[img]), "dsegs was not built for these commands"
    out = torch.from_numpy(dargs)
    return out if as_double else out.float()


def rasterize(commands, args, size=64, stroke_width=3.2, fill=False, n=10, groups=1, cull=None):
    """same contract as ops.rasterize, and composed as it is: records -> image (RR.rasterize goes from the float64 chord list
    to the image and differs from this in the last bits)"""
    segs, seg_counts = RR.raster_segments(commands, args, n=n, groups=groups, fill=fill)
    return RR.raster_sweep(segs, seg_counts, size=size, stroke_width=stroke_width, fill=fill)


NAMES = ("raster_sweep_nn", "raster_sweep_bwd", "raster_segments_bwd", "rasterize")


def install():
    """the forward restatements of tests/raster_ref.py and the three above in place of the ops -> what restore() needs"""
    import deepsvg_amd.ops as ops
    saved = RR.install()
    saved.update({n: getattr(ops, n) for n in NAMES if n not in saved})
    g = globals()
    for n in NAMES:
        setattr(ops, n, g[n])
    return saved


def restore(saved):
    RR.restore(saved)
