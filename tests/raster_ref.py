"""Float64 restatement of what an image is (include/dsvg.h, "Images of a decoded batch"), written from the definition and
not from the kernels' data layout: a Python walk over the rows of every sequence gives the chord list, and an image is a
[chords, H, W] broadcast in plain torch.  It is the oracle of tests/test_render_gpu.py, and on CPU - install() - the
emulated ops.raster_segments / ops.raster_sweep / ops.rasterize under deepsvg_amd.render (tests/test_render_host.py).

Geometry: `l` (1) and `c` (2) draw, nothing else does; the start point of row i is the end position (args 9:11) of row i - 1
whatever it holds, (0, 0) on row 0; a command gives n - 1 chords between the vertices at z = k / (n - 1), vertex 0 being the
start point and vertex n - 1 the end position themselves.  Fill mode closes every sub-path (a maximal run of consecutive
drawing rows) by one chord from its last vertex to its first.
Pixels: size x size over 0..256, pitch s = 256 / size, centre of (row r, column c) = ((c + 0.5) s, (r + 0.5) s).
Stroke: ink = clamp(0.5 + (w / 2 - d) / s, 0, 1), d the distance to the nearest chord; no chords: zeros.
Fill: inside = non-zero winding with respect to any one sequence (half-open rule on a ray towards +x); ink = clamp(0.5 + d / s,
0, 1) inside, clamp(0.5 - d / s, 0, 1) outside."""
import numpy as np
import torch

L_ID, C_ID = 1, 2
VIEW = 256.0


def chord_list(commands, args, n=10, groups=1, fill=False):
    """commands [B*groups, L], args [B*groups, L, 11] (any dtype) -> one dict per image, chords in drawing order:
    a, b float64 [C, 2]; seq int64 [C]: the sequence (group) a chord belongs to; back int64 [C]: on a closing chord the
    number of chords back to its sub-path's first chord, 0 elsewhere"""
    cmd = commands.detach().cpu().long().numpy()
    arg = args.detach().cpu().double().numpy()
    R, L = cmd.shape
    assert R % groups == 0
    z = (np.arange(n, dtype=np.float64) / (n - 1))[:, None]
    images = []
    for img in range(R // groups):
        a, b, seq, back = [], [], [], []
        count = 0
        for g in range(groups):
            row = img * groups + g
            sub_first, sub_index, last = None, 0, None          # the open sub-path: its first vertex, first chord, last vertex
            for i in range(L):
                draws = cmd[row, i] in (L_ID, C_ID)
                if draws:
                    start = arg[row, i - 1, 9:11] if i else np.zeros(2)
                    end = arg[row, i, 9:11]
                    if cmd[row, i] == L_ID:
                        v = start + z * (end - start)
                    else:
                        w = 1 - z
                        v = w ** 3 * start + 3 * w ** 2 * z * arg[row, i, 5:7] + 3 * w * z ** 2 * arg[row, i, 7:9] + z ** 3 * end
                    v[0], v[-1] = start, end
                    if sub_first is None:
                        sub_first, sub_index = start, count
                    last = end
                    a.append(v[:-1])
                    b.append(v[1:])
                    seq += [g] * (n - 1)
                    back += [0] * (n - 1)
                    count += n - 1
                if sub_first is not None and (not draws or i == L - 1):
                    if fill:
                        a.append(last[None])
                        b.append(sub_first[None])
                        seq.append(g)
                        back.append(count - sub_index)
                        count += 1
                    sub_first = None
        images.append({"a": torch.from_numpy(np.concatenate(a) if a else np.zeros((0, 2))),
                       "b": torch.from_numpy(np.concatenate(b) if b else np.zeros((0, 2))),
                       "seq": torch.tensor(seq, dtype=torch.int64), "back": torch.tensor(back, dtype=torch.int64)})
    return images


CHUNK = 256            # chords per [chords, H, W] broadcast


def image(a, b, seq, size, stroke_width=3.2, fill=False, dtype=torch.float64, return_distance=False):
    """chords a -> b ([C, 2]) of one image, seq [C] their sequences -> ink [size, size], every step in `dtype` (float64: the
    oracle; float32: the same formulas at the kernels' precision, tests/test_render_host.py)"""
    a, b = a.to(dtype), b.to(dtype)
    s = VIEW / size
    centre = (torch.arange(size, dtype=dtype) + 0.5) * s
    cx, cy = centre.view(1, 1, size), centre.view(1, size, 1)
    d2 = torch.full((size, size), float("inf"), dtype=dtype)
    inside = torch.zeros(size, size, dtype=torch.bool)
    for q in (torch.unique(seq).tolist() if fill else [None]):
        sel = slice(None) if q is None else seq == q
        aq, bq = a[sel], b[sel]
        wind = torch.zeros(size, size, dtype=torch.int64)
        for j in range(0, aq.shape[0], CHUNK):
            ax, ay = aq[j:j + CHUNK, 0].view(-1, 1, 1), aq[j:j + CHUNK, 1].view(-1, 1, 1)
            bx, by = bq[j:j + CHUNK, 0].view(-1, 1, 1), bq[j:j + CHUNK, 1].view(-1, 1, 1)
            dx, dy = bx - ax, by - ay
            len2 = dx * dx + dy * dy
            px, py = cx - ax, cy - ay
            t = torch.where(len2 > 0, (px * dx + py * dy) / torch.where(len2 > 0, len2, torch.ones_like(len2)),
                            torch.zeros_like(len2)).clamp(0, 1)
            qx, qy = px - t * dx, py - t * dy
            d2 = torch.minimum(d2, (qx * qx + qy * qy).amin(0))
            if fill:
                crossing = ax + (cy - ay) * dx / torch.where(dy != 0, dy, torch.ones_like(dy))          # x where the chord meets the row
                right = crossing > cx
                wind += ((ay <= cy) & (cy < by) & right).sum(0) - ((by <= cy) & (cy < ay) & right).sum(0)
        inside |= wind != 0
    d = d2.sqrt()
    if return_distance:
        return d, inside
    if fill:
        return torch.where(inside, 0.5 + d / s, 0.5 - d / s).clamp(0, 1)
    return (0.5 + (stroke_width / 2 - d) / s).clamp(0, 1)


def rasterize(commands, args, size=64, stroke_width=3.2, fill=False, n=10, groups=1, cull=None, as_double=False):
    """same contract as ops.rasterize (float64 inside, straight from the chord list)"""
    out = torch.stack([image(c["a"], c["b"], c["seq"], size, stroke_width, fill)
                       for c in chord_list(commands, args, n, groups, fill)])
    return out if as_double else out.float()


def records(chords):
    """the chord list of one image -> (f32 [C, 4]: ax, ay, bx - ax, by - ay of the fp32 vertices; int32 [C]: the flags word)"""
    a, b = chords["a"].float(), chords["b"].float()
    first = torch.ones_like(chords["seq"])
    first[1:] = chords["seq"][1:] != chords["seq"][:-1]
    return torch.cat([a, (b.double() - a.double()).float()], 1), (first | (chords["back"] << 1)).to(torch.int32)


def raster_segments(commands, args, n=10, groups=1, fill=False):
    """same contract as ops.raster_segments; records past seg_counts[b] are zero here"""
    lists = chord_list(commands, args, n, groups, fill)
    L = commands.shape[1]
    cap = groups * (L * (n - 1) + ((L + 1) // 2 if fill else 0))
    segs = torch.zeros(len(lists), max(cap, 1), 5)
    for i, c in enumerate(lists):
        r, f = records(c)
        segs[i, :len(f), :4] = r
        segs[i, :len(f), 4] = f.view(torch.float32)
    return segs, torch.tensor([len(c["seq"]) for c in lists], dtype=torch.int32)


def raster_sweep(segs, seg_counts, size=64, stroke_width=3.2, fill=False, cull=None):
    """same contract as ops.raster_sweep"""
    out = []
    for i in range(segs.shape[0]):
        r = segs[i, :int(seg_counts[i])]
        a = r[:, :2].double()
        seq = (r[:, 4].contiguous().view(torch.int32) & 1).long().cumsum(0)
        out.append(image(a, a + r[:, 2:4].double(), seq, size, stroke_width, fill))
    return torch.stack(out).float()


NAMES = ("raster_segments", "raster_sweep", "rasterize")


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
