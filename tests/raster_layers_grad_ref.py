"""Float64 restatement of the gradient of a layered image (include/dsvg.h, "Layered images: the gradient";
deepsvg_amd/csrc/raster.hip: dsvg_raster_sweep_layers_nn, dsvg_raster_blend_bwd, dsvg_raster_sweep_layers_bwd,
dsvg_raster_segments_layers_bwd), written from the definition on top of tests/raster_layers_ref.py (the picture) and
tests/raster_grad_ref.py (the nearest chord and its derivative).

Per pixel, over the layers that have chords in group order: C_0 = background, alpha_g = opacity_g cov_g, C_g = C_{g-1} + alpha_g
(p_g - C_{g-1}), out = C_K, with p_g the layer's colour or the background for ERASE.  With T_g = prod_{k > g} (1 - alpha_k),
carried down from the top layer (nothing is divided by 1 - alpha): d out_c / d alpha_g = T_g (p_g,c - C_{g-1,c}), d out_c / d p_g,c
= T_g alpha_g (ERASE and skipped layers: 0), d alpha / d cov = opacity, d alpha / d opacity = cov; a colour or an opacity given
outside 0..1 (the forward clamps it) or as NaN gets 0.  d cov / d d = -1 / s for OUTLINE and for FILL / ERASE where cov <= 0.5,
+1 / s for FILL / ERASE where cov > 0.5, 0 where the stored cov is 0 or 1; d d / d a, d d / d b as tests/raster_grad_ref.py, the
nearest chord taken among the layer's OWN chords, named by its index in the image.

A layer "has chords" as the kernel's walk decides it: its end (the next entry of layer_first clamped into 0..count, the count
for the last layer) lies past the end of every layer before it.

The ops TAKE cov, idx and dcov as given, as the kernels do: fed the kernels' own results they follow the kernels' choice of
nearest chord and of live pixels.  picture64 / picture_backward64 go from the ARGUMENTS in float64 with their own arg-min.
install() puts the restatements in place of the ops, on top of those of tests/raster_layers_ref.py and
tests/raster_grad_ref.py, so that the autograd wiring of deepsvg_amd.render runs on CPU."""
import numpy as np
import torch

from tests import raster_grad_ref as RG
from tests import raster_layers_ref as LR
from tests import raster_ref as RR

OUTLINE, FILL, ERASE = LR.OUTLINE, LR.FILL, LR.ERASE
L_ID, C_ID, VIEW = RR.L_ID, RR.C_ID, RR.VIEW


# ---- the layer table ----------------------------------------------------------------------------------------------------------
def layer_ranges(layer_first_i, count, NL, compound=None):
    """-> per layer (start, end) in records, (0, 0) for a layer the walk passes over"""
    if compound is not None:
        return [(0, int(count))] if int(count) > 0 else [(0, 0)]
    count, first = int(count), [int(v) for v in layer_first_i]
    out, reached = [], 0
    for g in range(NL):
        end = min(max(first[g + 1], 0), count) if g + 1 < NL else count
        if end > reached:
            out.append((reached, end))
            reached = end
        else:
            out.append((0, 0))
    return out


def layer_modes(modes_i, NL, compound=None):
    if compound is not None:
        return [FILL if compound == "fill" else OUTLINE]
    return [LR.norm_mode(modes_i[g]) for g in range(NL)]


def _records64(segs_i, count):
    r = segs_i[:int(count)].double()
    return r[:, :2], r[:, :2] + r[:, 2:4]


# ---- the four ops ---------------------------------------------------------------------------------------------------------------
def raster_sweep_layers_nn(segs, seg_counts, layer_first, modes, paint, background=(1.0, 1.0, 1.0), size=64, stroke_width=3.2,
                           evenodd=False, compound=None, cull=None):
    """same contract as ops.raster_sweep_layers_nn: the picture of LR.raster_sweep_layers, float64 coverage and arg-min"""
    out = LR.raster_sweep_layers(segs, seg_counts, layer_first, modes, paint, background=background, size=size,
                                 stroke_width=stroke_width, evenodd=evenodd, compound=compound)
    B, NL = segs.shape[0], 1 if compound else paint.shape[1]
    cov = torch.zeros(B, NL, size, size, dtype=torch.float32)
    idx = torch.full((B, NL, size, size), -1, dtype=torch.int32)
    for i in range(B):
        a, b = _records64(segs[i], seg_counts[i])
        mode = layer_modes(None if compound else modes[i], NL, compound)
        for g, (lo, hi) in enumerate(layer_ranges(None if compound else layer_first[i], seg_counts[i], NL, compound)):
            if hi > lo:
                c = LR.coverage(a[lo:hi], b[lo:hi], mode[g], size, stroke_width, evenodd).float()
                _, nn = RG.nearest(a[lo:hi], b[lo:hi], size)
                cov[i, g] = c
                idx[i, g] = torch.where((c > 0) & (c < 1), nn + lo, torch.full_like(nn, -1)).to(torch.int32)
    return out, cov, idx


def blend_bwd_pixels(cov, live, erase, paint, background, dout, dtype=torch.float64, sum_pixels=None):
    """one image: cov [NL, H, W], live / erase: lists of bool per layer, paint [NL, 4] as given, background three numbers, dout
    [3, H, W] -> (dcov [NL, H, W], dpaint [NL, 4]), every step in `dtype`; sum_pixels([k, H * W]) -> [k]: the sum over the pixels
    of an image (torch's sum unless given)"""
    sum_pixels = sum_pixels or (lambda t: t.sum(1))
    NL = cov.shape[0]
    cov, dout = cov.to(dtype), dout.to(dtype)
    rgba = LR.unit(paint, dtype)
    bg = LR.unit(background, dtype).view(3, 1, 1)
    canvas = bg.expand(3, *cov.shape[1:]).clone()
    slot = torch.zeros_like(cov)
    for g in range(NL):
        if not live[g]:
            continue
        p = bg if erase[g] else rgba[g, :3].view(3, 1, 1)
        slot[g] = (dout * (p - canvas)).sum(0)
        canvas = canvas + (rgba[g, 3] * cov[g]) * (p - canvas)
    dcov, dpaint = torch.zeros_like(cov), torch.zeros(NL, 4, dtype=dtype)
    T = torch.ones_like(cov[0])
    for g in reversed(range(NL)):
        if not live[g]:
            continue
        alpha = rgba[g, 3] * cov[g]
        dalpha = T * slot[g]
        dcov[g] = dalpha * rgba[g, 3]
        dpaint[g, 3] = sum_pixels((dalpha * cov[g]).flatten()[None])[0]
        if not erase[g]:
            dpaint[g, :3] = sum_pixels(((T * alpha) * dout).flatten(1))
        T = T - alpha * T
    given = torch.as_tensor(paint).to(dtype)
    return dcov, torch.where((given >= 0) & (given <= 1), dpaint, torch.zeros_like(dpaint))


def raster_blend_bwd(cov, seg_counts, layer_first, modes, paint, dout, cap, background=(1.0, 1.0, 1.0), compound=None,
                     dtype=torch.float64, as_double=False, sum_pixels=None):
    """same contract as ops.raster_blend_bwd"""
    B, NL = cov.shape[:2]
    dcov = torch.zeros(cov.shape, dtype=dtype)
    dpaint = torch.zeros(paint.shape, dtype=dtype)
    for i in range(B):
        count = min(max(int(seg_counts[i]), 0), int(cap))
        ranges = layer_ranges(None if compound else layer_first[i], count, NL, compound)
        mode = layer_modes(None if compound else modes[i], NL, compound)
        dcov[i], dpaint[i, :NL] = blend_bwd_pixels(cov[i], [hi > lo for lo, hi in ranges], [m == ERASE for m in mode],
                                                   paint[i, :NL].detach(), background, dout[i], dtype, sum_pixels)
    return (dcov, dpaint) if as_double else (dcov.float(), dpaint.float())


def raster_sweep_layers_bwd(segs, seg_counts, layer_first, modes, cov, idx, dcov, stroke_width=3.2, compound=None, wide=None,
                            dtype=torch.float64, as_double=False):
    """same contract as ops.raster_sweep_layers_bwd, with cov and idx as given; rows past the counts are zero here"""
    B, NL = cov.shape[:2]
    dsegs = torch.zeros(B, segs.shape[1], 4, dtype=dtype)
    for i in range(B):
        k = int(seg_counts[i])
        a, b = _records64(segs[i], k)
        mode = layer_modes(None if compound else modes[i], NL, compound)
        for g, (lo, hi) in enumerate(layer_ranges(None if compound else layer_first[i], k, NL, compound)):
            if hi > lo:
                own = torch.where((idx[i, g] >= lo) & (idx[i, g] < hi), idx[i, g], torch.full_like(idx[i, g], -1))
                da, db = RG.chords_bwd(a, b, cov[i, g], own, dcov[i, g], mode[g] != OUTLINE, dtype)
                dsegs[i, :k, :2] += da
                dsegs[i, :k, 2:] += db
    return dsegs if as_double else dsegs.float()


def raster_segments_layers_bwd(commands, dsegs, seg_counts, modes, n=10, groups=1, dtype=np.float64, as_double=False):
    """same contract as ops.raster_segments_layers_bwd: RG.raster_segments_bwd's walk with `fill` per group"""
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
            fill = LR.norm_mode(modes[img][g]) != OUTLINE
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
        assert count == int(seg_counts[img]), "dsegs was not built for these commands and modes"
    out = torch.from_numpy(dargs)
    return out if as_double else out.float()


# ---- from the arguments, in float64 ----------------------------------------------------------------------------------------------
def layer_vertices64(commands, args, modes, n=10, groups=1, compound=None):
    """the chord builder as differentiable torch, per layer: commands [B*groups, L], args float64 [B*groups, L, 11] (kept in
    the graph), modes [B][groups] -> per image a list over layers of (a, b float64 [C, 2], mode); closing chords where the
    layer's mode is FILL or ERASE; compound: one layer of all groups"""
    open_, closed = (RG.chord_vertices64(commands, args, n=n, groups=groups, fill=fill) for fill in (False, True))
    out = []
    for i in range(len(open_)):
        if compound is not None:
            src = closed[i] if compound == "fill" else open_[i]
            out.append([(src["a"], src["b"], FILL if compound == "fill" else OUTLINE)])
            continue
        layers = []
        for g in range(groups):
            mode = LR.norm_mode(modes[i][g])
            src = closed[i] if mode != OUTLINE else open_[i]
            sel = src["seq"] == g
            layers.append((src["a"][sel], src["b"][sel], mode))
        out.append(layers)
    return out


def picture64(commands, args, modes, paint, background=(1.0, 1.0, 1.0), size=64, stroke_width=3.2, evenodd=False, compound=None,
              n=10, groups=1):
    """float64 from the arguments -> (pictures float64 [B, 3, size, size], state for picture_backward64).  paint float64
    [B, groups, 4] as given (clamped here)"""
    per_image = layer_vertices64(commands, args.double(), modes, n, groups, compound)
    B, NL = len(per_image), 1 if compound else groups
    cov = torch.zeros(B, NL, size, size, dtype=torch.float64)
    idx = torch.full((B, NL, size, size), -1, dtype=torch.int64)
    out = []
    for i, layers in enumerate(per_image):
        lo = 0
        for g, (a, b, mode) in enumerate(layers):
            a, b = a.detach(), b.detach()
            if a.shape[0]:
                cov[i, g] = LR.coverage(a, b, mode, size, stroke_width, evenodd)
                idx[i, g] = RG.nearest(a, b, size)[1] + lo
            lo += a.shape[0]
        out.append(LR.paint_layers([(a.detach(), b.detach(), mode, paint[i, g].detach()) for g, (a, b, mode) in enumerate(layers)],
                                   background, size, stroke_width, evenodd))
    return torch.stack(out), (per_image, cov, idx)


def picture_backward64(commands, state, paint, dout, background=(1.0, 1.0, 1.0), compound=None, n=10, groups=1):
    """the restated backward in float64 on float64 chords with their own arg-min -> (dargs float64 [B*groups, L, 11], dpaint
    float64 [B, groups, 4])"""
    per_image, cov, idx = state
    B, NL = cov.shape[:2]
    cap = max(max(sum(a.shape[0] for a, _, _ in layers) for layers in per_image), 1)
    dsegs = torch.zeros(B, cap, 4, dtype=torch.float64)
    dpaint = torch.zeros(B, paint.shape[1], 4, dtype=torch.float64)
    counts, modes = [], []
    for i, layers in enumerate(per_image):
        a = torch.cat([ly[0].detach() for ly in layers])
        b = torch.cat([ly[1].detach() for ly in layers])
        dcov, dpaint[i, :NL] = blend_bwd_pixels(cov[i], [ly[0].shape[0] > 0 for ly in layers], [ly[2] == ERASE for ly in layers],
                                                paint[i, :NL].detach(), background, dout[i])
        for g, (_, _, mode) in enumerate(layers):
            da, db = RG.chords_bwd(a, b, cov[i, g], idx[i, g], dcov[g], mode != OUTLINE)
            dsegs[i, :a.shape[0], :2] += da
            dsegs[i, :a.shape[0], 2:] += db
        counts.append(a.shape[0])
        modes.append([ly[2] for ly in layers])
    counts = torch.tensor(counts, dtype=torch.int32)
    if compound is not None:
        return RG.raster_segments_bwd(commands, dsegs, counts, n=n, groups=groups, fill=compound == "fill", as_double=True), dpaint
    return raster_segments_layers_bwd(commands, dsegs, counts, modes, n=n, groups=groups, as_double=True), dpaint


# ---- in place of the ops ------------------------------------------------------------------------------------------------------------
def draw(commands, args, modes, paint, background=(1.0, 1.0, 1.0), size=64, stroke_width=3.2, evenodd=False, compound=None,
         n=10, groups=1, cull=None):
    """same contract as ops.draw, and composed as it is: records -> picture (LR.draw goes from the float64 chord lists to the
    picture and differs from this in the last bits)"""
    import deepsvg_amd.ops as ops
    if compound is None:
        segs, seg_counts, layer_first = ops.raster_segments_layers(commands, args, modes, n=n, groups=groups)
    else:
        segs, seg_counts = ops.raster_segments(commands, args, n=n, groups=groups, fill=compound == "fill")
        layer_first = None
    return ops.raster_sweep_layers(segs, seg_counts, layer_first, modes, paint, background=background, size=size,
                                   stroke_width=stroke_width, evenodd=evenodd, compound=compound)


NAMES = ("raster_sweep_layers_nn", "raster_blend_bwd", "raster_sweep_layers_bwd", "raster_segments_layers_bwd", "draw")


def install():
    """the restatements of tests/raster_grad_ref.py and tests/raster_layers_ref.py and the ones above in place of the ops (ops.draw_fwd_nn
    and ops.draw_bwd compose whatever stands in the module) -> what restore() needs"""
    import deepsvg_amd.ops as ops
    saved = RG.install()
    for name, fn in LR.install().items():
        saved.setdefault(name, fn)
    saved.update({n: getattr(ops, n) for n in NAMES if n not in saved})
    g = globals()
    for n in NAMES:
        setattr(ops, n, g[n])
    return saved


def restore(saved):
    RR.restore(saved)
