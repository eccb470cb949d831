"""Images of a decoded batch, on the device: the step from command sequences to pictures.  Every use the reference makes of
a trained model ends in ``SVG.from_tensor(...).draw(return_png=True)`` (deepsvg/svglib/svg.py:172-204): an SVG string handed to
cairosvg on the host, one icon at a time after a device -> host copy (``decode()`` of notebooks/interpolation.ipynb,
latent_ops.ipynb, animation.ipynb, fonts.ipynb; the trainer's visualisation hook, configs/deepsvg/default_icons.py:76-77).
Here the curves `metrics.sample_points` samples are rasterised by two launches of csrc/raster.hip for the whole batch.

What an image is (include/dsvg.h has the full definition, tests/raster_ref.py restates it in float64): `l` and `c` commands
become n - 1 chords each; the view box is 0..256 argument units (``Bbox(256)``), pixel (row r, column c) has its centre at
((c + 0.5) s, (r + 0.5) s) with s = 256 / size, y down.  Stroke mode (the reference's default): ink = clamp(0.5 +
(stroke_width / 2 - d) / s, 0, 1) with d the distance to the nearest chord.  Fill mode (no stroke, as
svglib/svg_primitive.py:34-38): every sub-path is closed, a pixel is inside an image when its non-zero winding number with
respect to any ONE sequence's chords is not 0, and ink = clamp(0.5 +- d / s, 0, 1).  No atomics: bit-reproducible.
`rasterize` carries no gradient; `rasterize_with_grad` draws the same bits and does (below).  Arcs are not drawn (the
reference's own sampler skips them).

Layered images (`draw`, `palette`; two more entry points of csrc/raster.hip, tests/raster_layers_ref.py restates them in
float64): the picture the reference shows for an icon - ``SVG.draw`` / ``draw_colored``, with the per-group `filling` of its
data path (svglib/svg_path.py:29-32: outline, fill, erase).  Group g of an icon is layer g, painted in group order onto a
canvas of three channels: its coverage is the stroke or fill coverage above computed from the group's OWN chords (fill rule
non-zero or even-odd), alpha = opacity * coverage, canvas = fmaf(alpha, paint - canvas, canvas) per channel, where paint is
the group's colour or, for an erase layer, the background - so the counter of an "O", a group of its own since
`paths.canonicalize`, is a hole again.  ``compound=True`` draws an icon as one <path> with many sub-paths instead.  `draw`
itself carries no gradient: `draw_with_grad` draws the same bits and does (last paragraph).  The dash arrays and the point /
handle / box extras of the reference's ``draw`` are not drawn.

The gradient of an image with respect to float32 `args` (`rasterize_with_grad`, `image_loss`, `refine_to_images`; three
more kernels of csrc/raster.hip, tests/raster_grad_ref.py restates them in float64): a pixel's ink depends on the chords only
through d, the distance to its nearest chord a -> b with the closest point at the clamped parameter t and q = p - (a + t
(b - a)): d d / d a = -(1 - t) q / d, d d / d b = -t q / d; d ink / d d = -1 / s (stroke, and fill outside), +1 / s (fill inside,
ink > 0.5), 0 where ink is clamped; the winding number is piecewise constant and carries none.  Of chords at equal fp32
d^2 the one with the lowest index takes the term; a pixel with d == 0 contributes nothing (in fill mode the limit exists but
needs an orientation the sweep does not carry: a shape whose unsaturated pixels all sit ON the outline, like the integer
square of INTEGRATION.md section 6 at size 64, has an exactly zero gradient); saturation is read from the stored image.
Chord vertices are linear in `args`; the start point of a command is the end position of the row before it whatever that
row holds, and columns 0-4, padding and rows that neither draw nor precede a drawing row get exact zeros.  A gather with
an arg-min saved by the forward: no atomics, bit-reproducible.

The gradient of a layered image (`draw_with_grad`, `picture_loss`, `refine_to_pictures`; four more entry points of
csrc/raster.hip, tests/raster_layers_grad_ref.py restates them in float64): with T_g the product of 1 - alpha_k over the layers
above g, d out / d alpha_g = T_g (paint_g - canvas_{g-1}), d out / d paint_g = T_g alpha_g (0 for an erase layer), d alpha / d cov =
opacity and d alpha / d opacity = cov; T is carried down from the top layer, so nothing is divided by 1 - alpha (0 inside an
opaque fill).  A layer's coverage reaches the arguments as above, through the nearest chord among the layer's OWN chords: the
hole of a ring pulls on its own outline.  Colours and opacities the kernel clamped get an exact 0.  The pixel sums of the paint
gradient run in a fixed order: bit-reproducible.
"""
import torch

from . import ops
from .metrics import _adam_refine, _evaluating, _flat_sequences

__all__ = ["rasterize", "draw", "palette", "rasterize_with_grad", "image_loss", "refine_to_images", "draw_with_grad",
           "picture_loss", "refine_to_pictures", "reconstruction_images", "interpolate", "interpolation_alphas"]


def rasterize(commands, args, size=64, stroke_width=3.2, fill=False, n=10):
    """commands [N, S] -> one image per row; commands [N, G, S] -> one image per icon, all its groups drawn; args [..., S, 11].
    float32 (as the dataset delivers them) and int64 (as greedy_sample returns them) are read as they are.
    -> f32 [N, size, size], 1 = ink, 0 = paper.  `stroke_width` is in argument units (3.2 of 256 = the reference's .3 of a
    24-unit view box); `fill` draws filled shapes without a stroke; `n` points per command, as sample_points.  Inputs are
    detached: no gradient.

    One image per group (the layers ``draw_colored`` gives random colours) comes from flattening the groups; composing them
    is one line of torch::

        layers = rasterize(commands.reshape(N * G, S), args.reshape(N * G, S, 11), fill=True).view(N, G, 1, size, size)
        rgb = 1 - (layers * (1 - torch.rand(N, G, 3, 1, 1, device=layers.device))).amax(1)          # [N, 3, size, size]

    `draw` paints the groups over each other in one sweep, with per-group outline / fill / erase, colours and opacities.
    """
    commands, args, groups = _flat_sequences("rasterize", commands.detach(), args.detach())
    return ops.rasterize(commands, args, size=size, stroke_width=stroke_width, fill=fill, n=n, groups=groups)


def _unit_numbers(name, what, values):
    """Python numbers in 0..1 -> list of float; anything else is refused under the caller's name"""
    values = [float(v) for v in values]
    if not all(0.0 <= v <= 1.0 for v in values):          # (a NaN fails both comparisons)
        raise ValueError(f"{name}: {what} in 0..1; got {values}")
    return values


def _per_group(name, what, value, N, G, last, device, keep_graph=False):
    """a table given per group ([G, *last]) or per icon and group ([N, G, *last]) -> float32, broadcastable to [N, G, *last];
    Python lists are checked against 0..1, tensors are left to the kernel's clamp (and detached unless `keep_graph`)"""
    if not torch.is_tensor(value):
        flat = torch.tensor(value, dtype=torch.float32)
        _unit_numbers(name, what, flat.flatten().tolist())
        value = flat
    value = (value if keep_graph else value.detach()).to(device=device, dtype=torch.float32)
    if tuple(value.shape) not in ((G, *last), (N, G, *last)):
        raise ValueError(f"{name}: {what} {[G, *last]} or {[N, G, *last]}; got {list(value.shape)}")
    return value


def draw(commands, args, filling=None, colors=None, opacity=1.0, background=1.0, size=64, stroke_width=3.2, fill=False,
         fill_rule="nonzero", compound=False, n=10):
    """The groups of every icon painted one over the other into ONE RGB image, the way the reference displays an icon
    (``SVG.draw``, ``draw_colored``): commands [N, G, S] / args [N, G, S, 11] ([N, S] / [N, S, 11]: G = 1), read, detached and
    sampled exactly as `rasterize` does -> f32 [N, 3, size, size], 1 = paper white, 0 = black.  No gradient (`draw_with_grad`).

    Group g is layer g; layers are painted in group order onto a canvas that starts at `background` (a number or three, in
    0..1); a group without chords is skipped.
    `filling`: int [N, G] or [N, G, 1] as the data sets deliver it (``model_args`` with "filling"): 1 = FILL, 2 = ERASE, any
    other value = OUTLINE; None: every layer OUTLINE, or FILL with ``fill=True``.  It is neither read back nor validated.
    Coverage of a layer, with d the distance to the nearest chord of ITS group: OUTLINE clamp(0.5 + (stroke_width / 2 - d) / s,
    0, 1); FILL and ERASE close every sub-path of the group, inside = winding number != 0 (`fill_rule` "nonzero") or odd
    ("evenodd"), clamp(0.5 +- d / s, 0, 1).
    Paint: `colors` None (black), [G, 3] or [N, G, 3]; `opacity` a number, [G] or [N, G]; alpha = opacity * coverage, and per
    channel canvas = fmaf(alpha, paint - canvas, canvas) with paint = the layer's colour, or `background` for an ERASE layer
    (the hole of a ring: INTEGRATION.md section 6).  Python numbers outside 0..1 raise ValueError; tensors are clamped by the
    kernel (NaN as 0) and not read back.
    `compound`: all groups of an icon as ONE layer, the way a single <path> with many sub-paths is drawn - winding counted
    across the groups, the mode from `fill`, the paint group 0's.  With ``fill=True, fill_rule="evenodd"`` it draws the holes
    of decoded output, which carries no `filling`.  Not together with `filling`.
    A one-group black-on-white image is ``1 - rasterize(...)`` bit for bit."""
    commands, args, G, modes, paint, background = _draw_inputs("draw", commands, args.detach(), filling, colors, opacity,
                                                               background, fill, fill_rule, compound)
    return ops.draw(commands, args, modes, paint, background=background, size=size, stroke_width=stroke_width,
                    evenodd=fill_rule == "evenodd", compound=("fill" if fill else "stroke") if compound else None, n=n, groups=G)


def _draw_inputs(name, commands, args, filling, colors, opacity, background, fill, fill_rule, compound, keep_graph=False):
    """the checks and tables of `draw`, under the caller's name -> (commands [N * G, S], args [N * G, S, 11], G, modes int32
    [N, G] or None (compound), paint f32 [N, G, 4], background: three floats).  `keep_graph`: `colors` / `opacity` tensors
    stay in the autograd graph, expanded to [N, G, ...] there (so that a per-group table sums its gradient over the icons)"""
    commands, args, G = _flat_sequences(name, commands.detach(), args)
    N, device = commands.shape[0] // G, commands.device
    if fill_rule not in ("nonzero", "evenodd"):
        raise ValueError(f"{name}: fill_rule 'nonzero' or 'evenodd'; got {fill_rule!r}")
    if compound and filling is not None:
        raise ValueError(f"{name}: compound=True draws one layer whose mode is `fill`; it takes no `filling`")
    background = _unit_numbers(name, "background", [background] * 3 if isinstance(background, (int, float)) else background)
    if len(background) != 3:
        raise ValueError(f"{name}: background is a number or three; got {len(background)} values")
    rgb = 0.0 if colors is None else _per_group(name, "colors", colors, N, G, (3,), device, keep_graph)
    opaque = (_unit_numbers(name, "opacity", [opacity])[0] if isinstance(opacity, (int, float))
              else _per_group(name, "opacity", opacity, N, G, (), device, keep_graph))
    if keep_graph and any(torch.is_tensor(t) and t.requires_grad for t in (rgb, opaque)):
        rgb = rgb if torch.is_tensor(rgb) else torch.full((), rgb, dtype=torch.float32, device=device)
        opaque = opaque if torch.is_tensor(opaque) else torch.full((), opaque, dtype=torch.float32, device=device)
        paint = torch.cat([rgb.expand(N, G, 3), opaque.expand(N, G).unsqueeze(-1)], -1)
    else:
        paint = torch.empty(N, G, 4, dtype=torch.float32, device=device)
        paint[..., :3] = rgb
        paint[..., 3] = opaque
    modes = None
    if not compound:
        if filling is None:
            modes = torch.full((N, G), 1 if fill else 0, dtype=torch.int32, device=device)
        else:
            if not torch.is_tensor(filling) or filling.is_floating_point() or tuple(filling.shape) not in ((N, G), (N, G, 1)):
                raise ValueError(f"{name}: filling is an int tensor {[N, G]} or {[N, G, 1]}; got "
                                 f"{tuple(filling.shape) if torch.is_tensor(filling) else type(filling).__name__}")
            modes = filling.detach().reshape(N, G).to(device=device, dtype=torch.int32).contiguous()
    return commands, args, G, modes, paint, background


def palette(G, device=None):
    """G distinct colours for ``draw_colored``-style pictures -> f32 [G, 3]: hues evenly spaced around the colour circle from
    a fixed start, at saturation 0.7 and value 0.85 (dark enough to read on white paper)"""
    hue = (torch.arange(G, dtype=torch.float32) / max(G, 1) + 0.58) % 1.0
    k = (torch.tensor([5.0, 3.0, 1.0]).view(1, 3) + hue.view(-1, 1) * 6.0) % 6.0
    rgb = 0.85 * (1.0 - 0.7 * torch.minimum(torch.minimum(k, 4.0 - k), torch.ones(())).clamp(min=0.0))
    return rgb.to(device) if device is not None else rgb


class _Rasterize(torch.autograd.Function):
    """raster_segments -> raster_sweep_nn; backward raster_sweep_bwd -> raster_segments_bwd"""

    @staticmethod
    def forward(ctx, commands, args, size, stroke_width, fill, n, groups):
        segs, seg_counts = ops.raster_segments(commands, args, n=n, groups=groups, fill=fill)
        out, idx = ops.raster_sweep_nn(segs, seg_counts, size=size, stroke_width=stroke_width, fill=fill)
        ctx.save_for_backward(commands, segs, seg_counts, out, idx)
        ctx.raster = (stroke_width, fill, n, groups)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        commands, segs, seg_counts, out, idx = ctx.saved_tensors
        stroke_width, fill, n, groups = ctx.raster
        dsegs = ops.raster_sweep_bwd(segs, seg_counts, out, idx, dout.contiguous(), stroke_width=stroke_width, fill=fill)
        dargs = ops.raster_segments_bwd(commands, dsegs, seg_counts, n=n, groups=groups, fill=fill)
        return None, dargs, None, None, None, None, None


def rasterize_with_grad(commands, args, size=64, stroke_width=3.2, fill=False, n=10):
    """`rasterize` for float32 `args` that receive a gradient: the same shapes, the same image bit for bit, and
    d image / d args flows back (module docstring: formulas and conventions).  `commands` of any dtype are read as float32;
    the backward is not differentiable again."""
    commands, flat_args, groups = _flat_sequences("rasterize_with_grad", commands.detach(), args)
    if args.dtype != torch.float32:
        raise ValueError(f"rasterize_with_grad: float32 args (integer arguments have no gradient); got {args.dtype}")
    return _Rasterize.apply(commands, flat_args, int(size), float(stroke_width), bool(fill), int(n), groups)


def image_loss(commands, args, target_images, **raster):
    """Mean squared ink difference between the images of `commands` / `args` and `target_images` f32 [N, size, size] (the size
    is the target's) -> {"loss": 0-d, the batch mean; "per_icon": [N]}.  Differentiable with respect to float32 `args`.
    `raster`: stroke_width, fill, n of `rasterize`."""
    if target_images.dim() != 3 or target_images.shape[-1] != target_images.shape[-2]:
        raise ValueError(f"image_loss: target_images (N, size, size); got {tuple(target_images.shape)}")
    images = rasterize_with_grad(commands, args, size=target_images.shape[-1], **raster)
    if images.shape != target_images.shape:
        raise ValueError(f"image_loss: {images.shape[0]} images against {target_images.shape[0]} targets")
    per_icon = (images - target_images.detach().to(images.dtype)).pow(2).flatten(1).mean(1)
    return {"loss": per_icon.mean(), "per_icon": per_icon}


def refine_to_images(commands, args, target_images, steps=150, lr=0.1, **raster):
    """The Adam loop of `metrics.refine` against pictures instead of point clouds: minimises `image_loss` on a float32 copy of
    `args` -> (refined args f32, history f32 [steps]: the loss before each step, kept on the device - the loop reads nothing
    back).  `target_images`: one tensor [N, size, size], or a list of such tensors of different sizes whose losses are summed.
    The gradient is local: only pixels within about one pixel of the outline (where ink is not saturated) pull on it, so the
    outline has to start within a pixel or so of where the target has ink to be drawn to it.  A coarse target widens that
    basin (a pixel of a 16 x 16 image is 16 argument units); a list from coarse to fine gives both reach and precision.
    Elements whose gradient is always zero (columns 0-4, padding, rows that neither draw nor precede a drawing row) come
    back as they went in."""
    targets = [target_images] if torch.is_tensor(target_images) else list(target_images)
    if not targets:
        raise ValueError("refine_to_images: no target images")

    def batch_loss(refined):
        value = image_loss(commands, refined, targets[0], **raster)["loss"]
        for target in targets[1:]:
            value = value + image_loss(commands, refined, target, **raster)["loss"]
        return value

    return _adam_refine(args, steps, lr, batch_loss)


class _Draw(torch.autograd.Function):
    """ops.draw_fwd_nn (segments -> raster_sweep_layers_nn); backward ops.draw_bwd (raster_blend_bwd -> raster_sweep_layers_bwd ->
    the transpose of the chord builder)"""

    @staticmethod
    def forward(ctx, commands, args, paint, modes, background, size, stroke_width, evenodd, compound, n, groups):
        paint = paint.contiguous()
        out, saved = ops.draw_fwd_nn(commands, args, modes, paint, background=background, size=size, stroke_width=stroke_width,
                                     evenodd=evenodd, compound=compound, n=n, groups=groups)
        segs, seg_counts, layer_first, cov, idx = saved
        ctx.save_for_backward(commands, paint, modes, segs, seg_counts, layer_first, cov, idx)
        ctx.draw = (background, stroke_width, compound, n, groups)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        commands, paint, modes, *saved = ctx.saved_tensors
        background, stroke_width, compound, n, groups = ctx.draw
        dargs, dpaint = ops.draw_bwd(commands, modes, paint, tuple(saved), dout.contiguous(), background=background,
                                     stroke_width=stroke_width, compound=compound, n=n, groups=groups)
        return (None, dargs, dpaint) + (None,) * 8


def draw_with_grad(commands, args, filling=None, colors=None, opacity=1.0, background=1.0, size=64, stroke_width=3.2, fill=False,
                   fill_rule="nonzero", compound=False, n=10):
    """`draw` for inputs that receive a gradient: the same arguments, the same checks and the same picture bit for bit, and
    d picture / d args flows back to float32 `args`, d picture / d colors to a `colors` tensor that requires grad ([G, 3] or
    [N, G, 3]) and d picture / d opacity to an `opacity` tensor that requires grad ([G] or [N, G]); a per-group table receives
    the sum over the icons.  The formulas are in the module docstring and in include/dsvg.h ("Layered images: the
    gradient"): a colour or an opacity outside 0..1 is clamped by the kernel and gets an exact 0, as do the colours of ERASE
    layers and of groups without chords; `filling` and the winding number carry none.  `commands` of any dtype are read as
    float32; the backward is not differentiable again."""
    name = "draw_with_grad"
    if args.dtype != torch.float32:
        raise ValueError(f"{name}: float32 args (integer arguments have no gradient); got {args.dtype}")
    commands, flat_args, G, modes, paint, background = _draw_inputs(name, commands, args, filling, colors, opacity, background,
                                                                    fill, fill_rule, compound, keep_graph=True)
    return _Draw.apply(commands, flat_args, paint, modes, tuple(background), int(size), float(stroke_width),
                       fill_rule == "evenodd", ("fill" if fill else "stroke") if compound else None, int(n), G)


def picture_loss(commands, args, target_pictures, **draw):
    """Mean squared difference between the pictures of `commands` / `args` and `target_pictures` f32 [N, 3, size, size] (the size
    is the target's) -> {"loss": 0-d, the batch mean; "per_icon": [N]}.  Differentiable with respect to float32 `args`, and
    to `colors` / `opacity` tensors that require grad.  `draw`: every other argument of `draw_with_grad`."""
    if target_pictures.dim() != 4 or target_pictures.shape[1] != 3 or target_pictures.shape[-1] != target_pictures.shape[-2]:
        raise ValueError(f"picture_loss: target_pictures (N, 3, size, size); got {tuple(target_pictures.shape)}")
    pictures = draw_with_grad(commands, args, size=target_pictures.shape[-1], **draw)
    if pictures.shape != target_pictures.shape:
        raise ValueError(f"picture_loss: {pictures.shape[0]} pictures against {target_pictures.shape[0]} targets")
    per_icon = (pictures - target_pictures.detach().to(pictures.dtype)).pow(2).flatten(1).mean(1)
    return {"loss": per_icon.mean(), "per_icon": per_icon}


def refine_to_pictures(commands, args, target_pictures, steps=150, lr=0.1, **draw):
    """`refine_to_images` against layered pictures: the Adam loop minimises `picture_loss` on a float32 copy of `args` ->
    (refined args f32, history f32 [steps]: the loss before each step, kept on the device).  `target_pictures`: one tensor
    [N, 3, size, size], or a list of such tensors of different sizes (coarse to fine) whose losses are summed.  With a
    `filling` that erases, the outline of a hole is pulled on like any other: what `image_loss(fill=True)`, which paints holes
    over, cannot see.  The gradient is as local as that of `refine_to_images`.  Elements whose gradient is always zero (columns
    0-4, padding, rows that neither draw nor precede a drawing row) come back as they went in."""
    targets = [target_pictures] if torch.is_tensor(target_pictures) else list(target_pictures)
    if not targets:
        raise ValueError("refine_to_pictures: no target pictures")

    def batch_loss(refined):
        value = picture_loss(commands, refined, targets[0], **draw)["loss"]
        for target in targets[1:]:
            value = value + picture_loss(commands, refined, target, **draw)["loss"]
        return value

    return _adam_refine(args, steps, lr, batch_loss)


def reconstruction_images(model, commands, args, label=None, size=64, temperature=0.0, **raster):
    """Decode `commands` / `args` with ``model.greedy_sample`` (as `metrics.reconstruction_error` does: eval mode, no
    gradients, ``concat_groups=False``) and draw the decoded icons next to the targets, taken exactly as passed.
    -> {"decoded": f32 [N, size, size], "target": f32 [N, size, size]}.  `raster`: stroke_width, fill, n of `rasterize`.
    The model's train / eval state is restored."""
    with _evaluating(model):
        commands_y, args_y = model.greedy_sample(commands, args, commands, args, label=label, concat_groups=False,
                                                 temperature=temperature)
        decoded = rasterize(commands_y, args_y, size=size, **raster)
        target = rasterize(commands, args, size=size, **raster)
    return {"decoded": decoded, "target": target}


def interpolation_alphas(steps, ease=True, device=None):
    """linspace(0, 1, steps), through the notebooks' ease-in-out t^2 / (2 (t^2 - t) + 1) when `ease` is set -> f32 [steps]"""
    t = torch.linspace(0, 1, steps, device=device)
    return t * t / (2 * (t * t - t) + 1) if ease else t


def interpolate(model, z1, z2, steps=25, ease=True, label=None, size=64, temperature=0.0, **raster):
    """The interpolation loop of the notebooks (``interpolate`` / ``decode`` of notebooks/interpolation.ipynb) for a whole
    batch: z = (1 - a) z1 + a z2 for the `steps` values a of `interpolation_alphas`, ONE ``greedy_sample(z=...)`` call over
    all N * steps latents, one `rasterize`.  z1 / z2: the latents of N icons in either layout the model hands out, batch-first
    (N, 1, 1, dim_z) or the seq-first (1, 1, N, dim_z) of ``encode_mode=True``.  `label` [N], if the model takes one, is
    repeated for every frame.  -> {"frames": f32 [N, steps, size, size], "commands": int64 [N, steps, G, S], "args": int64
    [N, steps, G, S, 11]}: frame 0 is the icon of z1, the last frame that of z2.  Eval mode, no gradients; the model's
    train / eval state is restored."""
    if z1.shape != z2.shape or z1.dim() != 4 or not (z1.shape[1] == 1 and (z1.shape[0] == 1 or z1.shape[2] == 1)):
        raise ValueError(f"interpolate: z1 and z2 both (N, 1, 1, dim_z) or both (1, 1, N, dim_z); got {tuple(z1.shape)} and "
                         f"{tuple(z2.shape)}")
    dim_z = z1.shape[-1]
    za, zb = z1.detach().reshape(-1, 1, dim_z), z2.detach().reshape(-1, 1, dim_z)
    N = za.shape[0]
    a = interpolation_alphas(steps, ease, device=za.device).to(za.dtype).view(1, steps, 1)
    z = ((1 - a) * za + a * zb).reshape(N * steps, 1, 1, dim_z)
    if label is not None:
        label = label.repeat_interleave(steps, dim=0)
    with _evaluating(model):
        commands_y, args_y = model.greedy_sample(None, None, None, None, label=label, z=z, concat_groups=False,
                                                 temperature=temperature)
        frames = rasterize(commands_y, args_y, size=size, **raster)
    return {"frames": frames.view(N, steps, size, size), "commands": commands_y.reshape(N, steps, *commands_y.shape[1:]),
            "args": args_y.reshape(N, steps, *args_y.shape[1:])}
