"""The canonical form of a batch of icons, on the device: the way back into the model.  The encoder was trained on icons the
reference preprocessed with ``SVG.canonicalize()`` followed by ``numericalize(256)`` (deepsvg/svglib/svg.py:333-349, 392-394):
one sub-path per group, degenerate commands dropped, closed paths started at their top-left-most command, groups sorted top
to bottom then left to right, clockwise orientation, no `z`, integer coordinates.  What `metrics.refine` /
`render.refine_to_images` hand back (float arguments that have drifted), what ``greedy_sample`` decodes (any order and
orientation, several `m` in a group, stray `z`) and what a user assembles by hand (notebooks/animation.ipynb: ``permute`` and
``reverse`` by hand) are generally not in that form.  The reference canonicalises on the host, one icon at a time through Python
objects; `canonicalize` is one launch of csrc/paths.hip for the whole batch.  Every output value is a copy of an input value
- only the decisions are computed - so tests/golden/paths/ compares with the reference's own results by equality.

The definition (include/dsvg.h; tests/paths_ref.py restates it in float64):
 1. rows: a group ends at its first EOS; the start point of a command is the end position (args 9:11) of the row before it;
    rows before the group's first `m` are ignored; an `m` opens a sub-path and ends the one before it; a `z` marks the open
    sub-path closed and ends it, rows after it are ignored until the next `m`.  Every sub-path becomes a group of its own, in
    reading order.
 2. an `l` / `c` whose start and end are close (|s - e| <= 1e-8 + 1e-5 |e| in both coordinates) is dropped - a Bezier loop
    that returns to its start too; a sub-path left without commands disappears.
 3. closed sub-paths are rotated to start at their top-left-most command: a running best over the commands in order, command
    i (start p) replacing the best (start q) when p.y == q.y ? p.x < q.x : (p.y < q.y or (the fp32 norms of p and q are close
    and p.x < q.x)).  As in the reference NO closing line is inserted: a closed sub-path whose last end is not its first start
    keeps its rows, and the gap the `z` drew is lost.
 4. sub-paths are sorted by (start.y, start.x) of their first command, stable in reading order - BEFORE step 5, so the result
    is generally not sorted by its final start points (the data sets were built this way).
 5. a sub-path of one command is clockwise when (start.x, start.y) <= (end.x, end.y), any other when the sum of start.x end.y
    - start.y end.x over its commands is >= 0; one that is not is reversed (commands in reverse order, start and end swapped,
    the control points of a `c` swapped).
 6. rows out: `m` with the first command's start, `l` with its end, `c` with control1, control2, end; never a `z`.
 7. numericalize=n: every enabled slot of the written rows becomes clip(round_half_even(v), 0, n - 1) after all decisions, which
    are taken on the raw values; nothing is filtered again after rounding (the reference's data path does not either).  This is
    ``Point.numericalize`` (svglib/geom.py:182-183) without the view-box rescale of ``SVG.numericalize``: arguments are taken
    to be in the 0..256 box already, as everywhere in this package.
The op is not idempotent in general (steps 4 and 5).  Arcs are out of scope, as in `metrics.sample_points` and the rasteriser.
`arcs_to_beziers` below removes them first: it turns every `a` into `c` rows, after which all three accept the icon.

`split` and `arcs_to_beziers` are the two steps of the reference's preprocessing chain in which a command becomes several
(``SVGPath.split``, svglib/svg_path.py:615-630, first and last step of ``simplify_heuristic``; ``SVGPath.simplify_arcs``,
svg_path.py:280-293): one launch of csrc/paths_expand.hip for the whole batch.  include/dsvg.h has their definition,
tests/paths_expand_ref.py restates it in float64.

`simplify` is the Bezier fit between the reference's two splits (``SVGPath.simplify``, svg_path.py:391-613: Schneider's curve
fit with Newton reparametrisation on the smooth stretches of a path, Ramer-Douglas-Peucker on the rest): one launch of
csrc/paths_simplify.hip for the whole batch; include/dsvg.h has its definition, tests/paths_simplify_ref.py restates it in
float64.  `simplify_heuristic` is ``SVGPath.simplify_heuristic`` (svg_path.py:386-389) as three launches.  The chain back into
the model, as every data set was preprocessed, is
``arcs_to_beziers -> simplify_heuristic -> canonicalize(numericalize=256)``, all of it on the device.

`transform` is the affine map at both ends of that chain, a program of float32 steps in one launch of
csrc/paths_transform.hip (include/dsvg.h has its definition, tests/paths_transform_ref.py restates it in numpy float32, and
tests/golden/paths/transform.npz compares with the reference by equality): `normalize` and `zoom` before it
(``svg.normalize().zoom(0.9)``, svg_dataset.py:112-116), `augment` with ``numericalize`` behind it (``SVGDataset._augment``
and ``SVG.numericalize(256)``, svg_dataset.py:137-156).  The whole chain of the reference's on-the-fly data set is then
``svgio.load_svgs -> arcs_to_beziers -> normalize(viewbox, 24) -> zoom(0.9, viewbox=24) -> canonicalize ->
simplify_heuristic(unit=1) -> dataset.PackedSVGStore.from_batch(viewbox=24) -> svg_dataset.SVGDataset.batch``, the first
link reading the text of SVG files on the device (`deepsvg_amd.svgio`, which also composes the links up to the store as
`svgio.preprocess` / `svgio.preprocess_files`), the last link drawing fresh augmentation parameters on the device for every
batch and applying them while it assembles the model's tensors.

`compute_filling` gives a decoded batch the per-group ``filling`` (0 = OUTLINE, 1 = FILL, 2 = ERASE) that `render.draw`,
``PackedSVGStore.from_batch`` and ``SVGDataset`` take and that tensors do not carry: ``SVGPathGroup.compute_filling`` over
``overlap_graph`` (svglib/svg_primitive.py:392-441), which ``SVG.canonicalize_new`` runs on all sub-paths of an icon
(svg.py:312-331).  The reference measures overlap with shapely polygons on the host, one icon at a time; `overlap` is this
package's own measure: sample counts on the rasteriser's chord records and crossing rule, one launch of csrc/paths_fill.hip
behind the rasteriser's segment pass.  A third launch walks the cover graph of every icon.  include/dsvg.h has the
definition, tests/paths_fill_ref.py restates it in float64, and tests/golden/paths/filling.npz holds the reference's own
walk on given graphs.  The chain for decoded output is ``greedy_sample -> canonicalize -> compute_filling -> render.draw``.
Out of scope: ``SVG.group_overlapping_paths`` (the regrouping into groups of several sub-paths; "parent" and "depth" are what
it needs), arcs, and any change to `draw` itself.
"""
import math

import numpy as np
import torch

from . import ops
from .svgtensor import CMD_ARGS_MASK, C_ID

__all__ = ["canonicalize", "numericalize", "split", "arcs_to_beziers", "simplify", "simplify_heuristic", "transform", "zoom",
           "rotate", "translate", "normalize", "augment", "augment_params", "overlap", "compute_filling"]

MAX_ROWS = 2048      # G * S rows per icon: the largest icon the model accepts in a two-stage config, 8 groups of 256
MAX_STEPS = 16       # steps of one `transform`
MAX_FILL_GROUPS = 32                 # groups per icon of `overlap` / `compute_filling`: one mask word
MIN_SAMPLES, MAX_SAMPLES = 8, 1024   # samples per side of `overlap`


def canonicalize(commands, args, max_num_groups=None, max_seq_len=None, layout="grouped", numericalize=None):
    """commands (N, G, S) with args (N, G, S, 11), or (N, S) with (N, S, 11) - read as G = 1, the one-stage layout with several
    `m` in a sequence.  float32 (dataset, `refine`) and int64 (``greedy_sample``) are read as they are, anything else as
    float32 (int64 arguments are compared as float32: exact below 2^24).  Inputs are detached; there is no gradient (the op is
    piecewise constant in its decisions).  -> a dict, in the dtype read:
      layout="grouped": "commands" (N, G_out, S_out), "args" (N, G_out, S_out, 11) as `dataset.batch` delivers commands_grouped /
        args_grouped: a group in use is SOS, m, ..., EOS...; an unused one SOS, EOS...; every slot CMD_ARGS_MASK does not
        enable is -1.  G_out = max_num_groups (default G; required for 2-D input), S_out = max_seq_len + 2 (default S).
      layout="concat": "commands" (N, S_out), "args" (N, S_out, 11): SOS, all groups' rows back to back (each begins with its
        `m`), EOS...: the dataset's `commands` / `args`.  max_seq_len is the total length here; max_num_groups still bounds
        the number of sub-paths.
      "n_groups" int32 [N]; "len_groups" int32 [N, G_out]: rows of each output group, its `m` included, 0 where unused;
      "source_group" int32 [N, G_out]: the input group an output group came from, -1 where unused (per-group side data such as
        `filling` follows with one gather); "reversed" bool [N, G_out]; "valid" bool [N].
    An icon is invalid when it has more surviving sub-paths than G_out, when a sub-path (concat: all of them together) does not
    fit S_out - 2 rows, or when it holds an `a` before its group's first EOS; it comes back as all-unused groups with n_groups
    = 0 (as ``filter_meta`` drops such icons).  A closed sub-path whose last end is not its first start keeps its rows: the
    reference inserts no closing line, and the gap is lost (module docstring, step 3)."""
    if commands.dim() not in (2, 3) or args.dim() != commands.dim() + 1 or args.shape[:-1] != commands.shape \
            or args.shape[-1] != 11:
        raise ValueError(f"canonicalize: commands (N, G, S) with args (N, G, S, 11), or (N, S) with (N, S, 11); got "
                         f"{tuple(commands.shape)} and {tuple(args.shape)}")
    if layout not in ("grouped", "concat"):
        raise ValueError(f"canonicalize: layout 'grouped' or 'concat'; got {layout!r}")
    if commands.dim() == 2:
        if max_num_groups is None:
            raise ValueError("canonicalize: max_num_groups is required for (N, S) input")
        commands, args = commands.unsqueeze(1), args.unsqueeze(1)
    N, G, S = commands.shape
    if N < 1:
        raise ValueError("canonicalize: an empty batch")
    if G * S > MAX_ROWS:
        raise ValueError(f"canonicalize: {G} x {S} = {G * S} rows per icon, at most {MAX_ROWS}")
    g_out = G if max_num_groups is None else int(max_num_groups)
    s_out = S if max_seq_len is None else int(max_seq_len) + 2
    if g_out < 1 or s_out < 2:
        raise ValueError(f"canonicalize: max_num_groups >= 1 and max_seq_len >= 0; got {max_num_groups} and {max_seq_len}")
    if numericalize is not None and int(numericalize) < 1:
        raise ValueError(f"canonicalize: numericalize >= 1 or None; got {numericalize}")
    commands, args = commands.detach(), args.detach()
    if commands.dtype != args.dtype or commands.dtype not in (torch.float32, torch.int64):
        commands, args = commands.float(), args.float()
    return ops.canonicalize(commands.contiguous(), args.contiguous(), g_out, s_out, concat=layout == "concat",
                            numericalize=0 if numericalize is None else int(numericalize))


def _expand(name, commands, args, max_seq_len, **mode):
    """the argument checks and the launch `split`, `arcs_to_beziers` and `simplify` share"""
    if commands.dim() not in (2, 3) or args.dim() != commands.dim() + 1 or args.shape[:-1] != commands.shape \
            or args.shape[-1] != 11:
        raise ValueError(f"{name}: commands (N, G, S) with args (N, G, S, 11), or (N, S) with (N, S, 11); got "
                         f"{tuple(commands.shape)} and {tuple(args.shape)}")
    squeeze = commands.dim() == 2
    if squeeze:
        commands, args = commands.unsqueeze(1), args.unsqueeze(1)
    N, G, S = commands.shape
    if N < 1:
        raise ValueError(f"{name}: an empty batch")
    if max_seq_len is not None and int(max_seq_len) < 0:
        raise ValueError(f"{name}: max_seq_len >= 0; got {max_seq_len}")
    s_out = S if max_seq_len is None else int(max_seq_len) + 2
    if S < 2 or G * S > MAX_ROWS or G * s_out > MAX_ROWS:
        raise ValueError(f"{name}: {G} x {S} rows per icon in, {G} x {s_out} out; at least 2 per group and at most {MAX_ROWS} "
                         f"per icon")
    commands, args = commands.detach().float().contiguous(), args.detach().float().contiguous()
    res = (ops.paths_simplify if name == "simplify" else ops.paths_expand)(commands, args, s_out, **mode)
    if squeeze:
        res = {k: (v if k == "valid" else v.squeeze(1)) for k, v in res.items()}
    return res


def split(commands, args, n=None, max_dist=None, include_lines=True, max_seq_len=None):
    """``SVGPath.split`` for a batch: every `l` (unless include_lines=False) and `c` becomes k rows that draw the same curve,
    k = n, or max(ceil(length / max_dist), 1) with the length of an `l` its chord and of a `c` the polyline through its 100
    points at z = i / 99 (``SVGCommandBezier.length``).  Exactly one of n (int >= 1) and max_dist (finite, > 0) is given.
    commands (N, G, S) with args (N, G, S, 11), or (N, S) with (N, S, 11) read as G = 1 (the group axis is squeezed away again
    in the result); G * S <= 2048 and G * S_out <= 2048.  Inputs are detached and read as float32.  -> a dict, float32, no
    gradient:
      "commands" (N, G, S_out), "args" (N, G, S_out, 11), S_out = max_seq_len + 2 (default S): SOS, the rows, EOS to the end;
        every slot CMD_ARGS_MASK does not enable is -1.  Row 0 of a group is its frame and is never read as a command; a group
        ends at its first EOS.  An `l` gives ends at (1 - a) p0 + a p1, a = (i + 1) / k; a `c` the sub-curves on [i / k,
        (i + 1) / k].  Float64 throughout, rounded to float32 once; the last piece carries the row's end position bit for bit,
        and as the layout stores no start points consecutive pieces join exactly.  m, z and rows with k = 1 pass through.
      "len_groups" int32 (N, G): rows between SOS and the first EOS; "source_row" int32 (N, G, S_out): the input row (index
        in its group) an output row came from, -1 on SOS, EOS and padding; "lengths" float32 (N, G, S): the length of every
        live `l` / `c`, 0 elsewhere; "valid" bool (N,).
    An icon is invalid when a group needs more than S_out - 2 rows, when it holds a live `a` (the reference raises; see
    `arcs_to_beziers`), a command outside the vocabulary, or a live `l` / `c` whose start, arguments or length is not finite.
    It comes back as SOS, EOS... in every group with len_groups = 0, as `canonicalize` hands back an invalid icon.  n = 1, or
    max_dist above every length, is the identity on valid icons."""
    if (n is None) == (max_dist is None):
        raise ValueError(f"split: exactly one of n and max_dist; got n={n!r} and max_dist={max_dist!r}")
    if n is not None and (isinstance(n, bool) or not isinstance(n, int) or n < 1):
        raise ValueError(f"split: n is an int >= 1; got {n!r}")
    if max_dist is not None:
        if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float)) or not math.isfinite(max_dist) or max_dist <= 0:
            raise ValueError(f"split: max_dist is finite and > 0; got {max_dist!r}")
    return _expand("split", commands, args, max_seq_len, n=0 if n is None else n,
                   max_dist=0.0 if max_dist is None else float(max_dist), include_lines=bool(include_lines))


def arcs_to_beziers(commands, args, max_seq_len=None):
    """``SVGPath.simplify_arcs`` for a batch: every live `a` row (rx, ry, phi in degrees, fA, fS, end; flags read as != 0,
    radii as absolute values) is dropped when both radii are 0 or when its start and end are close (the test of
    `canonicalize`, step 2), and otherwise becomes max(floor(|sweep| / 45 deg), 1) `c` rows over equal parts of its sweep: the
    centre parametrisation and the control points of ``SVGCommandArc.to_beziers``, formula by formula, in float64.  Every other
    row passes through.  Shapes, framing, the returned dict (without "lengths") and the invalid cases are those of `split`,
    except that no icon is invalid for holding an arc.  Two deliberate deviations from the reference:
      1. radii too small for the chord (x'^2 / rx^2 + y'^2 / ry^2 = lambda > 1): both radii are scaled by sqrt(lambda), as the
         SVG implementation note F.6.6 asks; the chord is then a diameter and the sweep half a turn (4 rows).  The reference
         keeps the radii, its curve then misses the start point, and its sweep rests on the sign of a determinant that is
         zero up to rounding.
      2. exactly one radius 0: one `l` to the end position (note F.6.2).  The reference divides by zero and raises.
    A dropped arc leaves no row: the command behind it starts where the row before the arc ended, as everywhere in this
    layout (the reference's command objects keep their own start points, and it writes an `m` right before a dropped arc
    from the start point of the command that follows)."""
    return _expand("arcs_to_beziers", commands, args, max_seq_len, arcs=True)


def _positive(name, what, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
        raise ValueError(f"{name}: {what} is finite and > 0; got {v!r}")
    return float(v)


def simplify(commands, args, tolerance=0.1, epsilon=0.1, angle_threshold=179.0, force_smooth=False, unit=256 / 24,
             max_seq_len=None):
    """``SVGPath.simplify`` for a batch: in every sub-path (a maximal run of `l` / `c` rows; `m` and `z` pass through) the
    stretches of `c` rows that join at most 180 - angle_threshold degrees off straight are replaced by cubics fitted
    through their end points (Schneider's fit: at most 5 rounds of least squares and one Newton step per point, split at the
    worst point when the squared distance stays >= tolerance), the `l` rows between them by Ramer-Douglas-Peucker lines
    (a point further than epsilon from the chord is kept).  force_smooth=True fits one curve sequence through a whole
    sub-path, corners and lines included.  Only end points are read: run `split(max_dist=..., include_lines=False)` first,
    as `simplify_heuristic` does, to give the fit points along the curves.
    tolerance and epsilon are in the reference's units (its 24 box): coordinates are divided by `unit` in float64 when they
    are loaded, the fit runs in reference units, and computed control points are multiplied by `unit` once before the one
    rounding to float32 (the reference's max(error, error^2) and its comparison of a squared distance with tolerance are not
    scale-invariant).  Shapes, framing, dtype handling and detaching are those of `split`.  -> a dict, float32, no gradient:
      "commands" (N, G, S_out), "args" (N, G, S_out, 11), S_out = max_seq_len + 2 (default S): SOS, the rows, EOS to the end,
        -1 in every slot CMD_ARGS_MASK does not enable.  Between two segments, and before / behind a segment at the ends of a
        sub-path, the reference emits a zero-length `l` (its data sets hold them; `canonicalize` step 2 drops them), so a
        group can grow: at most rows in + segments + 1 rows.
      "len_groups" int32 (N, G); "source_row" int32 (N, G, S_out): for an `m` / `z` the input row itself, for a written `l` /
        `c` the input row whose end position the output row carries bit for bit (end positions are copies, never
        recomputed), -1 on SOS, EOS and padding; "valid" bool (N,).
    An icon is invalid, and comes back as `split` hands one back, for the reasons `split` has (a live `a`, a command outside
    the vocabulary, a live value that is not finite), when a group needs more than S_out - 2 rows, and when a fit needs the
    direction between two points at distance exactly 0 (the reference raises ZeroDivisionError in ``normalize``)."""
    tolerance, epsilon = _positive("simplify", "tolerance", tolerance), _positive("simplify", "epsilon", epsilon)
    unit = _positive("simplify", "unit", unit)
    if isinstance(angle_threshold, bool) or not isinstance(angle_threshold, (int, float)) or not math.isfinite(angle_threshold) \
            or not 0 <= angle_threshold <= 180:
        raise ValueError(f"simplify: angle_threshold is finite and within [0, 180]; got {angle_threshold!r}")
    return _expand("simplify", commands, args, max_seq_len, tolerance=tolerance, epsilon=epsilon,
                   cos_threshold=math.cos(math.radians(float(angle_threshold))), force_smooth=bool(force_smooth), unit=unit)


def simplify_heuristic(commands, args, unit=256 / 24, max_seq_len=None, work_seq_len=None):
    """``SVGPath.simplify_heuristic`` for a batch, three launches: `split(max_dist=2 * unit, include_lines=False)` into
    work_seq_len rows per group (default 2048 // G - 2), `simplify(0.1, 0.2, 150.0, unit=unit)` into the same size, and
    `split(max_dist=7.5 * unit)` into max_seq_len (default S - 2).  Input as for `split`.  -> a dict: "commands", "args",
    "len_groups" of the last step, and "valid" bool (N,), the AND of the three steps; an icon invalid at any step comes back
    as `split` hands back an invalid icon."""
    unit = _positive("simplify_heuristic", "unit", unit)
    if commands.dim() not in (2, 3):
        raise ValueError(f"simplify_heuristic: commands (N, G, S) or (N, S); got {tuple(commands.shape)}")
    G, S = (1 if commands.dim() == 2 else commands.shape[1]), commands.shape[-1]
    if G < 1 or G > MAX_ROWS // 2:
        raise ValueError(f"simplify_heuristic: {G} groups, at most {MAX_ROWS // 2}")
    work = MAX_ROWS // G - 2 if work_seq_len is None else work_seq_len
    out_len = S - 2 if max_seq_len is None else max_seq_len
    for what, v in (("work_seq_len", work), ("max_seq_len", out_len)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0 or G * (v + 2) > MAX_ROWS:
            raise ValueError(f"simplify_heuristic: {what} is an int >= 0 with {G} x ({what} + 2) <= {MAX_ROWS}; got {v!r}")
    try:
        first = split(commands, args, max_dist=2 * unit, include_lines=False, max_seq_len=work)
    except ValueError as e:
        raise ValueError(str(e).replace("split:", "simplify_heuristic:", 1)) from None
    fit = simplify(first["commands"], first["args"], 0.1, 0.2, 150.0, unit=unit, max_seq_len=work)
    last = split(fit["commands"], fit["args"], max_dist=7.5 * unit, max_seq_len=out_len)
    # an icon invalid at one step is handed on as empty groups, which the later steps pass through: nothing to blank here
    return {"commands": last["commands"], "args": last["args"], "len_groups": last["len_groups"],
            "valid": first["valid"] & fit["valid"] & last["valid"]}


def _finite(name, what, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"{name}: {what} is a finite number or a tensor; got {v!r}")
    return float(v)


def _number(name, what, v):
    return np.float32(_finite(name, what, v))


def _pair(name, what, v):
    """a Python pair (or one number for both coordinates) -> float32 [2]"""
    if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
        v = (v, v)
    if not isinstance(v, (tuple, list, np.ndarray)) or len(v) != 2:
        raise ValueError(f"{name}: {what} is a pair of numbers or an (N, 2) tensor; got {v!r}")
    return np.array([_number(name, what, v[0]), _number(name, what, v[1])], dtype=np.float32)


def _pack_steps(name, steps, N, device):
    """steps -> (kinds [K], params float32 [N, K, 3] on the device).  Python parameters are rounded to float32 on the host
    and reach the device in one copy; tensor parameters are placed with device ops: nothing is read back"""
    if not isinstance(steps, (list, tuple)) or not 1 <= len(steps) <= MAX_STEPS:
        raise ValueError(f"{name}: steps is a list of 1..{MAX_STEPS} (kind, parameter) pairs; got "
                         f"{len(steps) if isinstance(steps, (list, tuple)) else steps!r}")
    K = len(steps)
    host = np.zeros((K, 3), dtype=np.float32)
    late = []                                   # (step, column slice, tensor [N, width])
    kinds = []
    for k, step in enumerate(steps):
        if not isinstance(step, (list, tuple)) or len(step) != 2 or step[0] not in ops.STEP_KINDS:
            raise ValueError(f"{name}: step {k} is ('translate', v), ('scale', f) or ('rotate', degrees); got {step!r}")
        kind, v = step
        kinds.append(ops.STEP_KINDS[kind])
        if isinstance(v, torch.Tensor):
            v = v.detach()
            want = (N, 2) if kind == "translate" else (N,)
            if tuple(v.shape) != want:
                raise ValueError(f"{name}: the tensor parameter of step {k} ({kind}) has shape {tuple(v.shape)}, need {want}")
            if kind == "translate":
                late.append((k, slice(0, 2), v.to(device=device, dtype=torch.float32)))
            elif kind == "scale":
                late.append((k, slice(0, 1), v.to(device=device, dtype=torch.float32).unsqueeze(1)))
            else:                               # cosine and sine in float64, rounded to float32 (get_rotation_matrix)
                deg = v.to(device=device, dtype=torch.float64)
                rad = torch.deg2rad(deg)
                late.append((k, slice(0, 3), torch.stack([torch.cos(rad), torch.sin(rad), deg], dim=1).float()))
        elif kind == "translate":
            host[k, :2] = _pair(name, f"the vector of step {k}", v)
        elif kind == "scale":
            host[k, 0] = _number(name, f"the factor of step {k}", v)
        else:
            deg = _finite(name, f"the angle of step {k}", v)
            rad = np.deg2rad(deg)
            host[k] = (np.cos(rad), np.sin(rad), deg)
    params = torch.from_numpy(host).to(device).unsqueeze(0).expand(N, K, 3).contiguous()
    for k, cols, t in late:
        params[:, k, cols] = t
    return kinds, params


def transform(commands, args, steps, numericalize=None):
    """An affine step program on every icon of a batch, one launch of csrc/paths_transform.hip: `steps` is a list of 1..16
    ("translate", v), ("scale", f), ("rotate", degrees), with v a pair or an (N, 2) tensor, f and degrees a number or an
    (N,) tensor (one value per icon, left on the device: nothing is read back).  commands (N, G, S) with args (N, G, S, 11),
    or (N, S) with (N, S, 11); G * S <= 2048.  Inputs are detached and read as float32; no gradient.  -> {"commands": the
    commands as read, "args": the same shape as args, float32}.
    Every coordinate pair CMD_ARGS_MASK enables on a row before its group's first EOS goes through the steps in order, each
    add and each multiply rounded to float32 once as the reference's in-place numpy operations are (svglib/geom.py:136-151);
    a rotate is x' = fl(fl(c x) - fl(s y)), y' = fl(fl(s x) + fl(c y)) with c, s the float64 cosine and sine rounded to
    float32.  No step is elided or merged.  On an `a` row the end position takes every step, the radii scale steps only, a
    rotate adds its degrees to the x-axis rotation and the flags are copied - the reference cannot rotate an arc at all, so
    the arc rule under rotation is this package's own.  Every other slot and every other row (SOS, EOS, `z`, rows at or behind
    the first EOS) is copied; no row is dropped.  numericalize=n rounds afterwards: clip(round_half_even(v), 0, n - 1) on
    every enabled slot of a live row, step 7 of `canonicalize`."""
    if commands.dim() not in (2, 3) or args.dim() != commands.dim() + 1 or args.shape[:-1] != commands.shape \
            or args.shape[-1] != 11:
        raise ValueError(f"transform: commands (N, G, S) with args (N, G, S, 11), or (N, S) with (N, S, 11); got "
                         f"{tuple(commands.shape)} and {tuple(args.shape)}")
    squeeze = commands.dim() == 2
    if squeeze:
        commands, args = commands.unsqueeze(1), args.unsqueeze(1)
    N, G, S = commands.shape
    if N < 1:
        raise ValueError("transform: an empty batch")
    if G * S < 1 or G * S > MAX_ROWS:
        raise ValueError(f"transform: {G} x {S} = {G * S} rows per icon, at least 1 and at most {MAX_ROWS}")
    if numericalize is not None and (isinstance(numericalize, bool) or int(numericalize) < 1):
        raise ValueError(f"transform: numericalize >= 1 or None; got {numericalize}")
    kinds, params = _pack_steps("transform", steps, N, commands.device)
    commands, args = commands.detach().float().contiguous(), args.detach().float().contiguous()
    out = ops.paths_transform(commands, args, kinds, params, numericalize=0 if numericalize is None else int(numericalize))
    if squeeze:
        commands, out = commands.squeeze(1), out.squeeze(1)
    return {"commands": commands, "args": out}


def _neg(v):
    return -v


def _centre(name, viewbox):
    """the centre of a view box given by its size (a number, or a (width, height) pair): xy + wh / 2 with xy = 0"""
    return _pair(name, "viewbox", viewbox) * np.float32(0.5)


def _zoom_steps(name, factor, center, viewbox):
    c = _centre(name, viewbox)
    if center is None:
        center = c
    elif not isinstance(center, torch.Tensor):
        center = _pair(name, "center", center)
    return [("translate", _neg(c)), ("scale", factor), ("translate", center)]


def _normalize_steps(name, viewbox, target):
    vb = _pair(name, "viewbox", viewbox)
    t = _number(name, "target", target)
    if not vb.max() > 0 or not t > 0:
        raise ValueError(f"{name}: viewbox and target are > 0; got {viewbox!r} and {target!r}")
    return _zoom_steps(name, t / vb.max(), (t * np.float32(0.5),) * 2, viewbox)     # float32 / float32, as the reference


def zoom(commands, args, factor, center=None, viewbox=256):
    """``SVG.zoom(factor, center)`` (svg.py:281-289) in a view box of size `viewbox` (a number or a (width, height) pair):
    translate by minus the view-box centre, scale, translate to `center` (default the view-box centre)."""
    return transform(commands, args, _zoom_steps("zoom", factor, center, viewbox))


def rotate(commands, args, degrees, center=None, viewbox=256):
    """``SVG.rotate(Angle(degrees), center)`` (svg.py:271-279): translate by minus the view-box centre, rotate, translate
    to `center`.  For arcs see `transform`."""
    steps = _zoom_steps("rotate", 1.0, center, viewbox)
    steps[1] = ("rotate", degrees)
    return transform(commands, args, steps)


def translate(commands, args, vec):
    """``SVG.translate(Point(*vec))`` (svg.py:268-269)."""
    return transform(commands, args, [("translate", vec)])


def normalize(commands, args, viewbox, target=256):
    """``SVG.normalize(Bbox(target))`` (svg.py:291-300) of icons drawn in a view box of size `viewbox`: a zoom by the
    float32 quotient target / max(viewbox) from the centre of the view box to the centre of the target box."""
    return transform(commands, args, _normalize_steps("normalize", viewbox, target))


def augment(commands, args, factor, vec, viewbox=256, numericalize=None):
    """``SVGDataset._augment`` (svg_dataset.py:137-142) with given draws: a zoom by `factor` about the view-box centre and a
    translation by `vec`, each a number / pair or one value per icon ((N,) and (N, 2) tensors, e.g. of `augment_params`).
    numericalize=n appends ``SVG.numericalize(n)`` (svg.py:392-394: normalize to the n box, round, clip) to the same launch:
    with it this is ``SVGDataset.preprocess(svg, augment=True, numericalize=True)``."""
    steps = _zoom_steps("augment", factor, None, viewbox) + [("translate", vec)]
    if numericalize is not None:
        steps += _normalize_steps("augment", viewbox, numericalize)
    return transform(commands, args, steps, numericalize=numericalize)


def augment_params(n, mean=False, viewbox=256, generator=None, device=None):
    """The draws of ``SVGDataset._augment`` for n icons -> (factor float32 [n], vec float32 [n, 2]): factor = 0.2 u + 0.6 and
    vec = (5 u - 2.5) * viewbox / 24 with u uniform in [0, 1) (the reference draws in its 24 box); mean=True gives 0.7 and
    (0, 0) (svg_dataset.py:138-142).  Drawn by the torch generator on `device` (default: the generator's, else "cuda"): the
    reference's distribution, not the sequence of python's `random`."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"augment_params: n is an int >= 1; got {n!r}")
    vb = float(_number("augment_params", "viewbox", viewbox))
    if not vb > 0:
        raise ValueError(f"augment_params: viewbox is > 0; got {viewbox!r}")
    if device is None:
        device = generator.device if generator is not None else "cuda"
    if mean:
        return torch.full((n,), 0.7, dtype=torch.float32, device=device), torch.zeros(n, 2, dtype=torch.float32, device=device)
    u = torch.rand(n, 3, dtype=torch.float32, device=device, generator=generator)
    return 0.2 * u[:, 2] + 0.6, (5.0 * u[:, :2] - 2.5) * (vb / 24.0)


def numericalize(args, commands, n=256):
    """step 7 on its own, elementwise: the slots CMD_ARGS_MASK enables for the row's command become clip(round_half_even(v), 0,
    n - 1) (integer dtypes: clip only); every other slot is returned as it is.  Shapes (..., 11) and (...); same dtype out."""
    if args.shape[:-1] != commands.shape or args.shape[-1] != 11:
        raise ValueError(f"numericalize: args (..., 11) with commands (...); got {tuple(args.shape)} and {tuple(commands.shape)}")
    args = args.detach()
    cmd = commands.detach().long().clamp(0, CMD_ARGS_MASK.shape[0] - 1)
    mask = CMD_ARGS_MASK.to(args.device)[cmd].bool() & (cmd <= C_ID).unsqueeze(-1)
    rounded = args.clamp(0, n - 1) if not args.is_floating_point() else args.round().clamp(0, n - 1)
    return torch.where(mask, rounded, args)


def _fill_inputs(name, commands, args, samples, n):
    """the argument checks `overlap` and `compute_filling` share -> (commands [N, G, S], args [N, G, S, 11]) as the kernels
    read them: detached, float32 or int64, contiguous"""
    if commands.dim() not in (2, 3) or args.dim() != commands.dim() + 1 or args.shape[:-1] != commands.shape \
            or args.shape[-1] != 11:
        raise ValueError(f"{name}: commands (N, G, S) with args (N, G, S, 11), or (N, S) with (N, S, 11); got "
                         f"{tuple(commands.shape)} and {tuple(args.shape)}")
    if commands.dim() == 2:
        commands, args = commands.unsqueeze(1), args.unsqueeze(1)
    N, G, S = commands.shape
    if N < 1:
        raise ValueError(f"{name}: an empty batch")
    if G < 1 or G > MAX_FILL_GROUPS:
        raise ValueError(f"{name}: {G} groups per icon, at least 1 and at most {MAX_FILL_GROUPS}")
    if S < 1 or G * S > MAX_ROWS:
        raise ValueError(f"{name}: {G} x {S} = {G * S} rows per icon, at least 1 and at most {MAX_ROWS}")
    if isinstance(samples, bool) or not isinstance(samples, int) or not MIN_SAMPLES <= samples <= MAX_SAMPLES:
        raise ValueError(f"{name}: samples is an int within {MIN_SAMPLES}..{MAX_SAMPLES}; got {samples!r}")
    if isinstance(n, bool) or not isinstance(n, int) or not 2 <= n <= 64:
        raise ValueError(f"{name}: n is an int within 2..64; got {n!r}")
    commands, args = commands.detach(), args.detach()
    if commands.dtype != args.dtype or commands.dtype not in (torch.float32, torch.int64):
        commands, args = commands.float(), args.float()
    return commands.contiguous(), args.contiguous()


def _overlap_counts(commands, args, samples, n, evenodd):
    N, G, S = commands.shape
    modes = torch.ones(N, G, dtype=torch.int32, device=commands.device)      # FILL: every sub-path gets its closing chord
    segs, seg_counts, layer_first = ops.raster_segments_layers(commands.view(N * G, S), args.view(N * G, S, 11), modes, n=n,
                                                               groups=G)
    return ops.overlap_counts(segs, seg_counts, layer_first, samples=samples, evenodd=evenodd)


def overlap(commands, args, samples=128, n=10, evenodd=False):
    """How much of every group of an icon lies inside every other one, measured on samples x samples points: the pixel
    centres of `render.rasterize(size=samples)`.  commands (N, G, S) with args (N, G, S, 11), or (N, S) with (N, S, 11) read
    as G = 1; G <= 32, G * S <= 2048, 8 <= samples <= 1024, 2 <= n <= 64 points per command.  float32 and int64 are read as
    they are, anything else as float32.  Inputs are detached; there is no gradient.  Every sub-path is closed by a chord, as
    the rasteriser fills it; a point is inside a group when its winding number with respect to that group's chords alone is
    not 0 (odd with evenodd=True, as `render.draw` has it).  Two launches, nothing is read back.  -> a dict:
      "area" int32 (N, G): the points inside each group; "inter" int32 (N, G, G): the points inside both groups, symmetric,
      with "area" on its diagonal; "fraction" float32 (N, G, G): inter[i, j] / area[i], the share of group i that lies inside
      group j, 0 where area[i] is 0.
    This is the package's own overlap measure, in place of the reference's shapely polygons (``overlap_graph``,
    svglib/svg_primitive.py:422-441).  Arcs draw nothing, as everywhere in the rasteriser."""
    commands, args = _fill_inputs("overlap", commands, args, samples, n)
    area, inter = _overlap_counts(commands, args, samples, n, bool(evenodd))
    a = area.unsqueeze(-1)
    fraction = torch.where(a > 0, inter.float() / a.clamp(min=1).float(), torch.zeros((), device=area.device))
    return {"area": area, "inter": inter, "fraction": fraction}


def compute_filling(commands, args, rule="evenodd", threshold=0.9, samples=128, n=10, evenodd=False, closed=None):
    """``SVGPathGroup.compute_filling`` (svglib/svg_primitive.py:392-420) for a batch, every group of an icon taken as one of
    the reference's sub-paths: which groups are filled, which are holes, and in what order to paint them.  Input and limits as
    for `overlap`; `closed` is an optional bool (N, G), default all true: it stands in for the reference's ``SVGPath.closed``,
    which tensors do not carry.  Three launches (the rasteriser's segment pass, the overlap counts, the walk); nothing is
    read back.  No gradient.  The definition (include/dsvg.h; tests/paths_fill_ref.py restates it):
     1. group i participates when closed[i] and area[i] > 0 (`overlap`); every other group gets filling 0, depth -1, parent
        -1 and has no edges.
     2. there is an edge j -> i ("j covers i") when i != j, both participate and inter[i, j] > threshold * area[i]
        (``overlap_graph`` with this package's overlap measure; 0 < threshold <= 1).
     3. clockwise[i] is ``SVGPath.is_clockwise`` over the drawing commands of the group, by step 5 of `canonicalize`; closing
        chords are not part of it.
     4. the roots are the participating groups nothing covers, in ascending index; each starts a walk at current = [(d = 1,
        root)].  Per level, for (d, g) in current in ascending g: filling[g] = FILL (1) if d != 0 else ERASE (2), depth[g] =
        the level; every group g2 that g covers, that is still in the graph and has not been visited in this level, is
        visited in ascending order with parent g and d2 = 1 - d (rule="evenodd"), or d2 = d + 1 if clockwise[g2] ==
        clockwise[g] else d - 1 (rule="orientation", the reference's).  Then current leaves the graph, and the next current
        is the visited groups nothing covers any more.  A group that is never reached - two groups that cover each other,
        for instance - keeps filling 0.
     5. paint_order is the groups sorted stably by (filling 0 last, depth, index): an ERASE never precedes the FILL it cuts.
    The reference iterates Python sets, so the order inside a level (ascending here) is the only place where the walk can
    differ from it: when two groups of one level reach the same group with different d2.  rule="evenodd" is the default
    because canonical icons, the ones the model emits, are all clockwise: orientation carries no information there.
    -> a dict: "filling" int64 (N, G), as `render.draw(filling=...)` and ``PackedSVGStore.from_batch(filling=...)`` take it;
      "depth", "parent" int32 (N, G); "clockwise" bool (N, G); "paint_order" int64 (N, G): ``torch.gather`` with it reorders
      commands, args and filling for painting; "area", "inter" as `overlap` returns them.
    ``SVG.group_overlapping_paths`` (the regrouping into groups of several sub-paths) is not provided: "parent" and "depth"
    are what it needs."""
    if rule not in ops.FILLING_RULES:
        raise ValueError(f"compute_filling: rule 'evenodd' or 'orientation'; got {rule!r}")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0 < threshold <= 1:
        raise ValueError(f"compute_filling: threshold is a number within (0, 1]; got {threshold!r}")
    commands, args = _fill_inputs("compute_filling", commands, args, samples, n)
    N, G, _ = commands.shape
    if closed is None:
        closed = torch.ones(N, G, dtype=torch.bool, device=commands.device)
    else:
        if not isinstance(closed, torch.Tensor) or tuple(closed.shape) != (N, G) or closed.dtype != torch.bool:
            raise ValueError(f"compute_filling: closed is a bool tensor of shape {(N, G)}; got "
                             f"{tuple(closed.shape) if isinstance(closed, torch.Tensor) else closed!r}")
        closed = closed.detach().to(commands.device).contiguous()
    area, inter = _overlap_counts(commands, args, samples, n, bool(evenodd))
    res = ops.filling_from_counts(area, inter, commands, args, closed, threshold=float(threshold), rule=rule)
    res["area"], res["inter"] = area, inter
    return res
