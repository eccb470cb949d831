"""From SVG files to the model's tensors and back: the first link of the preprocessing chain (`paths` has the rest) and the way
out as text.  The reference reads an icon with ``SVG.load_svg`` (svglib/svg.py:72-139): Python objects, one icon at a time.
Here the text of every `d` attribute and every `points` list of a batch goes to the device in one copy and comes back as
padded rows from one call of csrc/svg_parse.hip.

`parse_paths` is the kernel: ``SVGPath.from_str(s).to_tensor()`` (svglib/svg_path.py:79-157, svg_command.py:51-120) and the
`points` lists of polylines and polygons (svg_primitive.py:196-207) for P strings at once.  include/dsvg.h has the
definition - the number pattern as an automaton, the decimal rule, the float32 position arithmetic of the reference's
``Point``, the rows ``SVGPath.from_commands`` keeps - and tests/svgio_ref.py restates it in plain Python;
tests/golden/svgio/parse.npz holds the reference's own results.

`load_svgs` is the document layer, on the host with the standard library only: ``xml.dom.expatbuilder`` as the reference
uses it, groups in the reference's order (all `path`, then `rect`, `circle`, `ellipse`, `line`, `polyline`, `polygon`, each in
document order, nested elements included, `transform` ignored), `fill`, `filling` and the view box.  The rows of `rect`, `circle`,
`ellipse` and `line` (``to_path``, svg_primitive.py:87-96, 145-153, 178-179) have at most six numbers each and are formed on
the host in float32, as the reference's ``Point`` forms them, and placed with one indexed copy.

`preprocess` is the reference's dataset/preprocess.py for a batch: ``arcs_to_beziers -> normalize(viewbox, 24) -> zoom(0.9) ->
canonicalize -> simplify_heuristic(unit=1)``, composed from `paths`; `preprocess_files` runs it over files and returns a
``PackedSVGStore`` (``from_batch(viewbox=24)``) with the meta table of preprocess.py:26-32.  `to_svg` writes tensors as SVG
text that `load_svgs` reads back bit for bit.

Numbers: `parse_paths`, `load_svgs` and `preprocess_files` take ``numbers="fast"`` (the default: digits below 2^53 and a decimal
exponent within 22, SLOW_NUMBER otherwise) or ``numbers="exact"`` (dsvg_svg_parse_exact: every number of up to 19 significant
digits whose float32 value is finite and not zero, converted on the device with integers as ``float()`` converts it).  Files
the reference itself saved - ``SVG.save_svg`` prints float32 values through float64 with up to 17 digits, so its docs/ and the
output folder of dataset/preprocess.py - load with ``numbers="exact"``; tests/svgio_exact_ref.py restates that rule and
tests/golden/svgio/exact.npz holds the reference's rows for long numbers.

Out of scope: `transform=` attributes, styles, `<use>`, units and percentages, compact arc flags (`a1 1 0 01 2 2`: the
reference reads `01` as one number and asserts, this reports ARG_COUNT), ``SVG.load_splineset``, and numbers of more than 19
significant digits (status SLOW_NUMBER under either rule).
"""
import os
from xml.dom import expatbuilder
from xml.parsers.expat import ExpatError

import numpy as np
import torch

from . import lib as _l
from . import ops, paths
from .lib import DsvgError
from .svgtensor import CMD_ARGS_MASK

__all__ = ["parse_paths", "load_svgs", "preprocess", "preprocess_files", "to_svg", "meta_table", "STATUS", "TILE"]

KIND_PATH, KIND_POLYLINE, KIND_POLYGON = _l.DSVG_SVG_PATH, _l.DSVG_SVG_POLYLINE, _l.DSVG_SVG_POLYGON
OK, EMPTY, ARG_COUNT, SLOW_NUMBER, ROWS_OVERFLOW, BAD_SLOT, RANGE = range(7)
STATUS = ("OK", "EMPTY", "ARG_COUNT", "SLOW_NUMBER", "ROWS_OVERFLOW", "BAD_SLOT", "RANGE")
TILE = _l.DSVG_SVG_TILE                 # bytes of a string one wave of the kernel reads at a time
M, L, C, A, EOS, SOS, Z = range(7)
# the reference's order of groups (svglib/svg.py:127-137)
TAGS = ("path", "rect", "circle", "ellipse", "line", "polyline", "polygon")
_TEXT_KIND = {"path": ("d", KIND_PATH), "polyline": ("points", KIND_POLYLINE), "polygon": ("points", KIND_POLYGON)}


def _shape(name, N, G, S):
    for what, v in (("N", N), ("G", G), ("S", S)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}: {what} is an int; got {v!r}")
    if N < 1 or G < 1 or S < 2 or G * S > paths.MAX_ROWS:
        raise ValueError(f"{name}: N >= 1, G >= 1, S >= 2 and G * S <= {paths.MAX_ROWS} rows per icon; got N={N}, G={G}, S={S}")
    return int(N), int(G), int(S)


def pack_strings(strings):
    """a list of str / bytes -> (data uint8 [B], offsets int64 [P + 1]) as numpy arrays: the UTF-8 bytes back to back"""
    raw = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strings]
    offsets = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum(np.fromiter((len(r) for r in raw), dtype=np.int64, count=len(raw)), out=offsets[1:])
    return np.frombuffer(b"".join(raw), dtype=np.uint8).copy(), offsets


def _entry(name, numbers):
    """numbers = "fast" | "exact" -> the entry of `ops` that reads numbers that way"""
    if numbers == "fast":
        return ops.svg_parse
    if numbers == "exact":
        return ops.svg_parse_exact
    raise ValueError(f'{name}: numbers is "fast" or "exact"; got {numbers!r}')


def parse_paths(data, offsets=None, kind=None, slot=None, N=None, G=None, S=None, icon=None, device=None, numbers="fast"):
    """SVG path text -> padded rows, one call of csrc/svg_parse.hip.  Two forms:
      tensors on the device (nothing is read back): data uint8 [B], the UTF-8 bytes of P strings back to back; offsets int64
        [P + 1]; kind uint8 [P] (0 a `d` attribute, 1 the `points` of a polyline, 2 of a polygon); slot int32 [P], the output
        group n * G + g each string fills, -1 = parse for the status only; the ints N, G, S with S >= 2, G * S <= 2048.
      a list of str / bytes as `data`, with `icon` (a list of ints, default all 0) in place of slot: the strings of icon n fill
        its groups in list order; kind defaults to 0, N to max(icon) + 1, device to "cuda".
    -> a dict, framed as `paths.split` frames its result:
      "commands" float32 (N, G, S), "args" float32 (N, G, S, 11): SOS, the rows, EOS to the end; -1 in every slot
        CMD_ARGS_MASK does not enable, a `z` row all -1; a group no string fills is SOS, EOS...
      "len_groups" int32 (N, G); "status" int32 [P], an index into `STATUS`; "valid" bool [N].
    An icon is valid when every string with a slot in it is OK or EMPTY; an invalid icon comes back as SOS, EOS... in every
    group, as `paths.split` hands one back.  A string whose slot is outside [-1, N G), or shared with another string, is
    BAD_SLOT and is not parsed.
    numbers: "fast" (the default) converts a number whose digits are an integer below 2^53 with a decimal exponent of at most
    22 either way, and reports SLOW_NUMBER for any other; "exact" converts every number of up to 19 significant digits whose
    float32 value is finite and not zero, as Python's float() does - among them the 17-digit numbers ``SVG.save_svg`` prints.
    Where both give a value it is the same one."""
    entry = _entry("parse_paths", numbers)
    if isinstance(data, (list, tuple)):
        if offsets is not None or slot is not None:
            raise ValueError("parse_paths: a list of strings comes with `icon`, not with offsets or slot")
        P = len(data)
        if P < 1:
            raise ValueError("parse_paths: no strings")
        if G is None or S is None:
            raise ValueError("parse_paths: G and S are required")
        icon = [0] * P if icon is None else [int(i) for i in icon]
        if len(icon) != P or min(icon) < 0:
            raise ValueError(f"parse_paths: icon is a list of {P} ints >= 0")
        N = max(icon) + 1 if N is None else N
        N, G, S = _shape("parse_paths", N, G, S)
        seen, slots = {}, np.zeros(P, dtype=np.int32)
        for p, n in enumerate(icon):
            g = seen.get(n, 0)
            seen[n] = g + 1
            slots[p] = n * G + g if g < G and n < N else N * G       # past the last group: out of range, BAD_SLOT
        kinds = np.zeros(P, dtype=np.uint8) if kind is None else np.asarray(kind, dtype=np.uint8).reshape(P)
        host_data, host_off = pack_strings(data)
        device = "cuda" if device is None else device
        ops.require_device(device)
        data, offsets = torch.from_numpy(host_data).to(device), torch.from_numpy(host_off).to(device)
        kind, slot = torch.from_numpy(kinds).to(device), torch.from_numpy(slots).to(device)
    else:
        if not all(isinstance(t, torch.Tensor) for t in (data, offsets, kind, slot)):
            raise ValueError("parse_paths: data, offsets, kind and slot are tensors, or data is a list of strings")
        if N is None or G is None or S is None:
            raise ValueError("parse_paths: N, G and S are required")
        N, G, S = _shape("parse_paths", N, G, S)
        P = offsets.numel() - 1
        if data.dim() != 1 or offsets.dim() != 1 or P < 1 or tuple(kind.shape) != (P,) or tuple(slot.shape) != (P,):
            raise ValueError(f"parse_paths: data [B], offsets [P + 1] with P >= 1, kind [P] and slot [P]; got "
                             f"{tuple(data.shape)}, {tuple(offsets.shape)}, {tuple(kind.shape)} and {tuple(slot.shape)}")
        if data.dtype != torch.uint8 or offsets.dtype != torch.int64 or kind.dtype != torch.uint8 or slot.dtype != torch.int32:
            raise ValueError(f"parse_paths: data uint8, offsets int64, kind uint8, slot int32; got {data.dtype}, "
                             f"{offsets.dtype}, {kind.dtype} and {slot.dtype}")
        if data.numel() >= 2 ** 31:
            raise ValueError("parse_paths: 2^31 bytes of text or more in one call")
        data, offsets, kind, slot = (t.detach().contiguous() for t in (data, offsets, kind, slot))
    return entry(data, offsets, kind, slot, N, G, S)


# ---- the document layer ------------------------------------------------------------------------------------------------------
F = np.float32


def _row(cmd, arc=None, end=None):
    a = np.full(11, -1.0, dtype=F)
    if arc is not None:
        a[0:5] = arc
    if end is not None:
        a[9:11] = end
    return cmd, a


def _primitive_rows(tag, x):
    """``to_path`` of a rect, circle, ellipse or line (svg_primitive.py:87-96, 145-153, 178-179) -> [(command, args [11])].
    Attributes are read with float() and become float32 at once; every sum is one float32 add, as ``Point`` adds"""
    num = lambda name: F(float(x.getAttribute(name)))            # noqa: E731
    opt = lambda name: F(float(x.getAttribute(name) or 0.0))     # noqa: E731
    if tag == "rect":
        px = num("x") if x.hasAttribute("x") else F(0)
        py = num("y") if x.hasAttribute("y") else F(0)
        w, h = num("width"), num("height")
        p0, p1, p2, p3 = (px, py), (px + w, py + F(0)), (px + w, py + h), (px + F(0), py + h)
        return [_row(M, end=p0), _row(L, end=p1), _row(L, end=p2), _row(L, end=p3), _row(L, end=p0), _row(Z)]
    if tag == "line":
        return [_row(M, end=(opt("x1"), opt("y1"))), _row(L, end=(opt("x2"), opt("y2")))]
    cx, cy = num("cx"), num("cy")
    if tag == "circle":
        rx = ry = num("r")
    else:
        rx, ry = num("rx"), num("ry")
    # centre +- the projections of the radius: c - r is c + (-1 * r)
    p0, p1, p2, p3 = (cx + rx, cy + F(0)), (cx + F(0), cy + ry), (cx + -rx, cy + -F(0)), (cx + -F(0), cy + -ry)
    arc = (rx, ry, F(0), F(0), F(1))
    return [_row(M, end=p0)] + [_row(A, arc=arc, end=p) for p in (p1, p2, p3, p0)] + [_row(Z)]


def _viewbox(root):
    text = root.getAttribute("viewBox").replace(",", " ").split()
    if len(text) != 4:
        raise ValueError("viewBox")
    vb = np.array([float(t) for t in text], dtype=F)
    if not np.isfinite(vb).all():
        raise ValueError("viewBox")
    return vb


def _document(text):
    """one SVG document -> (view box float32 [4], [(tag, element, index in document order)] in the reference's group order)"""
    dom = expatbuilder.parseString(text, False)
    root = dom.getElementsByTagName("svg")[0]
    vb = _viewbox(root)
    order = {}
    for i, node in enumerate(n for n in dom.getElementsByTagName("*") if n.tagName in TAGS):
        order[id(node)] = i
    return vb, [(tag, x, order[id(x)]) for tag in TAGS for x in dom.getElementsByTagName(tag)]


def load_svgs(texts, max_num_groups=8, max_seq_len=30, device="cuda", numbers="fast"):
    """A list of SVG documents (str) -> the model's padded tensors: ``SVG.from_str(text)`` with every group through
    ``to_path()`` for the whole list.  Groups are taken in the reference's order: all `path`, then `rect`, `circle`,
    `ellipse`, `line`, `polyline`, `polygon`, each in document order, nested elements included, `transform` ignored.  G =
    max_num_groups, S = max_seq_len + 2.  The text of paths, polylines and polygons goes through `parse_paths`; the rows of
    the other primitives are formed on the host and placed with one indexed copy.  -> the dict of `parse_paths` ("status" in
    the order the strings were met) plus
      "fill" bool (N, G): no `fill` attribute, or one that is not "none"; "filling" int32 (N, G): the int attribute, or 0;
      "viewbox" float32 (N, 4): x, y, width, height (separated by spaces or commas); "source" int32 (N, G): the index of the
      group's element among the icon's drawable elements in document order, -1 where the group is unused.
    An icon is invalid - SOS, EOS... in every group, "valid" false - when a string of it is, when it has more groups than
    max_num_groups, when a primitive needs more than max_seq_len rows, holds a value that is not finite or lacks a number it
    needs, when its view box is not four finite numbers, or when the document does not parse.  numbers: how `parse_paths` reads
    the numbers of the text, "fast" or "exact" (a file ``SVG.save_svg`` wrote needs "exact"); the attributes of the other
    primitives are read by float() on the host either way."""
    _entry("load_svgs", numbers)
    if isinstance(texts, (str, bytes)) or len(texts) < 1:
        raise ValueError("load_svgs: texts is a non-empty list of SVG documents")
    N, G, S = _shape("load_svgs", len(texts), max_num_groups, max_seq_len + 2 if isinstance(max_seq_len, int) else max_seq_len)
    ops.require_device(device)
    strings, kinds, slots = [], [], []
    rows_cmd, rows_arg, rows_at, lens_at, lens = [], [], [], [], []
    fill = np.zeros((N, G), dtype=bool)
    filling = np.zeros((N, G), dtype=np.int32)
    viewbox = np.zeros((N, 4), dtype=F)
    source = np.full((N, G), -1, dtype=np.int32)
    host_valid = np.ones(N, dtype=bool)
    for n, text in enumerate(texts):
        mark = (len(strings), len(rows_cmd), len(lens))
        try:
            vb, elements = _document(text)
            if len(elements) > G:
                raise ValueError("groups")
            for g, (tag, x, index) in enumerate(elements):
                if tag in _TEXT_KIND:
                    attr, kind = _TEXT_KIND[tag]
                    strings.append(x.getAttribute(attr))
                    kinds.append(kind)
                    slots.append(n * G + g)
                else:
                    rows = _primitive_rows(tag, x)
                    if len(rows) > S - 2 or not all(np.isfinite(a[a != -1.0]).all() for _, a in rows):
                        raise ValueError("primitive")
                    for r, (c, a) in enumerate(rows):
                        rows_cmd.append(c)
                        rows_arg.append(a)
                        rows_at.append((n * G + g) * S + 1 + r)
                    lens_at.append(n * G + g)
                    lens.append(len(rows))
                fill[n, g] = not x.hasAttribute("fill") or x.getAttribute("fill") != "none"
                filling[n, g] = int(x.getAttribute("filling")) if x.hasAttribute("filling") else 0
                source[n, g] = index
            viewbox[n] = vb
        except (ValueError, IndexError, ExpatError):     # what a document can lack: the icon is dropped, the batch goes on
            host_valid[n] = False
            del strings[mark[0]:], kinds[mark[0]:], slots[mark[0]:]
            del rows_cmd[mark[1]:], rows_arg[mark[1]:], rows_at[mark[1]:]
            del lens_at[mark[2]:], lens[mark[2]:]
            fill[n], filling[n], source[n], viewbox[n] = False, 0, -1, 0
    if not strings:                         # the kernel also writes the frames: give it one string that fills nothing
        strings, kinds, slots = [""], [KIND_PATH], [-1]
    host_data, host_off = pack_strings(strings)
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    res = parse_paths(up(host_data), up(host_off), up(np.asarray(kinds, dtype=np.uint8)), up(np.asarray(slots, dtype=np.int32)),
                      N, G, S, numbers=numbers)
    valid = res["valid"] & up(host_valid)
    if rows_cmd:
        at = up(np.asarray(rows_at, dtype=np.int64))
        res["commands"].view(-1).index_copy_(0, at, up(np.asarray(rows_cmd, dtype=F)))
        res["args"].view(-1, 11).index_copy_(0, at, up(np.stack(rows_arg)))
        res["len_groups"].view(-1).index_copy_(0, up(np.asarray(lens_at, dtype=np.int64)), up(np.asarray(lens, dtype=np.int32)))
    # an icon one of whose strings failed: the rows placed above go too
    keep = valid.view(N, 1, 1)
    frame = torch.full((S,), float(EOS), device=dev)
    frame[0] = float(SOS)
    res["commands"] = torch.where(keep, res["commands"], frame.view(1, 1, S))
    res["args"] = torch.where(keep.unsqueeze(-1), res["args"], torch.full((), -1.0, device=dev))
    res["len_groups"] = torch.where(valid.view(N, 1), res["len_groups"], torch.zeros((), dtype=torch.int32, device=dev))
    res["valid"] = valid
    res["fill"], res["filling"], res["viewbox"], res["source"] = up(fill), up(filling), up(viewbox), up(source)
    return res


# ---- dataset/preprocess.py for a batch -------------------------------------------------------------------------------------------
def preprocess(batch, max_num_groups=None, max_seq_len=None, work_seq_len=None):
    """The reference's dataset/preprocess.py (``svg.normalize(); svg.zoom(0.9); svg.canonicalize(); svg.simplify_heuristic()``)
    on a batch of `load_svgs`, or any dict with "commands" (N, G, S), "args" (N, G, S, 11), "viewbox" (N, 4) and optionally
    "valid" (N,) and "filling" (N, G): the chain of the `paths` docstring,
      ``arcs_to_beziers -> normalize(viewbox, 24) -> zoom(0.9, viewbox=24) -> canonicalize -> simplify_heuristic(unit=1)``,
    every link an existing function of `paths`; nothing is read back.  The view boxes are per icon and stay on the device:
    centre = xy + wh / 2 and factor = 24 / max(wh), both formed in float32 as ``SVG.normalize`` forms them, are the (N, 2) and
    (N,) tensor parameters of one `paths.transform` with the six steps of the two zooms.  Work happens in rows of
    work_seq_len per group (default 2048 // G - 2); the result has max_num_groups groups (default G) of max_seq_len rows
    (default S - 2).  -> {"commands", "args", "len_groups", "valid": the AND over every link and the batch's own, "filling"
    int64 (N, max_num_groups): the batch's filling carried along by ``source_group`` (0 where unused), "n_groups" int32 (N,)};
    coordinates are in the 24 box."""
    cmd, arg, vb = batch["commands"], batch["args"], batch["viewbox"]
    if cmd.dim() != 3 or tuple(arg.shape) != tuple(cmd.shape) + (11,) or tuple(vb.shape) != (cmd.shape[0], 4):
        raise ValueError(f"preprocess: commands (N, G, S), args (N, G, S, 11) and viewbox (N, 4); got {tuple(cmd.shape)}, "
                         f"{tuple(arg.shape)} and {tuple(vb.shape)}")
    N, G, S = cmd.shape
    g_out = G if max_num_groups is None else int(max_num_groups)
    s_out = S - 2 if max_seq_len is None else int(max_seq_len)
    if g_out < 1 or s_out < 0 or g_out * (s_out + 2) > paths.MAX_ROWS:
        raise ValueError(f"preprocess: max_num_groups >= 1, max_seq_len >= 0 and max_num_groups x (max_seq_len + 2) <= "
                         f"{paths.MAX_ROWS}; got {max_num_groups} and {max_seq_len}")
    work = paths.MAX_ROWS // max(G, g_out) - 2 if work_seq_len is None else int(work_seq_len)
    if work < 0 or max(G, g_out) * (work + 2) > paths.MAX_ROWS:
        raise ValueError(f"preprocess: work_seq_len >= 0 with {max(G, g_out)} x (work_seq_len + 2) <= {paths.MAX_ROWS}; got "
                         f"{work_seq_len}")
    vb = vb.detach().to(device=cmd.device, dtype=torch.float32)
    centre = vb[:, :2] + vb[:, 2:] * 0.5
    # the float32 quotient, correctly rounded: a float64 division rounded once more is that (53 >= 2 * 24 + 2 bits), whatever
    # the device's float32 division rounds to
    factor = (24.0 / vb[:, 2:].max(dim=1).values.double()).float()
    flat = paths.arcs_to_beziers(cmd, arg, max_seq_len=work)
    steps = [("translate", -centre), ("scale", factor), ("translate", (12.0, 12.0))] + paths._zoom_steps("preprocess", 0.9, None, 24)
    moved = paths.transform(flat["commands"], flat["args"], steps)
    canon = paths.canonicalize(moved["commands"], moved["args"], max_num_groups=g_out, max_seq_len=work)
    simple = paths.simplify_heuristic(canon["commands"], canon["args"], unit=1.0, max_seq_len=s_out, work_seq_len=work)
    valid = flat["valid"] & canon["valid"] & simple["valid"]
    if batch.get("valid") is not None:
        valid = valid & batch["valid"].to(cmd.device)
    src = canon["source_group"].long()
    filling = torch.zeros(N, g_out, dtype=torch.int64, device=cmd.device)
    if batch.get("filling") is not None:
        filling = torch.gather(batch["filling"].to(cmd.device).long(), 1, src.clamp(min=0))
        filling = torch.where(src >= 0, filling, torch.zeros_like(filling))
    lens = torch.where(valid.view(N, 1), simple["len_groups"], torch.zeros_like(simple["len_groups"]))
    return {"commands": simple["commands"], "args": simple["args"], "len_groups": lens, "valid": valid, "filling": filling,
            "n_groups": (lens > 0).sum(dim=1).to(torch.int32)}


def meta_table(ids, len_groups):
    """The meta table of dataset/preprocess.py:26-32 from the rows per group of every icon: one record per icon with id,
    total_len, nb_groups, len_groups (the groups in use), max_len_group.  -> a pandas DataFrame, which
    ``SVGTensorDataset.filter_meta`` takes (a list of dicts where pandas is missing)"""
    lens = np.asarray(len_groups.detach().cpu() if isinstance(len_groups, torch.Tensor) else len_groups, dtype=np.int64)
    if lens.ndim != 2 or len(ids) != lens.shape[0]:
        raise ValueError(f"meta_table: len_groups (N, G) with one id per icon; got {lens.shape} and {len(ids)} ids")
    records = []
    for i, row in zip(ids, lens):
        used = [int(v) for v in row if v > 0]
        records.append({"id": i, "total_len": sum(used), "nb_groups": len(used), "len_groups": used,
                        "max_len_group": max(used) if used else 0})
    try:
        import pandas as pd
    except ImportError:
        return records
    return pd.DataFrame(records, columns=["id", "total_len", "nb_groups", "len_groups", "max_len_group"])


def preprocess_files(files, max_num_groups=8, max_seq_len=30, device="cuda", batch_size=4096, numbers="fast"):
    """dataset/preprocess.py over SVG files: `load_svgs` and `preprocess` in batches of batch_size, the icons that stay valid
    (and are not empty) packed by ``PackedSVGStore.from_batch(viewbox=24)``.  -> (store, meta): the store's ids are the file
    names without their extension, meta is `meta_table` over the same icons, in the same order.  numbers goes to `load_svgs`:
    "exact" for files the reference saved (the output folder of its dataset/preprocess.py among them)."""
    from .dataset import PackedSVGStore
    _entry("preprocess_files", numbers)
    files = list(files)
    if not files:
        raise ValueError("preprocess_files: no files")
    parts, ids = [], []
    for lo in range(0, len(files), int(batch_size)):
        chunk = files[lo:lo + int(batch_size)]
        texts = []
        for f in chunk:
            with open(f, "r", encoding="utf-8", errors="replace") as fh:      # a stray byte is a separator
                texts.append(fh.read())
        res = preprocess(load_svgs(texts, max_num_groups, max_seq_len, device, numbers=numbers))
        keep = (res["valid"] & (res["n_groups"] > 0)).nonzero().view(-1)
        ids += [os.path.splitext(os.path.basename(chunk[i]))[0] for i in keep.tolist()]
        parts.append({k: res[k].index_select(0, keep) for k in ("commands", "args", "len_groups", "filling")})
    cat = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    if cat["commands"].shape[0] == 0:
        raise DsvgError("preprocess_files: no icon survived preprocessing")
    store = PackedSVGStore.from_batch(cat["commands"], cat["args"], cat["len_groups"], filling=cat["filling"], viewbox=24.0)
    store.ids = ids
    return store, meta_table(ids, cat["len_groups"])


# ---- the way out -------------------------------------------------------------------------------------------------------------------
def _number(v):
    """the shortest decimal that reads back to the float32 v through the parser's fast path"""
    if not np.isfinite(v):
        raise ValueError(f"to_svg: {v!r} is not finite")
    text = np.format_float_positional(v, unique=True, trim="-")
    digits = text.lstrip("-")
    whole, _, frac = digits.partition(".")
    if int(whole + frac) >= 2 ** 53 or len(frac) > 22 or F(float(text)).tobytes() != F(v).tobytes():
        raise ValueError(f"to_svg: {v!r} has no decimal form the parser's fast path reads ({text})")
    return text


_LETTER = {M: "M", L: "L", C: "C", A: "A", Z: "Z"}


def to_svg(commands, args, filling=None, viewbox=256):
    """Tensors -> SVG text, on the host: commands (N, G, S) with args (N, G, S, 11) (or (G, S) and (G, S, 11) for one icon),
    filling (N, G) optional -> a list of N documents.  Every group up to the last one with rows becomes a
    ``<path fill="none" filling="k" d="...">`` (a group without rows an empty `d`, so that groups keep their index); a group
    ends at its first EOS and its frame row is skipped.  Letters are upper case (M L C Z A) and every number is the shortest
    decimal that reads back to the same float32, so `load_svgs` returns the rows bit for bit.  Raises ValueError for a value
    the parser's fast path would not read (not finite, or more than 2^53 as a digit string) and for a command outside m, l, c,
    a, z in front of a group's first EOS."""
    cmd = np.asarray(commands.detach().cpu() if isinstance(commands, torch.Tensor) else commands)
    arg = np.asarray(args.detach().cpu() if isinstance(args, torch.Tensor) else args).astype(F)
    if cmd.ndim == 2:
        cmd, arg = cmd[None], arg[None]
        filling = None if filling is None else np.asarray(filling.cpu() if isinstance(filling, torch.Tensor) else filling)[None]
    if cmd.ndim != 3 or arg.shape != cmd.shape + (11,):
        raise ValueError(f"to_svg: commands (N, G, S) with args (N, G, S, 11); got {cmd.shape} and {arg.shape}")
    N, G, S = cmd.shape
    fil = np.zeros((N, G), dtype=np.int64) if filling is None else \
        np.asarray(filling.detach().cpu() if isinstance(filling, torch.Tensor) else filling).reshape(N, G)
    mask = CMD_ARGS_MASK.numpy().astype(bool)
    vb = _number(F(viewbox))
    docs = []
    for n in range(N):
        groups = []
        for g in range(G):
            parts = []
            for r in range(1, S):
                c = int(cmd[n, g, r])
                if c == EOS:
                    break
                if c not in _LETTER:
                    raise ValueError(f"to_svg: command {c} in icon {n}, group {g}, row {r}")
                parts.append(_LETTER[c] + " ".join(_number(v) for v in arg[n, g, r][mask[c]]))
            groups.append(" ".join(parts))
        while groups and not groups[-1]:
            groups.pop()
        body = "".join(f'<path fill="none" filling="{int(fil[n, g])}" d="{d}"/>' for g, d in enumerate(groups))
        docs.append(f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 {vb} {vb}">{body}</svg>')
    return docs
