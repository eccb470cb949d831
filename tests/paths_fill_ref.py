"""Float64 restatement of the filling of a decoded batch (include/dsvg.h, "Filling of a decoded batch"), written from the
definition.  It is the oracle of tests/test_paths_fill_gpu.py and tests/test_paths_fill_host.py, and
tests/golden/make_golden_filling.py checks its walk against the reference's own ``SVGPathGroup.compute_filling``.

Overlap counts work from chord RECORDS (ax, ay, bx - ax, by - ay, flags; tests/raster_ref.records), so the vertices are the
producer's own numbers.  The samples are the K x K pixel centres ((col + 0.5) s, (row + 0.5) s), s = 256 / K, in the float32
expressions of the sweep.  A sample is inside group i when its winding number with respect to the chords of group i alone is
not 0 (odd: even-odd), counted on a ray towards +x with the half-open rule: a chord with ay <= cy < by counts +1, one with by
<= cy < ay counts -1, each when e = dx py - dy px (p = the sample minus a) is > 0 resp. < 0; by is the a.y of the record that
follows (of the sub-path's first record on a closing chord), so that a shared vertex is one number.
A sample is BORDERLINE for a group when some chord of the group whose half-open y-range holds the sample has 0 < |e| <= 2**-20
(|dx py| + |dy px|): the float32 sign test of the device (two rounded differences, one rounded product, one fused multiply-
add: a relative error of a few 2**-24 of that sum) may then differ from the float64 one.

Filling from counts: participation, edges, and the level-by-level walk of svglib/svg_primitive.py:396-418 with the order
inside a level fixed (ascending; "descending" is there to find the cases in which the order matters)."""
import numpy as np

OUTLINE, FILL, ERASE = 0, 1, 2
VIEW = 256.0
BORDER_REL = 2.0 ** -20


def centres(samples):
    """the float32 sample coordinates of the sweep, as float64"""
    s = np.float32(VIEW) / np.float32(samples)
    return ((np.arange(samples, dtype=np.float32) + np.float32(0.5)) * s).astype(np.float64)


def end_y(rec, flags):
    """records float64 [C, 4], flags int [C] -> the y of every chord's end vertex as the next record holds it"""
    C = rec.shape[0]
    by = rec[:, 1] + rec[:, 3]
    back = flags.astype(np.int64) >> 1
    j = np.arange(C)
    closing = (back > 0) & (back <= j)
    by[closing] = rec[(j - back)[closing], 1]
    nxt = (back == 0) & (j + 1 < C)
    by[nxt] = rec[(j + 1)[nxt], 1]
    return by


def group_membership(rec, by, samples, evenodd):
    """the chords of ONE group -> (inside bool [K, K], borderline bool [K, K], on_line bool [K, K]), [row, col]; on_line: some
    chord whose half-open y-range holds the sample has e == 0 exactly (reported, not part of any bound)"""
    K = samples
    c = centres(K)
    wind = np.zeros((K, K), dtype=np.int64)
    border = np.zeros((K, K), dtype=bool)
    on_line = np.zeros((K, K), dtype=bool)
    if rec.shape[0] == 0:
        return wind != 0, border, on_line
    ax, ay, dx, dy = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    for row in range(K):
        cy = c[row]
        down, up = (ay <= cy) & (cy < by), (by <= cy) & (cy < ay)
        sel = down | up
        if not sel.any():
            continue
        px = c[None, :] - ax[sel, None]
        py = (cy - ay[sel])[:, None]
        t1, t2 = dx[sel, None] * py, dy[sel, None] * px
        e = t1 - t2
        wind[row] += ((e > 0) & down[sel, None]).sum(0) - ((e < 0) & up[sel, None]).sum(0)
        border[row] |= ((np.abs(e) <= BORDER_REL * (np.abs(t1) + np.abs(t2))) & (e != 0)).any(0)
        on_line[row] |= (e == 0).any(0)
    inside = (wind % 2 != 0) if evenodd else (wind != 0)
    return inside, border, on_line


def overlap_counts(segs, seg_counts, layer_first, samples, evenodd=False, with_on_line=False):
    """segs [B, cap, 5] (the flags word as float32 bits), seg_counts [B], layer_first [B, G + 1] as
    ops.raster_segments_layers returns them with every mode FILL -> (area int64 [B, G], inter int64 [B, G, G], borderline int64
    [B, G, G]: the samples that are borderline for group i or for group j; the diagonal: for group i); with_on_line: also the
    samples, counted the same way, that lie exactly on the line of a chord of group i or j (e == 0 in float64)"""
    segs = np.ascontiguousarray(np.asarray(segs, dtype=np.float32))
    seg_counts, layer_first = np.asarray(seg_counts), np.asarray(layer_first)
    B, G = layer_first.shape[0], layer_first.shape[1] - 1
    area = np.zeros((B, G), dtype=np.int64)
    inter = np.zeros((B, G, G), dtype=np.int64)
    borderline = np.zeros((B, G, G), dtype=np.int64)
    exact = np.zeros((B, G, G), dtype=np.int64)
    for b in range(B):
        cnt = int(seg_counts[b])
        rec = segs[b, :cnt, :4].astype(np.float64)
        flags = segs[b, :cnt, 4].copy().view(np.int32)
        by = end_y(rec, flags)
        first = np.clip(layer_first[b].astype(np.int64), 0, cnt)
        ins, bor, onl = [], [], []
        for g in range(G):
            i, b_, o = group_membership(rec[first[g]:first[g + 1]], by[first[g]:first[g + 1]], samples, evenodd)
            ins.append(i)
            bor.append(b_)
            onl.append(o)
        for i in range(G):
            area[b, i] = ins[i].sum()
            for j in range(G):
                inter[b, i, j] = (ins[i] & ins[j]).sum()
                borderline[b, i, j] = (bor[i] | bor[j]).sum()
                exact[b, i, j] = (onl[i] | onl[j]).sum()
    return (area, inter, borderline, exact) if with_on_line else (area, inter, borderline)


def is_clockwise(commands, args):
    """commands [S], args [S, 11] of one group -> SVGPath.is_clockwise over its drawing rows (`l` = 1, `c` = 2) as the
    rasteriser reads them: the start of a row is the end position of the row before it, (0, 0) on row 0; coordinates are read
    as float32; the determinant sum in float64, one operation at a time"""
    cmd = np.asarray(commands).astype(np.int64)
    arg = np.asarray(args).astype(np.float32).astype(np.float64)
    terms, single = [], True
    for t in range(cmd.shape[0]):
        if cmd[t] not in (1, 2):
            continue
        s = arg[t - 1, 9:11] if t else np.zeros(2)
        e = arg[t, 9:11]
        if not terms:
            single = (s[0], s[1]) <= (e[0], e[1])
        terms.append(s[0] * e[1] - s[1] * e[0])
    if len(terms) == 1:
        return bool(single)
    det = 0.0
    for v in terms:
        det += v
    return bool(det >= 0.0)


def filling_from_counts(area, inter, clockwise, participating, threshold=0.9, rule="evenodd", order="ascending"):
    """one icon: area [G], inter [G, G], clockwise [G], participating [G] -> dict of lists: filling, depth, parent,
    paint_order.  `order` is the order inside a level, of the current groups and of their neighbours alike"""
    assert rule in ("evenodd", "orientation") and order in ("ascending", "descending")
    G = len(area)
    part = [bool(participating[i]) and int(area[i]) > 0 for i in range(G)]
    covers = [set() for _ in range(G)]          # covers[j]: the groups j covers (edges j -> i)
    under = [set() for _ in range(G)]           # under[i]: the groups that cover i
    for i in range(G):
        for j in range(G):
            if i != j and part[i] and part[j] and float(int(inter[i][j])) > float(threshold) * float(int(area[i])):
                covers[j].add(i)
                under[i].add(j)
    key = (lambda v: v) if order == "ascending" else (lambda v: -v)
    filling, depth, parent = [OUTLINE] * G, [-1] * G, [-1] * G
    alive = {i for i in range(G) if part[i]}
    roots = [i for i in range(G) if part[i] and not under[i]]
    for root in roots:
        current = [(1, root, -1)]
        level = 0
        while current:
            visited, neighbours = set(), []
            for d, n, via in sorted(current, key=lambda v: key(v[1])):
                filling[n] = FILL if d != 0 else ERASE
                depth[n], parent[n] = level, via
                for n2 in sorted(covers[n] & alive, key=key):
                    if n2 not in visited:
                        visited.add(n2)
                        if rule == "evenodd":
                            d2 = 1 - d
                        else:
                            d2 = d + (1 if bool(clockwise[n2]) == bool(clockwise[n]) else -1)
                        neighbours.append((d2, n2, n))
            alive -= {n for _, n, _ in current}
            current = [(d, n, via) for d, n, via in neighbours if not (under[n] & alive)]
            level += 1
    rank = sorted(range(G), key=lambda i: (filling[i] == OUTLINE, depth[i] if filling[i] != OUTLINE else 0, i))
    return {"filling": filling, "depth": depth, "parent": parent, "paint_order": rank}


def compute_filling(segs, seg_counts, layer_first, commands, args, samples=128, rule="evenodd", threshold=0.9, evenodd=False,
                    closed=None):
    """the whole op from records: commands [N, G, S], args [N, G, S, 11] -> dict of int64 arrays [N, G] (+ area, inter)"""
    commands, args = np.asarray(commands), np.asarray(args)
    N, G = commands.shape[:2]
    area, inter, _ = overlap_counts(segs, seg_counts, layer_first, samples, evenodd)
    out = {k: np.zeros((N, G), dtype=np.int64) for k in ("filling", "depth", "parent", "paint_order", "clockwise")}
    for b in range(N):
        cw = [is_clockwise(commands[b, g], args[b, g]) for g in range(G)]
        part = [True] * G if closed is None else [bool(v) for v in np.asarray(closed)[b]]
        r = filling_from_counts(area[b], inter[b], cw, part, threshold, rule)
        for k, v in r.items():
            out[k][b] = v
        out["clockwise"][b] = cw
    out["area"], out["inter"] = area, inter
    return out


def counts_from_adjacency(adj):
    """adj [G, G] with adj[j, i] != 0 for an edge j -> i ("j covers i") -> synthetic (area, inter) that give exactly these
    edges at any threshold in (0, 1): every area is 100, inter[i, j] is 100 where j covers i and 0 elsewhere"""
    adj = np.asarray(adj)
    G = adj.shape[0]
    area = np.full(G, 100, dtype=np.int32)
    inter = np.ascontiguousarray(np.where(adj.T != 0, 100, 0).astype(np.int32))
    inter[np.arange(G), np.arange(G)] = 100
    return area, inter
