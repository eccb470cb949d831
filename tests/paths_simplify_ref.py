"""float64 restatement of deepsvg_amd.paths.simplify and deepsvg_amd.paths.simplify_heuristic (csrc/paths_simplify.hip;
include/dsvg.h has the definition): the reference's SVGPath.simplify - Schneider's curve fit with Newton reparametrisation
plus Ramer-Douglas-Peucker - on padded command / argument arrays, in plain Python, one icon, one run and one point at a
time.  Written from the definition, not from the reference's code; every arithmetic operation is a Python float operation
in the order the header states (Python never fuses a multiply with an add), the two stated summation orders included, and
every written value is rounded to float32 once.  tests/golden/paths/simplify.npz holds what the reference itself returns
and tests/test_paths_simplify_host.py compares the two.  numpy in, numpy out: no torch, no device.

`trace`, when a dict is passed, records the smallest relative margin of every kind of decision the fit took - the golden
generator screens its candidates with it (the reference computes with float32 points, so near-ties decide differently)."""
import math

import numpy as np

try:
    from .paths_expand_ref import split as split_ref
except ImportError:                                                   # run as a script's sibling (tests/golden/make_golden_*.py)
    from paths_expand_ref import split as split_ref

M, L, C, A, EOS, SOS, Z = range(7)
N_ARGS = 11
MAX_ROWS = 2048
UNIT = 256 / 24
EPS12 = 1e-12
MACHINE_EPSILON = 1.12e-16


class _Bad(Exception):
    """the icon is invalid: a direction between two points at distance 0, or a value that is not finite"""


def _close(s, e):
    return abs(s - e) <= 1e-8 + 1e-5 * abs(e)


def _div(a, b):
    """IEEE division: Python raises on a zero divisor"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _norm(dx, dy):
    return math.sqrt(dx * dx + dy * dy)


def _margin(trace, kind, value, threshold, scale=None):
    """relative distance of a value from the threshold it is compared with"""
    if trace is None:
        return
    s = max(abs(value), abs(threshold)) if scale is None else scale
    m = abs(value - threshold) / s if s > 0 and math.isfinite(s) else math.inf
    if m == m:
        trace[kind] = min(trace.get(kind, math.inf), m)


def strided_sum(terms):
    """definition point 5 (b): 64 strided partials in ascending order from 0.0, combined by halving"""
    part = [0.0] * 64
    for i, t in enumerate(terms):
        part[i % 64] = part[i % 64] + t
    d = 32
    while d >= 1:
        for j in range(d):
            part[j] = part[j] + part[j + d]
        d //= 2
    return part[0]


def bezier(p0, c1, c2, p3, t):
    w = 1.0 - t
    b0, b1, b2, b3 = (w * w) * w, (3.0 * (w * w)) * t, (3.0 * w) * (t * t), (t * t) * t
    return ((b0 * p0 + b1 * c1) + b2 * c2) + b3 * p3


def _d1(p0, c1, c2, p3, t):
    w = 1.0 - t
    return ((3.0 * (w * w)) * (c1 - p0) + ((6.0 * w) * t) * (c2 - c1)) + (3.0 * (t * t)) * (p3 - c2)


def _d2(p0, c1, c2, p3, t):
    w = 1.0 - t
    return (6.0 * w) * ((c2 - 2.0 * c1) + p0) + (6.0 * t) * ((p3 - 2.0 * c2) + c1)


class _Run:
    """one sub-path: points P (reference units, float64), the chord table, and the rows it emits"""

    def __init__(self, P, tolerance, epsilon, trace):
        self.P, self.tol, self.eps, self.trace = P, tolerance, epsilon, trace
        self.Lc = [0.0]
        for i in range(1, len(P)):                                    # 5 (a): once per sub-path, ascending
            self.Lc.append(self.Lc[-1] + _norm(P[i][0] - P[i - 1][0], P[i][1] - P[i - 1][1]))
        self.rows = []                                                # ("l", point) / ("c", point, c1x, c1y, c2x, c2y)

    def _unit_vector(self, a, b):
        """normalize(P[a] - P[b])"""
        vx, vy = self.P[a][0] - self.P[b][0], self.P[a][1] - self.P[b][1]
        n = _norm(vx, vy)
        if n == 0.0:
            raise _Bad
        return _div(vx, n), _div(vy, n)

    def tangents(self, first, last, jf, jl):
        """point 6: recomputed from integers - the end tangents of the job [jf, jl], or +/- the centre tangent of a split"""
        if first == jf:
            t1 = self._unit_vector(first + 1, first)
        else:
            cx, cy = self._unit_vector(first - 1, first + 1)
            t1 = (-cx, -cy)
        t2 = self._unit_vector(last - 1, last) if last == jl else self._unit_vector(last - 1, last + 1)
        return t1, t2

    # ---- Ramer-Douglas-Peucker -------------------------------------------------------------------------------------
    def dist_to_line(self, i, a, b):
        (px, py), (ax, ay), (bx, by) = self.P[i], self.P[a], self.P[b]
        if _close(ax, bx) and _close(ay, by):
            return _norm(px - ax, py - ay)
        dx, dy = bx - ax, by - ay
        return _div(abs(dx * (ay - py) - dy * (ax - px)), _norm(dx, dy))

    def _runner_up(self, values, best):
        """trace: how far the second largest value is below the largest, where the index of the largest is used"""
        if self.trace is not None and len(values) > 1:
            _margin(self.trace, "argmax", sorted(v for v in values if v == v)[-2], best)

    def rdp(self, first, last):
        stack = [(first, last)]
        while stack:
            f, l = stack.pop()
            best, idx, dists = 0.0, -1, []
            for i in range(f + 1, l):
                d = self.dist_to_line(i, f, l)
                dists.append(d)
                if d >= best:
                    best, idx = d, i
            if idx >= 0:
                _margin(self.trace, "rdp", best, self.eps)
            if best > self.eps:
                self._runner_up(dists, best)
                stack.append((idx, l))
                stack.append((f, idx))
            else:
                self.rows.append(("l", l))

    # ---- Schneider's fit ---------------------------------------------------------------------------------------------
    def generate(self, first, last, u, t1, t2):
        P = self.P
        (p1x, p1y), (p2x, p2y) = P[first], P[last]
        c00, c01, c11, x0, x1 = [], [], [], [], []
        for i in range(last - first + 1):
            ui = u[i]
            t = 1.0 - ui
            b = (3.0 * ui) * t
            b0, b1, b2, b3 = (t * t) * t, b * t, b * ui, (ui * ui) * ui
            a1x, a1y, a2x, a2y = t1[0] * b1, t1[1] * b1, t2[0] * b2, t2[1] * b2
            tx = (P[first + i][0] - p1x * (b0 + b1)) - p2x * (b2 + b3)
            ty = (P[first + i][1] - p1y * (b0 + b1)) - p2y * (b2 + b3)
            c00.append(a1x * a1x + a1y * a1y)
            c01.append(a1x * a2x + a1y * a2y)
            c11.append(a2x * a2x + a2y * a2y)
            x0.append(a1x * tx + a1y * ty)
            x1.append(a2x * tx + a2y * ty)
        c00, c01, c11, x0, x1 = (strided_sum(v) for v in (c00, c01, c11, x0, x1))
        det = c00 * c11 - c01 * c01
        _margin(self.trace, "det", abs(det), EPS12)
        if c00 * c11 > 0:
            _margin(self.trace, "cond", abs(det) / (c00 * c11), 0.0, scale=1.0)
        if abs(det) > EPS12:
            det_c0x = c00 * x1 - c01 * x0
            det_xc1 = x0 * c11 - x1 * c01
            al1, al2 = _div(det_xc1, det), _div(det_c0x, det)
        else:
            s0, s1 = c00 + c01, c01 + c11
            al1 = al2 = _div(x0, s0) if abs(s0) > EPS12 else (_div(x1, s1) if abs(s1) > EPS12 else 0.0)
        seg = _norm(p2x - p1x, p2y - p1y)
        cut = EPS12 * seg
        if self.trace is not None and seg > 0:
            _margin(self.trace, "alpha", min(al1, al2), cut, scale=seg)
        if al1 < cut or al2 < cut:
            al1 = al2 = seg / 3.0
        else:
            lx, ly = p2x - p1x, p2y - p1y
            h1x, h1y, h2x, h2y = t1[0] * al1, t1[1] * al1, t2[0] * al2, t2[1] * al2
            lhs = (h1x * lx + h1y * ly) - (h2x * lx + h2y * ly)
            _margin(self.trace, "handle", lhs, seg * seg)
            if lhs > seg * seg:
                al1 = al2 = seg / 3.0
        return (p1x + t1[0] * al1, p1y + t1[1] * al1, p2x + t2[0] * al2, p2y + t2[1] * al2)

    def max_error(self, first, last, ctrl, u):
        P = self.P
        (p1x, p1y), (p2x, p2y) = P[first], P[last]
        best, idx = 0.0, -1
        self.errors = []
        for i in range(1, last - first):
            qx = bezier(p1x, ctrl[0], ctrl[2], p2x, u[i])
            qy = bezier(p1y, ctrl[1], ctrl[3], p2y, u[i])
            d = _norm(qx - P[first + i][0], qy - P[first + i][1])
            d = d * d
            self.errors.append(d)
            if d >= best:
                best, idx = d, first + i
        if idx < 0:
            raise _Bad                                                # every distance is a NaN
        return best, idx

    def reparametrize(self, first, last, ctrl, u):
        P = self.P
        (p1x, p1y), (p2x, p2y) = P[first], P[last]
        for i in range(last - first + 1):
            t = u[i]
            fx = bezier(p1x, ctrl[0], ctrl[2], p2x, t) - P[first + i][0]
            fy = bezier(p1y, ctrl[1], ctrl[3], p2y, t) - P[first + i][1]
            ax, ay = _d1(p1x, ctrl[0], ctrl[2], p2x, t), _d1(p1y, ctrl[1], ctrl[3], p2y, t)
            bx, by = _d2(p1x, ctrl[0], ctrl[2], p2x, t), _d2(p1y, ctrl[1], ctrl[3], p2y, t)
            num = fx * ax + fy * ay
            den = (ax * ax + ay * ay) + (fx * bx + fy * by)
            if not (-MACHINE_EPSILON <= den <= MACHINE_EPSILON):
                u[i] = t - _div(num, den)
        ordered = True
        for i in range(1, len(u)):
            if self.trace is not None:
                self.trace["order"] = min(self.trace.get("order", math.inf), abs(u[i] - u[i - 1]))
            if u[i] <= u[i - 1]:
                ordered = False
        return ordered

    def fit(self, jf, jl):
        P = self.P
        stack = [(jf, jl)]
        while stack:
            first, last = stack.pop()
            t1, t2 = self.tangents(first, last, jf, jl)
            (p1x, p1y), (p2x, p2y) = P[first], P[last]
            if last - first == 1:
                d = _norm(p1x - p2x, p1y - p2y) / 3.0
                self.rows.append(("c", last, p1x + d * t1[0], p1y + d * t1[1], p2x + d * t2[0], p2y + d * t2[1]))
                continue
            total = self.Lc[last] - self.Lc[first]
            if total == 0.0:
                raise _Bad
            u = [_div(self.Lc[first + i] - self.Lc[first], total) for i in range(last - first + 1)]
            limit = max(self.tol, self.tol * self.tol)
            ordered, accepted, split = True, False, -1
            for _ in range(5):
                ctrl = self.generate(first, last, u, t1, t2)
                err, split = self.max_error(first, last, ctrl, u)
                if ordered:
                    _margin(self.trace, "accept", err, self.tol)
                if err < self.tol and ordered:
                    self.rows.append(("c", last) + ctrl)
                    accepted = True
                    break
                _margin(self.trace, "limit", err, limit)
                if err >= limit:
                    break
                ordered = self.reparametrize(first, last, ctrl, u)
                limit = err
            if not accepted:
                self._runner_up(self.errors, err)
                stack.append((split, last))
                stack.append((first, split))


def _break(prev, cur, start, cos_threshold, unit, trace):
    """definition point 2: does the segment break between the `c` row prev (args) and the `c` row cur that starts at `start`"""
    t1x = 3.0 * (float(prev[9]) / unit - float(prev[7]) / unit)
    t1y = 3.0 * (float(prev[10]) / unit - float(prev[8]) / unit)
    t2x = -(3.0 * (float(cur[5]) / unit - start[0]))
    t2y = -(3.0 * (float(cur[6]) / unit - start[1]))
    n1, n2 = _norm(t1x, t1y), _norm(t2x, t2y)
    if n1 <= 1e-8 or n2 <= 1e-8:
        return True
    c = _div(t1x, n1) * _div(t2x, n2) + _div(t1y, n1) * _div(t2y, n2)
    c = -1.0 if c < -1.0 else (1.0 if c > 1.0 else c)
    if trace is not None:                                             # the margin in degrees: cos is flat at 180
        _margin(trace, "break", math.degrees(math.acos(c)), math.degrees(math.acos(cos_threshold)))
    return c > cos_threshold


def simplify_run(cmds, rows_args, start, tolerance, epsilon, cos_threshold, force_smooth, unit, trace=None):
    """one sub-path: cmds (L / C per row), rows_args float32 [n, 11], start (x, y) as read -> rows ("l", i) / ("c", i, c1x,
    c1y, c2x, c2y) with i the point index (0 = the start, k = the end of row k - 1) and controls in reference units"""
    n = len(cmds)
    P = [(float(start[0]) / unit, float(start[1]) / unit)] + \
        [(float(a[9]) / unit, float(a[10]) / unit) for a in rows_args]
    run = _Run(P, tolerance, epsilon, trace)
    if force_smooth:
        run.fit(0, n)
        return run.rows
    segments, cur = [], []
    for i in range(n):
        if cmds[i] == L:
            if cur:
                segments.append(cur)
                cur = []
            continue
        if cur and _break(rows_args[i - 1], rows_args[i], P[i], cos_threshold, unit, trace):
            segments.append(cur)
            cur = []
        cur.append(i)
    if cur:
        segments.append(cur)
    at = 0
    for seg in segments:
        run.rdp(at, seg[0])
        run.fit(seg[0], seg[-1] + 1)
        at = seg[-1] + 1
    run.rdp(at, n)
    return run.rows


def simplify_icon(commands, args, s_out, tolerance, epsilon, cos_threshold, force_smooth, unit, trace=None):
    """one icon: commands [G, S], args [G, S, 11] float32 -> (rows per group: lists of (command, args float32 [11], source
    row), ok)"""
    G, S = commands.shape
    groups, ok = [], True
    for g in range(G):
        live = []
        for r in range(S):
            cf = float(commands[g, r])
            c = int(cf) if 0.0 <= cf < 7.0 else 7
            if c == EOS:
                break
            live.append(c)
        rows, r = [], 1
        while r < len(live):
            c = live[r]
            if c in (A, 7):
                ok = False
                r += 1
                continue
            if c not in (L, C):
                out = np.full(N_ARGS, -1.0, np.float32)
                if c == M:
                    out[9:11] = args[g, r, 9:11]
                rows.append((c, out, r))
                r += 1
                continue
            e = r
            while e < len(live) and live[e] in (L, C):
                e += 1
            used = [float(v) for v in args[g, r - 1, 9:11]]
            for q in range(r, e):
                used += [float(v) for v in (args[g, q, 9:11] if live[q] == L else args[g, q, 5:11])]
            if not all(math.isfinite(v) for v in used):
                ok = False
            else:
                try:
                    res = simplify_run(live[r:e], args[g, r:e], args[g, r - 1, 9:11], tolerance, epsilon, cos_threshold,
                                       force_smooth, unit, trace)
                except _Bad:
                    ok, res = False, []
                for row in res:
                    src = r - 1 + row[1]
                    out = np.full(N_ARGS, -1.0, np.float32)
                    out[9:11] = args[g, src, 9:11]
                    if row[0] == "c":
                        with np.errstate(all="ignore"):
                            out[5:9] = np.array([v * unit for v in row[2:6]], np.float64).astype(np.float32)
                    rows.append((L if row[0] == "l" else C, out, src))
            r = e
        groups.append(rows)
    if any(len(rows) > s_out - 2 for rows in groups):
        ok = False
    return groups, ok


def simplify(commands, args, tolerance=0.1, epsilon=0.1, angle_threshold=179.0, force_smooth=False, unit=UNIT,
             max_seq_len=None, trace=None):
    """numpy restatement of deepsvg_amd.paths.simplify"""
    commands, args = np.asarray(commands, np.float32), np.asarray(args, np.float32)
    squeeze = commands.ndim == 2
    if squeeze:
        commands, args = commands[:, None], args[:, None]
    N, G, S = commands.shape
    s_out = S if max_seq_len is None else max_seq_len + 2
    assert args.shape == (N, G, S, N_ARGS) and G * S <= MAX_ROWS and G * s_out <= MAX_ROWS and s_out >= 2
    cos_threshold = math.cos(math.radians(float(angle_threshold)))
    oc = np.full((N, G, s_out), EOS, np.float32)
    oc[..., 0] = SOS
    oa = np.full((N, G, s_out, N_ARGS), -1.0, np.float32)
    len_groups = np.zeros((N, G), np.int32)
    source_row = np.full((N, G, s_out), -1, np.int32)
    valid = np.zeros(N, bool)
    for b in range(N):
        groups, ok = simplify_icon(commands[b], args[b], s_out, float(tolerance), float(epsilon), cos_threshold,
                                   bool(force_smooth), float(unit), trace)
        valid[b] = ok
        if not ok:
            continue
        for g, rows in enumerate(groups):
            len_groups[b, g] = len(rows)
            for j, (c, a, r) in enumerate(rows, 1):
                oc[b, g, j], oa[b, g, j], source_row[b, g, j] = c, a, r
    res = {"commands": oc, "args": oa, "len_groups": len_groups, "source_row": source_row, "valid": valid}
    if squeeze:
        res = {k: (v if k == "valid" else v[:, 0]) for k, v in res.items()}
    return res


def simplify_heuristic(commands, args, unit=UNIT, max_seq_len=None, work_seq_len=None):
    """numpy restatement of deepsvg_amd.paths.simplify_heuristic: the three calls by hand"""
    commands = np.asarray(commands, np.float32)
    G = 1 if commands.ndim == 2 else commands.shape[1]
    work = MAX_ROWS // G - 2 if work_seq_len is None else work_seq_len
    a = split_ref(commands, args, max_dist=2 * unit, include_lines=False, max_seq_len=work)
    b = simplify(a["commands"], a["args"], 0.1, 0.2, 150.0, unit=unit, max_seq_len=work)
    c = split_ref(b["commands"], b["args"], max_dist=7.5 * unit,
                  max_seq_len=commands.shape[-1] - 2 if max_seq_len is None else max_seq_len)
    # an icon invalid at one step is handed on as empty groups, which the later steps pass through
    return {"commands": c["commands"], "args": c["args"], "len_groups": c["len_groups"],
            "valid": a["valid"] & b["valid"] & c["valid"]}


# ---- inputs -------------------------------------------------------------------------------------------------------------
def smooth_path(rng, n_cmd, smooth=0.6, lines=0.25, scale=60.0, origin=None):
    """an `m` followed by n_cmd `l` / `c` commands in the 256 box: a `c` behind a `c` continues its tangent with probability
    `smooth` -> list of (command, [values]), at most 3 n_cmd + 1 rows"""
    p = rng.uniform(60, 196, 2) if origin is None else np.asarray(origin, float)
    rows, prev_dir = [(M, list(p))], None
    for _ in range(n_cmd):
        e = np.clip(p + rng.uniform(-scale, scale, 2), 4, 252)
        if rng.random() < lines:                                      # a line, in 1-3 nearly collinear pieces: RDP has something to merge
            k = int(rng.integers(1, 4))
            for i in range(1, k):
                rows.append((L, list(p + (e - p) * (i / k) + rng.uniform(-1, 1, 2))))
            rows.append((L, list(e)))
            prev_dir = None
        else:
            if prev_dir is not None and rng.random() < smooth:
                c1 = p + prev_dir * rng.uniform(5, scale / 2)
            else:
                c1 = p + rng.uniform(-scale / 2, scale / 2, 2)
            c2 = e + rng.uniform(-scale / 2, scale / 2, 2)
            d = e - c2
            prev_dir = d / max(float(np.hypot(*d)), 1e-6)
            rows.append((C, list(c1) + list(c2) + list(e)))
        p = e
    return rows


def pack(icons, G, S):
    """icons: per icon a list of groups, each a list of (command, values) -> commands float32 [n, G, S], args [n, G, S, 11]"""
    cmd = np.full((len(icons), G, S), EOS, np.float32)
    arg = np.full((len(icons), G, S, N_ARGS), -1.0, np.float32)
    cmd[:, :, 0] = SOS
    for b, groups in enumerate(icons):
        assert len(groups) <= G
        for g, rows in enumerate(groups):
            assert len(rows) <= S - 2, (len(rows), S)
            for r, (c, v) in enumerate(rows, 1):
                cmd[b, g, r] = c
                if len(v):
                    arg[b, g, r, N_ARGS - len(v):] = v
    return cmd, arg


def random_batch(n, G, S, seed, max_cmd=4, work=None):
    """seeded icons of smooth paths, pre-split on the host as simplify_heuristic's first step does -> commands [n, G, S],
    args [n, G, S, 11]; every group fits S - 2 rows"""
    rng = np.random.default_rng(seed)
    icons = []
    for _ in range(n):
        groups = []
        for _ in range(G):
            while True:
                rows = smooth_path(rng, int(rng.integers(0, max_cmd + 1))) if rng.random() < 0.9 else []
                cmd, arg = pack([[rows]], 1, max(len(rows) + 2, 2))
                res = split_ref(cmd, arg, max_dist=2 * UNIT, include_lines=False, max_seq_len=S - 2)
                if res["valid"][0]:
                    break
            k = int(res["len_groups"][0, 0])
            groups.append([(int(res["commands"][0, 0, j]),
                            list(res["args"][0, 0, j, {M: 9, L: 9, C: 5}[int(res["commands"][0, 0, j])]:]))
                           for j in range(1, 1 + k)])
        icons.append(groups)
    return pack(icons, G, S)


def enabled(commands):
    """bool [..., 11]: the slots CMD_ARGS_MASK enables for each command"""
    commands = np.asarray(commands).astype(np.int64)
    mask = np.zeros((7, N_ARGS), bool)
    mask[[M, L], 9:11] = True
    mask[C, 5:11] = True
    mask[A, 0:5] = True
    mask[A, 9:11] = True
    return mask[commands]


def _rows_of(res, g=0):
    cmd, arg = res["commands"][0, g], res["args"][0, g]
    return [(int(cmd[j]), list(arg[j, {M: 9, L: 9, C: 5, Z: 11, SOS: 11}[int(cmd[j])]:]))
            for j in range(1, 1 + int(res["len_groups"][0, g]))]


def pieces(cubic, n):
    """an `m` and one cubic (8 values: start, control1, control2, end) cut into n `c` rows: n + 1 points, smooth joins"""
    cmd, arg = pack([[[(M, cubic[:2]), (C, cubic[2:])]]], 1, 4)
    return _rows_of(split_ref(cmd, arg, n=n, max_seq_len=n + 1))


def zigzag(n, seed=5, amplitude=9.0):
    """n `c` rows whose ends alternate around a slope, handles on the chords with some noise: no fit of two intervals
    passes tolerance 0.1, so a fit over all of it recurses down to single intervals"""
    rng = np.random.default_rng(seed)
    p = np.array([12.0, 100.0])
    rows = [(M, list(p))]
    for i in range(n):
        e = np.array([p[0] + 5.0 + rng.uniform(0, 1), 100.0 + 0.4 * i + (amplitude if i % 2 == 0 else -amplitude) + rng.uniform(-1, 1)])
        rows.append((C, list(p + (e - p) * 0.3 + rng.uniform(-0.5, 0.5, 2)) + list(p + (e - p) * 0.7 + rng.uniform(-0.5, 0.5, 2))
                     + list(e)))
        p = e
    return rows


CORNER = [(M, [30.0, 30.0]), (C, [60.0, 10.0, 95.0, 70.0, 120.0, 30.0]), (L, [120.0, 120.0]),
          (C, [90.0, 150.0, 50.0, 95.0, 30.0, 120.0]), (C, [10.0, 100.0, 40.0, 60.0, 80.0, 90.0])]      # c-l-c-c, a corner between the last two
GROWS = [(M, [20.0, 20.0]), (C, [40.0, 5.0, 60.0, 5.0, 80.0, 20.0]), (C, [60.0, 40.0, 60.0, 70.0, 85.0, 90.0]),
         (C, [60.0, 95.0, 40.0, 120.0, 20.0, 100.0])]      # three `c` that meet at corners: 3 fits and 4 empty gaps, 7 rows from 3


def check_properties(commands, args, out, tolerance, epsilon, unit=UNIT):
    """what the definition promises of a result, whoever computed it (numpy arrays, (N, G, S) layout), derived not measured:
    an accepted `c` over >= 2 intervals passes within sqrt(tolerance) * unit of every interior point (its accept test was
    |curve(u_i) - P_i|^2 < tolerance), checked against 2,001 samples of the curve with their polyline's length / 4,000
    for the sampling; an `l` passes within epsilon * unit of every interior point, by the distance RDP itself uses; end
    positions are input values bit for bit through source_row.  -> (rows checked: c over several intervals, l over several)"""
    n_c = n_l = 0
    z = np.linspace(0.0, 1.0, 2001)[:, None]
    for b in range(commands.shape[0]):
        if not out["valid"][b]:
            continue
        for g in range(commands.shape[1]):
            n = int(out["len_groups"][b, g])
            oc, oa, src = out["commands"][b, g], out["args"][b, g], out["source_row"][b, g]
            assert oc[0] == SOS and (oc[1 + n:] == EOS).all() and (src[1 + n:] == -1).all() and src[0] == -1
            for j in range(1, 1 + n):
                c, r = int(oc[j]), int(src[j])
                assert commands[b, g, r] == c or c in (L, C)
                if c in (M, L, C):
                    assert oa[j, 9:11].tobytes() == args[b, g, r, 9:11].tobytes(), (b, g, j)
                if c not in (L, C):
                    continue
                r0 = int(src[j - 1]) if j > 1 else r
                assert r0 <= r
                inner = args[b, g, r0 + 1:r, 9:11].astype(np.float64)
                if not len(inner):
                    continue
                p0, p3 = args[b, g, r0, 9:11].astype(np.float64), oa[j, 9:11].astype(np.float64)
                if c == C:
                    n_c += 1
                    c1, c2 = oa[j, 5:7].astype(np.float64), oa[j, 7:9].astype(np.float64)
                    w = 1.0 - z
                    curve = w ** 3 * p0 + 3 * w ** 2 * z * c1 + 3 * w * z ** 2 * c2 + z ** 3 * p3
                    length = float(np.linalg.norm(np.diff(curve, axis=0), axis=1).sum())
                    d = np.linalg.norm(inner[:, None, :] - curve[None], axis=2).min(axis=1)
                    bound = math.sqrt(tolerance) * unit + length / 4000.0
                    assert d.max() <= bound, (b, g, j, float(d.max()), bound)
                else:
                    n_l += 1
                    run = _Run([(float(x) / unit, float(y) / unit) for x, y in [p0, *inner, p3]], tolerance, epsilon, None)
                    far = max(run.dist_to_line(i, 0, len(inner) + 1) for i in range(1, len(inner) + 1))
                    assert far <= epsilon, (b, g, j, far, epsilon)
    return n_c, n_l
