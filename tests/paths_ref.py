"""float64 restatement of deepsvg_amd.paths.canonicalize (csrc/paths.hip; include/dsvg.h has the definition): the reference's
SVG.canonicalize() on padded command / argument arrays, in plain Python, one icon and one row at a time.  Written from the
definition, not from the reference's code; tests/golden/paths/canonicalize.npz holds what the reference itself returns and
tests/test_paths_host.py compares the two.  numpy in, numpy out: no torch, no device."""
import math

import numpy as np

M, L, C, A, EOS, SOS, Z = range(7)
N_ARGS = 11
MAX_ROWS = 2048


def _close(s, e):
    """np.allclose of one coordinate, in float64"""
    return abs(s - e) <= 1e-8 + 1e-5 * abs(e)


def _norm32(x, y):
    """the fp32 norm of a start point: products, sum and root each rounded to fp32"""
    x, y = np.float32(x), np.float32(y)
    return np.sqrt(np.float32(np.float32(x * x) + np.float32(y * y)), dtype=np.float32)


def _norms_close(p, q):
    npf, nq = _norm32(*p), _norm32(*q)
    d = abs(float(np.float32(npf - nq)))
    return d <= 1e-8 + 1e-5 * abs(float(nq))


def _left_of(p, q):
    """step 3: does a command starting at p replace the best so far, which starts at q"""
    if p[1] == q[1]:
        return p[0] < q[0]
    return p[1] < q[1] or (p[0] < q[0] and _norms_close(p, q))


def split_icon(commands, args):
    """steps 1 and 2 on one icon: commands [G, S], args [G, S, 11] -> (sub-paths in reading order, has_arc).  A sub-path is a
    dict: group, closed, n_raw (its drawing rows before the degeneracy test) and cmds, a list of (row, command, start, end) with
    start / end as pairs of Python floats and row the (group, index) of the input row the command came from"""
    G, S = commands.shape
    paths, has_arc = [], False
    for g in range(G):
        cur = None
        for r in range(S):
            c = int(commands[g, r])
            if c == EOS:
                break
            if c == A:
                has_arc = True
            if c == M:
                if cur is not None:
                    paths.append(cur)
                cur = {"group": g, "closed": False, "cmds": [], "n_raw": 0}
            elif c == Z:
                if cur is not None:
                    cur["closed"] = True
                    paths.append(cur)
                cur = None
            elif c in (L, C) and cur is not None:
                s = (float(args[g, r - 1, 9]), float(args[g, r - 1, 10]))
                e = (float(args[g, r, 9]), float(args[g, r, 10]))
                cur["n_raw"] += 1
                if not (_close(s[0], e[0]) and _close(s[1], e[1])):
                    cur["cmds"].append(((g, r), c, s, e))
        if cur is not None:
            paths.append(cur)
    return [p for p in paths if p["cmds"]], has_arc


def canonical_paths(commands, args):
    """steps 1-5 on one icon -> (list of output groups in output order, has_arc).  An output group is a dict: group (the input
    group), reversed, closed, dropped (degenerate commands removed), rows: a list of (command, ((group, row), column) * k)
    naming the input elements each output row copies into its enabled slots, in slot order"""
    paths, has_arc = split_icon(commands, args)
    for p in paths:
        cmds = p["cmds"]
        if p["closed"]:
            best = 0
            for i in range(1, len(cmds)):
                if _left_of(cmds[i][2], cmds[best][2]):
                    best = i
            cmds = cmds[best:] + cmds[:best]
        p["cmds"] = cmds
    paths.sort(key=lambda p: (p["cmds"][0][2][1], p["cmds"][0][2][0]))          # stable
    out = []
    for p in paths:
        cmds = p["cmds"]
        if len(cmds) == 1:
            cw = cmds[0][2] <= cmds[0][3]
        else:
            det = 0.0
            for _, _, s, e in cmds:
                det += s[0] * e[1] - s[1] * e[0]
            cw = det >= 0.0
        # every value as (input row, column): the start of a command is the end position of the row before it
        def start(k):
            (g, r) = k[0]
            return [((g, r - 1), 9), ((g, r - 1), 10)]

        def end(k):
            return [(k[0], 9), (k[0], 10)]

        def ctrl(k, which):
            return [(k[0], 5 + 2 * which), (k[0], 6 + 2 * which)]

        rows = []
        if cw:
            rows.append((M, start(cmds[0])))
            for k in cmds:
                rows.append((k[1], (ctrl(k, 0) + ctrl(k, 1) if k[1] == C else []) + end(k)))
        else:
            rows.append((M, end(cmds[-1])))
            for k in reversed(cmds):
                rows.append((k[1], (ctrl(k, 1) + ctrl(k, 0) if k[1] == C else []) + start(k)))
        out.append({"group": p["group"], "reversed": not cw, "closed": p["closed"], "rows": rows,
                    "dropped": p["n_raw"] - len(cmds),
                    "gap": p["closed"] and cmds[-1][3] != cmds[0][2]})
    return out, has_arc


def numericalize_value(v, n, integer):
    if integer:
        return min(max(int(v), 0), n - 1)
    v = np.float32(v)
    return np.float32(min(max(np.round(v), np.float32(0)), np.float32(n - 1)))      # np.round: half to even


def numericalize(args, commands, n=256):
    """the elementwise step on its own: enabled slots of m / l / c rows -> clip(round_half_even(v), 0, n - 1)"""
    args = np.array(args)
    integer = args.dtype.kind in "iu"
    flat_c, flat_a = np.asarray(commands).reshape(-1), args.reshape(-1, N_ARGS)
    for i, c in enumerate(flat_c):
        c = int(c)
        cols = range(9, 11) if c in (M, L) else range(5, 11) if c == C else ()
        for col in cols:
            flat_a[i, col] = numericalize_value(flat_a[i, col], n, integer)
    return flat_a.reshape(args.shape)


def canonicalize(commands, args, max_num_groups=None, max_seq_len=None, layout="grouped", numericalize=None):
    """numpy restatement of deepsvg_amd.paths.canonicalize: float32 or int64 arrays in, the same seven outputs as numpy arrays"""
    commands, args = np.asarray(commands), np.asarray(args)
    if commands.dtype != args.dtype or commands.dtype not in (np.float32, np.int64):
        commands, args = commands.astype(np.float32), args.astype(np.float32)
    if commands.ndim == 2:
        commands, args = commands[:, None], args[:, None]
        assert max_num_groups is not None
    N, G, S = commands.shape
    assert args.shape == (N, G, S, N_ARGS) and G * S <= MAX_ROWS
    G_out = G if max_num_groups is None else max_num_groups
    S_out = S if max_seq_len is None else max_seq_len + 2
    integer = commands.dtype == np.int64
    dt = commands.dtype
    rows_out = (G_out, S_out) if layout == "grouped" else (S_out,)
    assert layout in ("grouped", "concat")
    oc = np.full((N,) + rows_out, EOS, dtype=dt)
    oc[..., 0] = SOS
    oa = np.full((N,) + rows_out + (N_ARGS,), -1, dtype=dt)
    n_groups = np.zeros(N, np.int32)
    len_groups = np.zeros((N, G_out), np.int32)
    source_group = np.full((N, G_out), -1, np.int32)
    reversed_ = np.zeros((N, G_out), bool)
    valid = np.zeros(N, bool)
    for b in range(N):
        groups, has_arc = canonical_paths(commands[b], args[b])
        lens = [len(g["rows"]) for g in groups]
        fits = all(n <= S_out - 2 for n in lens) if layout == "grouped" else sum(lens) <= S_out - 2
        if has_arc or len(groups) > G_out or not fits:
            continue
        valid[b] = True
        n_groups[b] = len(groups)
        at = 1
        for k, grp in enumerate(groups):
            len_groups[b, k], source_group[b, k], reversed_[b, k] = lens[k], grp["group"], grp["reversed"]
            for i, (c, srcs) in enumerate(grp["rows"]):
                where = (b, k, 1 + i) if layout == "grouped" else (b, at)
                at += 1
                oc[where] = c
                for col, ((g, r), scol) in zip(range(N_ARGS - len(srcs), N_ARGS), srcs):
                    v = args[b, g, r, scol]
                    oa[where + (col,)] = v if numericalize is None else numericalize_value(v, numericalize, integer)
    return {"commands": oc, "args": oa, "n_groups": n_groups, "len_groups": len_groups, "source_group": source_group,
            "reversed": reversed_, "valid": valid}


def icon_facts(commands, args):
    """per icon of an (N, G, S) batch: (nothing dropped and no closed sub-path with a gap, has_arc) - the icons whose drawn
    geometry the op preserves"""
    out = []
    for b in range(commands.shape[0]):
        groups, has_arc = canonical_paths(np.asarray(commands[b]), np.asarray(args[b]))
        out.append((all(g["dropped"] == 0 and not g["gap"] for g in groups), has_arc))
    return out


def decisive(commands, args):
    """[N] bool: every closeness test of steps 2 and 3 is outside the band [0.5, 2] x its threshold, and every determinant sum
    is at least 1e-4 of the sum of the magnitudes of its terms (sub-paths of one command: no sum, always decisive) - the
    icons on which float32 rounding cannot change a decision"""
    commands, args = np.asarray(commands), np.asarray(args)
    if commands.ndim == 2:
        commands, args = commands[:, None], args[:, None]

    def band(d, thr):
        return 0.5 * thr <= d <= 2.0 * thr

    res = np.ones(commands.shape[0], bool)
    for b in range(commands.shape[0]):
        G, S = commands[b].shape
        ok = True
        # step 2: every drawing row's closeness test (rows that are ignored anyway included: harmless)
        for g in range(G):
            for r in range(1, S):
                c = int(commands[b, g, r])
                if c == EOS:
                    break
                if c in (L, C):
                    for col in (9, 10):
                        s, e = float(args[b, g, r - 1, col]), float(args[b, g, r, col])
                        ok &= not band(abs(s - e), 1e-8 + 1e-5 * abs(e))
        paths, _ = split_icon(commands[b], args[b])
        for p in paths:
            cmds = p["cmds"]
            if p["closed"]:                     # step 3: the norm test between every pair the scan could compare
                for i in range(len(cmds)):
                    for j in range(len(cmds)):
                        ni, nj = math.hypot(*cmds[i][2]), math.hypot(*cmds[j][2])
                        ok &= not band(abs(ni - nj), 1e-8 + 1e-5 * abs(nj))
            if len(cmds) > 1:
                terms = [s[0] * e[1] - s[1] * e[0] for _, _, s, e in cmds]
                mags = sum(abs(s[0] * e[1]) + abs(s[1] * e[0]) for _, _, s, e in cmds)
                ok &= abs(sum(terms)) >= 1e-4 * mags
        res[b] = ok
    return res


def golden_expected(gold, layout="grouped", rounded=False, dtype=np.float32):
    """what the reference returned for the icons of tests/golden/paths/canonicalize.npz, laid out as the op lays it out with
    max_num_groups = GO and max_seq_len = LO (grouped) or the longest total (concat), where every icon is valid
    -> (max_num_groups, max_seq_len, {"commands", "args", "n_groups", "len_groups"})"""
    oc, oa = gold["out_commands"], gold["out_args_256" if rounded else "out_args"]
    n, ln = gold["out_n"], gold["out_len"]
    N, GO, LO = oc.shape
    max_seq_len = LO if layout == "grouped" else int(ln.sum(1).max())
    rows = (GO, max_seq_len + 2) if layout == "grouped" else (max_seq_len + 2,)
    ec = np.full((N,) + rows, EOS, dtype=dtype)
    ec[..., 0] = SOS
    ea = np.full((N,) + rows + (N_ARGS,), -1, dtype=dtype)
    for b in range(N):
        at = 1
        for k in range(n[b]):
            for i in range(ln[b, k]):
                where = (b, k, 1 + i) if layout == "grouped" else (b, at)
                at += 1
                ec[where] = oc[b, k, i]
                ea[where] = oa[b, k, i]
    return GO, max_seq_len, {"commands": ec, "args": ea, "n_groups": n.astype(np.int32), "len_groups": ln.astype(np.int32)}


def random_float_icons(n, G=4, S=16, seed=0):
    """icons with float32 coordinates uniform in [0, 256): per group SOS, a random mix of m / l / c / z rows that starts
    with an m, EOS padding -> commands float32 [n, G, S], args float32 [n, G, S, 11]"""
    rng = np.random.default_rng(seed)
    cmd = np.full((n, G, S), EOS, np.float32)
    arg = np.full((n, G, S, N_ARGS), -1.0, np.float32)
    cmd[:, :, 0] = SOS
    for b in range(n):
        for g in range(G):
            rows = int(rng.integers(0, S - 1))
            for r in range(1, 1 + rows):
                c = M if r == 1 else int(rng.choice([M, L, L, L, C, C, C, Z]))
                cmd[b, g, r] = c
                if c in (M, L):
                    arg[b, g, r, 9:11] = rng.uniform(0, 256, 2).astype(np.float32)
                elif c == C:
                    arg[b, g, r, 5:11] = rng.uniform(0, 256, 6).astype(np.float32)
    np.clip(arg, -1.0, np.float32(255.99998), out=arg)
    return cmd, arg
