"""The definition of dsvg_svg_parse (include/dsvg.h) restated in plain Python: SVG path text -> the rows of one group, as the
reference's `SVGPath.from_str(s).to_tensor()` gives them (svglib/svg_path.py:79-157, svg_command.py:51-120,
svg_primitive.py:196-207) reduced to the command and the model's eleven argument columns under CMD_ARGS_MASK.  No `re`, no
reference code: the number pattern is a nine-state automaton written out below, the decimal rule is integer arithmetic and one
float64 operation, and positions are float32 values added in float32, one rounding per add, as the reference's `Point`
holds and adds them (svglib/geom.py:60-137: `np.float32` arrays).  csrc/svg_parse.hip runs the same tables and the same walk.
"""
import struct

import numpy as np

F = np.float32
M, L, C, A, EOS, SOS, Z = range(7)
OK, EMPTY, ARG_COUNT, SLOW_NUMBER, ROWS_OVERFLOW, BAD_SLOT, RANGE = range(7)
KIND_PATH, KIND_POLYLINE, KIND_POLYGON = 0, 1, 2
TILE = 64                                   # bytes of a string a wave of the kernel reads at a time

LETTERS = b"MmZzLlHhVvCcSsQqTtAa"
ARITY = {"m": 2, "l": 2, "t": 2, "h": 1, "v": 1, "c": 6, "s": 4, "q": 4, "a": 7, "z": 0}

# ---- tokens: re.findall(r"[-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?") as an automaton ------------------------------------------
DIGIT, DOT, SIGN, EXP, OTHER = range(5)                                     # byte classes
IDLE, S_SIGN, DOT0, INT, INTDOT, FRAC, EXP0, EXPSIGN, EXPD = range(9)       # states
# NEXT[state][class].  INT, FRAC and EXPD accept; INTDOT and EXP0 lie one byte behind the last accepting state, EXPSIGN two: when
# the number does not go on from there the match ends at the accepting byte (the regex backtracks) and the bytes behind it are
# read again as if from IDLE - which is what the rows of the pending states say, column by column.
NEXT = (
    (INT, DOT0, S_SIGN, IDLE, IDLE),        # IDLE
    (INT, DOT0, S_SIGN, IDLE, IDLE),        # S_SIGN: a sign, nothing yet
    (FRAC, DOT0, S_SIGN, IDLE, IDLE),       # DOT0: [sign] dot, no digit yet
    (INT, INTDOT, S_SIGN, EXP0, IDLE),      # INT
    (FRAC, DOT0, S_SIGN, IDLE, IDLE),       # INTDOT: digits and a dot
    (FRAC, DOT0, S_SIGN, EXP0, IDLE),       # FRAC
    (EXPD, DOT0, EXPSIGN, IDLE, IDLE),      # EXP0: a number and an `e`
    (EXPD, DOT0, S_SIGN, IDLE, IDLE),       # EXPSIGN: a number, an `e` and a sign
    (EXPD, DOT0, S_SIGN, IDLE, IDLE),       # EXPD
)
BEHIND = (0, 0, 0, 0, 1, 0, 1, 2, 0)        # bytes between the last accepting byte and the state
# the classes on which the number a state belongs to goes on
GOES_ON = ((), (), (), (DIGIT, DOT, EXP), (DIGIT,), (DIGIT, EXP), (DIGIT, SIGN), (DIGIT,), (DIGIT,))


def byte_class(b):
    if 0x30 <= b <= 0x39:
        return DIGIT
    if b == 0x2E:
        return DOT
    if b == 0x2B or b == 0x2D:
        return SIGN
    if b == 0x65 or b == 0x45:
        return EXP
    return OTHER


def step(state, cls, i):
    """one byte of class `cls` at index i from `state` -> (next state, end of the number that ends here or -1 (exclusive),
    start of the number that begins here or -1)"""
    nxt = NEXT[state][cls]
    end = i - BEHIND[state] if state >= INT and cls not in GOES_ON[state] else -1
    start = -1
    if nxt == S_SIGN or (nxt == INT and state == IDLE) or (nxt == DOT0 and state != S_SIGN):
        start = i - 1 if state == EXPSIGN and nxt == DOT0 else i           # `4e+.5` is 4 and +.5: the sign starts the second
    return nxt, end, start


def tokens(data, kind=KIND_PATH):
    """bytes -> [("n", start, end) | ("c", letter)] in reading order; a command letter is a token for kind 0 only.  One
    separator is read behind the last byte, so that a number at the end of the string ends"""
    out, state, start = [], IDLE, -1
    for i in range(len(data) + 1):
        b = data[i] if i < len(data) else 0x20
        letter = kind == KIND_PATH and b in LETTERS
        state, end, new = step(state, byte_class(b), i)
        if end >= 0:
            out.append(("n", start, end))
        if new >= 0:
            start = new
        if letter:
            out.append(("c", chr(b)))
    return out


# ---- the value of a number --------------------------------------------------------------------------------------------------
POW10 = [float(10 ** k) for k in range(23)]                                  # exact in float64


def decimal(text):
    """the bytes of one match -> float64, or None outside the fast path (SLOW_NUMBER).  Leading zeros and the trailing zeros of
    the fraction are dropped; the digits left are an integer w < 2^53, e10 = exponent - fraction digits kept, |e10| <= 22; the
    value is w * 10^e10 or w / 10^-e10: one correctly rounded float64 operation on exact operands, which is `float(text)`"""
    i, n = 0, len(text)
    neg = False
    if text[i] in b"+-":
        neg = text[i] == 0x2D
        i += 1
    w, kept, zeros, slow, frac = 0, 0, 0, False, False
    while i < n and text[i] not in b"eE":
        if text[i] == 0x2E:
            frac = True
        else:
            d = text[i] - 0x30
            if frac and d == 0:
                zeros += 1                                                   # kept only when a digit follows
            else:
                for _ in range(zeros + 1 if frac else 1):
                    if w > (2 ** 64 - 1 - 9) // 10:
                        slow = True                                          # the 64-bit accumulator would overflow
                    else:
                        w *= 10
                if frac:
                    kept += zeros + 1
                    zeros = 0
                w += d
        i += 1
    ex, eneg = 0, False
    if i < n:
        i += 1
        if text[i] in b"+-":
            eneg = text[i] == 0x2D
            i += 1
        while i < n:
            ex = min(ex * 10 + (text[i] - 0x30), 100000)
            i += 1
    e10 = (-ex if eneg else ex) - kept
    if slow or w >= 2 ** 53 or abs(e10) > 22:
        return None
    v = float(w) * POW10[e10] if e10 >= 0 else float(w) / POW10[-e10]
    return -v if neg else v


# ---- the walk ------------------------------------------------------------------------------------------------------------------
def _row(cmd, **cols):
    a = np.full(11, -1.0, dtype=F)
    for k, v in cols.items():
        lo = {"arc": 0, "c1": 5, "c2": 7, "end": 9}[k]
        a[lo:lo + len(v)] = v
    return cmd, a


class _Walk:
    """SVGCommand.from_str over the (letter, numbers) list and SVGPath.from_commands(allow_empty=False, add_closing=False) over
    its commands, row by row"""

    def __init__(self):
        self.pos = self.init = (F(0), F(0))
        self.bez = None                     # control2 of the previous command when that was a Bezier
        self.open, self.drawn, self.move = False, False, None
        self.rows = []

    def pt(self, x, y, rel):
        with np.errstate(over="ignore", invalid="ignore"):
            x, y = F(x), F(y)               # a `Point` is float32
            return (x + self.pos[0], y + self.pos[1]) if rel else (x, y)

    def emit(self, row, end, bez=None):
        if self.open:
            if not self.drawn:
                self.rows.append(_row(M, end=self.move))
                self.drawn = True
            self.rows.append(row)
        self.pos, self.bez = end, bez

    def reflect(self):
        if self.bez is None:
            return self.pos
        with np.errstate(over="ignore", invalid="ignore"):
            return (F(2) * self.pos[0] - self.bez[0], F(2) * self.pos[1] - self.bez[1])

    def close(self):
        if self.open and self.drawn:
            self.rows.append(_row(Z))
        self.open = False
        self.pos, self.bez = self.init, None

    def command(self, letter, a, first):
        rel, c = letter.islower(), letter.lower()
        if c == "m" and first:
            self.pos = self.init = self.move = self.pt(a[0], a[1], rel)
            self.bez, self.open, self.drawn = None, True, False
        elif c in "mlhv":
            if c == "h":
                e = (self.pt(a[0], 0.0, rel)[0], self.pos[1])
            elif c == "v":
                e = (self.pos[0], self.pt(0.0, a[0], rel)[1])
            else:
                e = self.pt(a[0], a[1], rel)
            self.emit(_row(L, end=e), e)
        elif c in "csqt":
            if c == "c":
                c1, c2, e = self.pt(a[0], a[1], rel), self.pt(a[2], a[3], rel), self.pt(a[4], a[5], rel)
            elif c == "s":
                c1, c2, e = self.reflect(), self.pt(a[0], a[1], rel), self.pt(a[2], a[3], rel)
            elif c == "q":
                c1 = c2 = self.pt(a[0], a[1], rel)
                e = self.pt(a[2], a[3], rel)
            else:
                c1 = c2 = self.reflect()
                e = self.pt(a[0], a[1], rel)
            self.emit(_row(C, c1=c1, c2=c2, end=e), e, bez=c2)
        else:                               # radii, angle and flags are not translated; a flag is int(value)
            e = self.pt(a[5], a[6], rel)
            with np.errstate(over="ignore"):
                arc = (F(a[0]), F(a[1]), F(a[2]), F(float(int(a[3]))), F(float(int(a[4]))))
            self.emit(_row(A, arc=arc, end=e), e)


def parse(data, kind=KIND_PATH, S=None):
    """one string -> (status, commands int [n], args float32 [n, 11]); rows only with status OK.  S: the rows of a group with
    its frame (None: no bound)"""
    data = bytes(data)
    w = _Walk()
    err = OK                                # the first ARG_COUNT / SLOW_NUMBER in reading order
    letter, nums, cnt, pts = None, [], 0, []

    def end_segment():
        nonlocal err
        if letter is not None and letter not in "zZ" and err == OK and (cnt == 0 or nums):
            err = ARG_COUNT                 # k = 0 included: the reference raises on the empty command list

    for tok in tokens(data, kind):
        if tok[0] == "c":
            end_segment()
            letter, nums, cnt = tok[1], [], 0
            if letter in "zZ" and err == OK:
                w.close()
            continue
        if kind == KIND_PATH and letter is None:
            continue                        # numbers before the first command letter are never converted
        v = decimal(data[tok[1]:tok[2]])
        if err != OK:
            continue
        if v is None:
            err = SLOW_NUMBER
        elif kind != KIND_PATH:
            nums.append(v)
            if len(nums) == 2:
                pts.append(w.pt(nums[0], nums[1], False))
                nums = []
        elif letter in "zZ":
            err = ARG_COUNT
        else:
            nums.append(v)
            if len(nums) == ARITY[letter.lower()]:
                w.command(letter, nums, cnt == 0)
                nums, cnt = [], cnt + 1
    if kind == KIND_PATH:
        end_segment()
    else:
        if nums and err == OK:
            err = ARG_COUNT
        if len(pts) >= 2:
            w.rows = [_row(M, end=pts[0])] + [_row(L, end=p) for p in pts[1:]] + ([_row(Z)] if kind == KIND_POLYGON else [])
    none = (np.zeros(0, dtype=np.int64), np.zeros((0, 11), dtype=F))
    if err != OK:
        return (err,) + none
    if S is not None and len(w.rows) > S - 2:
        return (ROWS_OVERFLOW,) + none
    if not w.rows:
        return (EMPTY,) + none
    cmd = np.array([r[0] for r in w.rows], dtype=np.int64)
    args = np.stack([r[1] for r in w.rows])
    if not np.isfinite(args).all():
        return (RANGE,) + none
    return OK, cmd, args


def parse_paths(data, offsets, kind, slot, N, G, S):
    """the whole call on numpy arrays -> the dict of deepsvg_amd.svgio.parse_paths, as numpy arrays"""
    data = np.asarray(data, dtype=np.uint8).tobytes()
    P = len(kind)
    cmd = np.full((N, G, S), EOS, dtype=F)
    cmd[:, :, 0] = SOS
    args = np.full((N, G, S, 11), -1.0, dtype=F)
    lens = np.zeros((N, G), dtype=np.int32)
    status = np.zeros(P, dtype=np.int32)
    valid = np.ones(N, dtype=bool)
    users = {}
    for p in range(P):
        users.setdefault(int(slot[p]), []).append(p)
    for p in range(P):
        s = int(slot[p])
        if s < -1 or s >= N * G or (s >= 0 and len(users[s]) > 1):
            status[p] = BAD_SLOT
        else:
            lo, hi = min(max(int(offsets[p]), 0), len(data)), min(max(int(offsets[p + 1]), 0), len(data))
            st, c, a = parse(data[lo:max(hi, lo)], int(kind[p]), S)
            status[p] = st
            if st == OK and s >= 0:
                n, g = divmod(s, G)
                cmd[n, g, 1:1 + len(c)], args[n, g, 1:1 + len(c)], lens[n, g] = c, a, len(c)
        if 0 <= s < N * G and status[p] not in (OK, EMPTY):
            valid[s // G] = False
    cmd[~valid, :, 1:], args[~valid], lens[~valid] = EOS, -1.0, 0
    return {"commands": cmd, "args": args, "len_groups": lens, "status": status, "valid": valid}


def bits(x):
    """float32 array -> its bit patterns, for comparisons that tell -0 from 0"""
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def f64_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]
