"""The exact number rule of include/dsvg.h restated in plain Python, integers only, and the restatement of dsvg_svg_parse
(tests/svgio_ref.py) with a choice of rule: `numbers="fast"` is that module unchanged, `numbers="exact"` is its tokens and its
walk with `decimal_exact` in place of its `decimal`.  deepsvg_amd/csrc/decimal_exact.h computes the same bits on the device."""
import contextlib
import struct

from tests import svgio_ref as R

DIGITS, E10_MIN, E10_MAX = 19, -64, 38


def split(text):
    """the bytes of one match of the number pattern -> (negative, w, nd, e10): the digit string without its leading and trailing
    zeros as an integer w of nd digits (0 digits: w = 0), and the decimal exponent of its last digit"""
    i, n = 0, len(text)
    neg = False
    if text[i] in b"+-":
        neg = text[i] == 0x2D
        i += 1
    digits, fraction, frac = b"", 0, False
    while i < n and text[i] not in b"eE":
        if text[i] == 0x2E:
            frac = True
        else:
            digits += text[i:i + 1]
            fraction += frac
        i += 1
    ex, eneg = 0, False
    if i < n:
        i += 1
        if text[i] in b"+-":
            eneg = text[i] == 0x2D
            i += 1
        while i < n:
            ex = min(ex * 10 + (text[i] - 0x30), 100000)            # saturated as the fast rule saturates it
            i += 1
    kept = digits.lstrip(b"0")
    stripped = len(kept) - len(kept.rstrip(b"0"))
    kept = kept.rstrip(b"0")
    return neg, int(kept) if kept else 0, len(kept), (-ex if eneg else ex) - fraction + stripped


def nearest_double_bits(w, e10):
    """w > 0 -> the bits of the float64 nearest to w * 10^e10, ties to even; the result is a normal number on the domain"""
    num, den = (w * 10 ** e10, 1) if e10 >= 0 else (w, 10 ** -e10)
    # scale so that the quotient has 55 or 56 bits: 53 of the mantissa, two or three below it, the remainder is the rest
    shift = 55 - (num.bit_length() - den.bit_length())
    if shift >= 0:
        num <<= shift
    else:
        den <<= -shift
    q, rem = divmod(num, den)
    extra = q.bit_length() - 53                                     # the bits below the mantissa
    mant, low = q >> extra, q & ((1 << extra) - 1)
    half = 1 << (extra - 1)
    if low > half or (low == half and (rem != 0 or mant & 1)):
        mant += 1
    top = 52 + extra - shift                                        # value = mant * 2^(extra - shift)
    if mant >> 53:
        mant >>= 1
        top += 1
    assert 1 <= top + 1023 <= 2046
    return (top + 1023) << 52 | (mant & ((1 << 52) - 1))


def decimal_exact(text):
    """the bytes of one match -> float64, or None outside the exact domain (SLOW_NUMBER)"""
    neg, w, nd, e10 = split(text)
    if w == 0:
        bits = 0
    elif nd > DIGITS or e10 < E10_MIN or e10 > E10_MAX:
        return None
    else:
        bits = nearest_double_bits(w, e10)
    return struct.unpack("<d", struct.pack("<Q", bits | (neg << 63)))[0]


def _rule(numbers):
    if numbers not in ("fast", "exact"):
        raise ValueError(f'numbers is "fast" or "exact"; got {numbers!r}')
    return numbers == "exact"


@contextlib.contextmanager
def _exact_rule():
    """tests/svgio_ref.py reads its rule through its module attribute `decimal`: the walk runs unchanged with another rule"""
    own = R.decimal
    R.decimal = decimal_exact
    try:
        yield
    finally:
        R.decimal = own


def parse(data, kind=R.KIND_PATH, S=None, numbers="fast"):
    if not _rule(numbers):
        return R.parse(data, kind, S)
    with _exact_rule():
        return R.parse(data, kind, S)


def parse_paths(data, offsets, kind, slot, N, G, S, numbers="fast"):
    if not _rule(numbers):
        return R.parse_paths(data, offsets, kind, slot, N, G, S)
    with _exact_rule():
        return R.parse_paths(data, offsets, kind, slot, N, G, S)
