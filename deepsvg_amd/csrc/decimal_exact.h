// The exact rule of include/dsvg.h: the bytes of one number -> the float64 nearest to its value, ties to even, which is strtod
// and Python's float(), for every number of at most DSVG_SVG_EXACT_DIGITS significant digits whose float32 value is finite
// and not zero.  Integers only: no floating-point operation, no 128-bit type, no library call.  Plain C++ for a device compiler
// and a host compiler alike (tests/decimal_exact_check.cpp runs it on the host against strtod); nothing of HIP is included,
// and the function qualifiers sit behind DSVG_HD.
//   w * 10^e10 = w * 5^e10 * 2^e10.  A power of five is a product of at most three table entries 5^0 .. 5^27 (each below 2^63).
//   e10 >= 0   the product w * 5^e10 (at most 64 + 89 bits) in three named 64-bit limbs; its top 64 bits, the rest is sticky.
//   e10 <  0   w shifted up until its top bit is set, then shift-and-subtract long division by 5^-e10 until the quotient has 64
//              bits; the remainder is sticky.  5^k fits one word for k <= 27 (one hardware division starts the quotient, at most
//              64 steps follow); above that the divisor and the remainder are three named limbs (at most 149 steps).
//   then 64 bits -> 53, round to nearest even on (the 11 bits below, sticky), and the bits of the double are put together.
//   Every result is a normal number (1e-64 .. 1e57).
// No array is indexed at run time but the constant table, so nothing here leaves the registers.
#ifndef DSVG_DECIMAL_EXACT_H
#define DSVG_DECIMAL_EXACT_H
#include <stdint.h>
#include "../../include/dsvg.h"         // DSVG_SVG_EXACT_DIGITS, DSVG_SVG_EXACT_E10_MIN, DSVG_SVG_EXACT_E10_MAX

#ifndef DSVG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSVG_HD __host__ __device__ inline
#else
#define DSVG_HD inline
#endif
#endif

namespace dsvg_exact {

struct U192 {                           // l0 the lowest 64 bits
    uint64_t l0, l1, l2;
};

DSVG_HD void mul64(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    lo = (mid << 32) | (uint32_t)p00;
    hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// a * b where the product is known to fit 192 bits
DSVG_HD U192 mul_word(U192 a, uint64_t b) {
    uint64_t h0, h1, h2, x0, x1, x2;
    mul64(a.l0, b, h0, x0);
    mul64(a.l1, b, h1, x1);
    mul64(a.l2, b, h2, x2);
    U192 r;
    r.l0 = x0;
    r.l1 = h0 + x1;
    r.l2 = h1 + x2 + (r.l1 < h0 ? 1ull : 0ull);
    return r;
}

DSVG_HD uint64_t pow5(int k) {          // 0 <= k <= 27
    constexpr uint64_t kPow5[28] = {
        0x1ull, 0x5ull, 0x19ull, 0x7dull, 0x271ull, 0xc35ull, 0x3d09ull, 0x1312dull, 0x5f5e1ull, 0x1dcd65ull, 0x9502f9ull, 0x2e90eddull,
        0xe8d4a51ull, 0x48c27395ull, 0x16bcc41e9ull, 0x71afd498dull, 0x2386f26fc1ull, 0xb1a2bc2ec5ull, 0x3782dace9d9ull,
        0x1158e460913dull, 0x56bc75e2d631ull, 0x1b1ae4d6e2ef5ull, 0x878678326eac9ull, 0x2a5a058fc295edull, 0xd3c21bcecceda1ull,
        0x422ca8b0a00a425ull, 0x14adf4b7320334b9ull, 0x6765c793fa10079dull};
    return kPow5[k];
}

// m with bit 63 set, worth 2^top at that bit, and whether anything non-zero lies below its lowest bit -> the bits of the double
DSVG_HD uint64_t round_pack(uint64_t m, bool sticky, int top) {
    uint64_t mant = m >> 11;
    const uint64_t rem = m & 0x7FFull;
    if (rem > 0x400ull || (rem == 0x400ull && (sticky || (mant & 1ull) != 0))) ++mant;
    if ((mant >> 53) != 0) {
        mant >>= 1;
        ++top;
    }
    return ((uint64_t)(top + 1023) << 52) | (mant & 0xFFFFFFFFFFFFFull);
}

// w != 0, DSVG_SVG_EXACT_E10_MIN <= e10 <= DSVG_SVG_EXACT_E10_MAX -> the bits of the float64 nearest to w * 10^e10
DSVG_HD uint64_t convert(uint64_t w, int e10) {
    if (e10 >= 0) {
        const int a = e10 < 27 ? e10 : 27;
        U192 p = {w, 0ull, 0ull};
        p = mul_word(mul_word(p, pow5(a)), pow5(e10 - a));
        int top = 191;                  // the index of the limbs' top bit
        if (p.l2 == 0) {
            p.l2 = p.l1, p.l1 = p.l0, p.l0 = 0;
            top -= 64;
        }
        if (p.l2 == 0) {
            p.l2 = p.l1, p.l1 = p.l0, p.l0 = 0;
            top -= 64;
        }
        const int lz = __builtin_clzll(p.l2);
        const uint64_t m = lz != 0 ? (p.l2 << lz) | (p.l1 >> (64 - lz)) : p.l2;
        return round_pack(m, ((p.l1 << lz) | p.l0) != 0, top - lz + e10);
    }
    const int k = -e10;
    const int lzw = __builtin_clzll(w);
    const uint64_t wl = w << lzw;       // w = wl * 2^-lzw, and w * 10^e10 = wl / 5^k * 2^(-lzw - k)
    uint64_t q;
    bool sticky;
    int s = 0;                          // q = floor(wl * 2^s / 5^k)
    if (k <= 27) {
        const uint64_t d = pow5(k);     // 5 <= d < 2^63: a remainder doubled fits the word
        q = wl / d;
        uint64_t r = wl % d;
        while ((q >> 63) == 0) {
            q <<= 1;
            r <<= 1;
            if (r >= d) {
                r -= d;
                q |= 1ull;
            }
            ++s;
        }
        sticky = r != 0;
    } else {
        const int a = k - 27 < 27 ? k - 27 : 27;
        U192 d = {pow5(27), 0ull, 0ull};
        d = mul_word(mul_word(d, pow5(a)), pow5(k - 27 - a));       // 2^65 < d < 2^149: wl < d, and a remainder doubled fits
        uint64_t r0 = wl, r1 = 0, r2 = 0;
        q = 0;
        while ((q >> 63) == 0) {
            q <<= 1;
            r2 = (r2 << 1) | (r1 >> 63);
            r1 = (r1 << 1) | (r0 >> 63);
            r0 <<= 1;
            const uint64_t t0 = r0 - d.l0, b0 = r0 < d.l0 ? 1ull : 0ull;
            const uint64_t t1 = r1 - d.l1 - b0, b1 = (r1 < d.l1 || (r1 == d.l1 && b0 != 0)) ? 1ull : 0ull;
            const uint64_t t2 = r2 - d.l2 - b1;
            const bool below = r2 < d.l2 || (r2 == d.l2 && b1 != 0);
            if (!below) {
                r0 = t0, r1 = t1, r2 = t2;
                q |= 1ull;
            }
            ++s;
        }
        sticky = (r0 | r1 | r2) != 0;
    }
    return round_pack(q, sticky, 63 - s - lzw - k);
}

// the bytes [lo, hi) of one match of the number pattern -> its float64 value; false outside the exact domain
DSVG_HD bool decimal_exact(const uint8_t* t, long long lo, long long hi, double& out) {
    long long i = lo;
    bool neg = false;
    if (t[i] == '+' || t[i] == '-') {
        neg = t[i] == '-';
        ++i;
    }
    uint64_t w = 0;
    int nd = 0;                         // digits of w
    long long pending = 0, fraction = 0;        // zeros behind w's last digit; digits behind the dot
    bool frac = false;
    for (; i < hi; ++i) {
        const int b = t[i];
        if (b == 'e' || b == 'E') break;
        if (b == '.') {
            frac = true;
            continue;
        }
        if (frac) ++fraction;
        const int d = b - '0';
        if (d == 0) {
            if (nd > 0) ++pending;      // part of w only when another digit follows
            continue;
        }
        if (pending + 1 > (long long)(DSVG_SVG_EXACT_DIGITS - nd)) return false;
        for (int z = 0; z <= (int)pending; ++z) w *= 10ull;
        w += (uint64_t)d;
        nd += (int)pending + 1;
        pending = 0;
    }
    int ex = 0;
    bool eneg = false;
    if (i < hi) {
        ++i;
        if (i < hi && (t[i] == '+' || t[i] == '-')) {
            eneg = t[i] == '-';
            ++i;
        }
        for (; i < hi; ++i) ex = ex < 10000 ? ex * 10 + (t[i] - '0') : 100000;
    }
    uint64_t bits = 0;
    if (w != 0) {
        const long long e10 = (long long)(eneg ? -ex : ex) - fraction + pending;
        if (e10 < DSVG_SVG_EXACT_E10_MIN || e10 > DSVG_SVG_EXACT_E10_MAX) return false;
        bits = convert(w, (int)e10);
    }
    if (neg) bits |= 1ull << 63;
    __builtin_memcpy(&out, &bits, sizeof(double));
    return true;
}

}  // namespace dsvg_exact
#endif
