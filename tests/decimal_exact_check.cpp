// deepsvg_amd/csrc/decimal_exact.h on its own, on the host: seeded and directed decimal texts through dsvg_exact::decimal_exact
// against strtod, by bits.  A program of its own (tests/test_svgio_exact_host.py builds it with the host compiler and
// -fsanitize=undefined,address and runs it); any mismatch gives a non-zero exit.
//   decimal_exact_check [cases]      default 1,000,000 seeded cases
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../deepsvg_amd/csrc/decimal_exact.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                 // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

static long long failures = 0, checked = 0;

// 1: a value, 0: outside the domain
static int run(const std::string& text, double& v) {
    return dsvg_exact::decimal_exact((const uint8_t*)text.data(), 0, (long long)text.size(), v) ? 1 : 0;
}
static void expect_value(const std::string& text) {
    double got = 0.0;
    const double want = strtod(text.c_str(), nullptr);
    ++checked;
    uint64_t gb, wb;
    if (!run(text, got)) {
        if (++failures <= 20) printf("refused: %s\n", text.c_str());
        return;
    }
    memcpy(&gb, &got, 8);
    memcpy(&wb, &want, 8);
    if (gb != wb && ++failures <= 20) printf("mismatch: %s -> %016" PRIx64 ", strtod %016" PRIx64 "\n", text.c_str(), gb, wb);
}
static void expect_refused(const std::string& text) {
    double got = 0.0;
    ++checked;
    if (run(text, got) && ++failures <= 20) printf("accepted: %s\n", text.c_str());
}

// the digits of w (no leading, no trailing zero unless asked for) with 10^e10, spelled one of several ways
static std::string spell(const std::string& digits, int e10) {
    std::string body;
    const int style = below(4);
    const int nd = (int)digits.size();
    if (style == 0 && e10 <= 0 && -e10 <= 40) {              // a plain fraction
        if (-e10 < nd) body = digits.substr(0, nd + e10) + "." + digits.substr(nd + e10);
        else body = (below(2) ? "0." : ".") + std::string(-e10 - nd, '0') + digits;
        if (body.back() == '.') body += "0";
    } else if (style == 1 && e10 >= 0 && e10 <= 30) {        // a plain integer
        body = digits + std::string(e10, '0');
        if (below(2)) body += "." + std::string(below(3) + 1, '0');
    } else {                                                 // exponent form, the dot anywhere
        const int cut = below(nd + 1);
        body = digits.substr(0, cut);
        if (cut < nd || below(2)) body += "." + digits.substr(cut);
        if (body.back() == '.') body += "0";
        int ex = e10 + (nd - cut);
        if (below(3) == 0) {                                 // trailing zeros of the fraction
            const int z = below(4) + 1;
            if (body.find('.') == std::string::npos) body += ".";
            body += std::string(z, '0');
        }
        char buf[32];
        snprintf(buf, sizeof buf, below(2) ? "e%+d" : "E%d", ex);
        body += buf;
    }
    if (below(3) == 0) body = std::string(below(4) + 1, '0') + body;       // leading zeros
    const int sign = below(3);
    return (sign == 0 ? "" : sign == 1 ? "-" : "+") + body;
}

static std::string random_digits(int nd) {
    std::string d(nd, '0');
    for (int i = 0; i < nd; ++i) d[i] = (char)('0' + below(10));
    d[0] = (char)('1' + below(9));
    d[nd - 1] = (char)('1' + below(9));
    return d;
}

int main(int argc, char** argv) {
    const long long cases = argc > 1 ? atoll(argv[1]) : 1000000;
    for (long long c = 0; c < cases; ++c) {
        const int nd = 1 + below(DSVG_SVG_EXACT_DIGITS);
        // every e10 of the domain, and more often the ones coordinates have
        const int e10 = below(3) ? DSVG_SVG_EXACT_E10_MIN + below(DSVG_SVG_EXACT_E10_MAX - DSVG_SVG_EXACT_E10_MIN + 1) : -below(24);
        expect_value(spell(random_digits(nd), e10));
    }
    char buf[64];
    // exact midpoints between neighbouring doubles, (2m + 1) << s below 10^19, and their neighbours
    for (int c = 0; c < 200000; ++c) {
        const uint64_t m = (1ull << 52) | (rnd() >> 12);
        const uint64_t mid = ((2 * m + 1) << below(10)) + (uint64_t)(below(3) - 1);
        if (mid >= 10000000000000000000ull) continue;
        snprintf(buf, sizeof buf, "%" PRIu64, mid);
        expect_value(buf);
        std::string withexp = std::string(buf) + "e" + std::to_string(below(20));       // halfway digits times a power of ten
        expect_value(withexp);
    }
    // float32 values printed through float64 with 17 digits, as the reference's save_svg prints them
    for (int c = 0; c < 200000; ++c) {
        uint32_t bits = (uint32_t)rnd();
        float f;
        memcpy(&f, &bits, 4);
        const double d = (double)f;
        if (!(d == d) || d - d != 0.0 || d == 0.0 || (d < 0 ? -d : d) < 1e-37) continue;
        snprintf(buf, sizeof buf, "%.17g", d);
        expect_value(buf);
        snprintf(buf, sizeof buf, "%.16e", d);
        expect_value(buf);
    }
    const char* directed[] = {"0.12345678901234567", "9007199254740991", "9007199254740992", "9007199254740993", "9007199254740995",
        "123456789012345678", "1234567890123456789", "9999999999999999999", "12345678901234567890", "1e23", "1e22", "8.5e22", "1.5e-30",
        "-5.9604644775390625e-08", "1e38", "9999999999999999999e38", "1e-64", "1e-45", "9999999999999999999e-64", "3.4028234663852886e+38",
        "1.401298464324817e-45", "0.000000000000000000000000000000123", "0.0000000000000000000000000000001234567890123456789",
        "70000000000000000000000000", "1234567890123456789000000000000000000000000000", "0e999", "-0.000e-999", "0", "-0", "+0.0",
        "000000000000000000000000000000000000000017", "1.0000000000000000000000000000000000", "4.35", "0.1", "2.2250738585072014e-30",
        "9007199254740993e3", "18014398509481985", "18014398509481987", "4503599627370497.5", "1e-28", "1e-27", "123e-28", "5e27",
        "5e28", "1e1", "100000000000000000000e-20", "1e000000000000000000000012", "7e-0000000000000000000003"};
    for (const char* s : directed) expect_value(s);
    const char* refused[] = {"12345678901234567891", "1.2345678901234567891", "1e39", "1e-65", "10e38", "0.1e-64", "1e999", "1e-999",
        "12345678901234567890123", "1e100000000000000000000", "123456789012345678901e-30"};
    for (const char* s : refused) expect_refused(s);
    printf("decimal_exact_check: %lld texts, %lld failures\n", checked, failures);
    return failures == 0 ? 0 : 1;
}
