// sph_text.hpp -- float32 and int32 as the decimal text of the frame exports, one routine for the device passes
// (sph_text_passes.hpp), the host entry sph_text_format_f32_host and the exhaustive check (tools/check_text_digits.cpp).
// Integer arithmetic only: no floating point, no double, no libm, so the strict build, the fast build and the host give the same bytes.
//   text_decode   bits -> sign, class, the shortest decimal digits that round-trip (at most 9, the closest to the value where several
//                 are shortest, ties to even), decimal exponent: the digits of std::to_chars(..., chars_format::scientific)
//   text_f32      the characters sphexp::format_f32 (sph_export.hpp) makes of them; text_f32_len: their number alone
//   text_index    a 1-based index 1..2^31 in decimal
// The digit method is Ryu's (Adams, PLDI 2018) for binary32: the three values 4 m2 - 1 (- 1 at a binade's lower edge), 4 m2, 4 m2 + 2
// scaled by 2^e2 / 10^q with one 64-bit factor from sph_text_table.hpp (generated from exact integers by sph_project_amd/text_table.py),
// then digits are dropped while the interval still holds a shorter number.
#pragma once
#include <cstdint>
#include "sph_text_table.hpp"

#if defined(__HIPCC__)
#define TEXT_HD __host__ __device__ static inline
#else
#define TEXT_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define TEXT_TABLE static __device__ const
#else
#define TEXT_TABLE static const
#endif

TEXT_TABLE uint64_t TEXT_POW5_INV[TEXT_N_POW5_INV] = TEXT_POW5_INV_LIST;
TEXT_TABLE uint64_t TEXT_POW5[TEXT_N_POW5] = TEXT_POW5_LIST;

// The longest number: sign, 16 digits before the point (|v| < 1e16 is positional, and only the first 9 are significant), ".0" = 19
// ("-9999999000000000.0").  Every other form is shorter: positional with a fraction has at most 9 digits + "0." + 3 zeros + sign = 15
// (|v| >= 1e-4), scientific sign + d + . + 8 digits + e+XX = 15.
#define TEXT_F32_MAX 19
#define TEXT_INDEX_MAX 10          // 2147483648
#define TEXT_PLY_ROW_MAX (3 * (TEXT_F32_MAX + 1) + 1)              // "x y z \n"
#define TEXT_OBJ_V_ROW_MAX (2 + 3 * (1 + TEXT_F32_MAX) + 1)        // "vn x y z\n"
#define TEXT_OBJ_F_ROW_MAX (1 + 3 * (1 + 2 * TEXT_INDEX_MAX + 2) + 1)   // "f a//a b//b c//c\n"
#define TEXT_ROW_MAX TEXT_OBJ_F_ROW_MAX                            // 71
static_assert(TEXT_ROW_MAX >= TEXT_OBJ_V_ROW_MAX && TEXT_ROW_MAX >= TEXT_PLY_ROW_MAX, "the face row is the longest");

enum { TEXT_FINITE = 0, TEXT_ZERO = 1, TEXT_INF = 2, TEXT_NAN = 3 };
struct TextDec {
    uint32_t digits;   // 1..999999999, no trailing zero unless it is the only digit
    int32_t exp10;     // value = digits x 10^exp10
    int32_t nd;        // decimal digits of `digits`
    int32_t cls;       // TEXT_*
    int32_t neg;
};

TEXT_HD uint32_t text_pow5bits(int32_t e) { return (uint32_t)(((uint32_t)e * 1217359u) >> 19) + 1u; }   // bit length of 5^e, e in 0..3528
TEXT_HD uint32_t text_log10_pow2(int32_t e) { return ((uint32_t)e * 78913u) >> 18; }                  // floor(log10(2^e)), e in 0..1650
TEXT_HD uint32_t text_log10_pow5(int32_t e) { return ((uint32_t)e * 732923u) >> 20; }                 // floor(log10(5^e)), e in 0..2620
// floor(m x factor / 2^shift), shift > 32, the result below 2^32
TEXT_HD uint32_t text_mul_shift(uint32_t m, uint64_t factor, int32_t shift) {
    const uint64_t lo = (uint64_t)m * (uint32_t)factor;
    const uint64_t hi = (uint64_t)m * (uint32_t)(factor >> 32);
    return (uint32_t)(((lo >> 32) + hi) >> (shift - 32));
}
TEXT_HD bool text_multiple_of_pow5(uint32_t v, uint32_t p) {
    uint32_t n = 0;
    for (;;) {
        const uint32_t q = v / 5u;
        if (v - 5u * q != 0u) break;
        v = q;
        ++n;
    }
    return n >= p;
}
TEXT_HD bool text_multiple_of_pow2(uint32_t v, uint32_t p) { return (v & ((1u << p) - 1u)) == 0u; }
TEXT_HD int32_t text_digits_of(uint32_t v) {
    return v >= 100000000u ? 9 : v >= 10000000u ? 8 : v >= 1000000u ? 7 : v >= 100000u ? 6 : v >= 10000u ? 5 : v >= 1000u ? 4 :
           v >= 100u ? 3 : v >= 10u ? 2 : 1;
}

TEXT_HD TextDec text_decode(uint32_t bits) {
    TextDec o;
    o.neg = (int32_t)(bits >> 31);
    o.digits = 0u; o.exp10 = 0; o.nd = 1;
    const uint32_t mant = bits & 0x7FFFFFu, expo = (bits >> 23) & 0xFFu;
    if (expo == 255u) { o.cls = mant ? TEXT_NAN : TEXT_INF; return o; }
    if (expo == 0u && mant == 0u) { o.cls = TEXT_ZERO; return o; }
    o.cls = TEXT_FINITE;
    int32_t e2;
    uint32_t m2;
    if (expo == 0u) { e2 = 1 - 127 - 23 - 2; m2 = mant; }
    else { e2 = (int32_t)expo - 127 - 23 - 2; m2 = (1u << 23) | mant; }
    const bool accept = (m2 & 1u) == 0u;   // round to even: the interval's ends belong to an even mantissa
    const uint32_t mv = 4u * m2, mp = 4u * m2 + 2u;
    const uint32_t mm_shift = (mant != 0u || expo <= 1u) ? 1u : 0u;
    const uint32_t mm = 4u * m2 - 1u - mm_shift;
    uint32_t vr, vp, vm;
    int32_t e10;
    bool vm_tz = false, vr_tz = false;
    uint32_t last = 0u;
    if (e2 >= 0) {
        const uint32_t q = text_log10_pow2(e2);
        e10 = (int32_t)q;
        const int32_t k = TEXT_POW5_INV_BITS + (int32_t)text_pow5bits((int32_t)q) - 1;
        const int32_t i = -e2 + (int32_t)q + k;
        vr = text_mul_shift(mv, TEXT_POW5_INV[q], i);
        vp = text_mul_shift(mp, TEXT_POW5_INV[q], i);
        vm = text_mul_shift(mm, TEXT_POW5_INV[q], i);
        if (q != 0u && (vp - 1u) / 10u <= vm / 10u) {   // one digit will go: its value comes from the next coarser scaling
            const int32_t l = TEXT_POW5_INV_BITS + (int32_t)text_pow5bits((int32_t)q - 1) - 1;
            last = text_mul_shift(mv, TEXT_POW5_INV[q - 1u], -e2 + (int32_t)q - 1 + l) % 10u;
        }
        if (q <= 9u) {   // only then can 5^q divide a 26-bit value
            if (mv % 5u == 0u) vr_tz = text_multiple_of_pow5(mv, q);
            else if (accept) vm_tz = text_multiple_of_pow5(mm, q);
            else vp -= text_multiple_of_pow5(mp, q) ? 1u : 0u;
        }
    } else {
        const uint32_t q = text_log10_pow5(-e2);
        e10 = (int32_t)q + e2;
        const int32_t i = -e2 - (int32_t)q;
        const int32_t k = (int32_t)text_pow5bits(i) - TEXT_POW5_BITS;
        int32_t j = (int32_t)q - k;
        vr = text_mul_shift(mv, TEXT_POW5[i], j);
        vp = text_mul_shift(mp, TEXT_POW5[i], j);
        vm = text_mul_shift(mm, TEXT_POW5[i], j);
        if (q != 0u && (vp - 1u) / 10u <= vm / 10u) {
            j = (int32_t)q - 1 - ((int32_t)text_pow5bits(i + 1) - TEXT_POW5_BITS);
            last = text_mul_shift(mv, TEXT_POW5[i + 1], j) % 10u;
        }
        if (q <= 1u) {
            vr_tz = true;   // mv = 4 m2 has at least two factors of 2
            if (accept) vm_tz = mm_shift == 1u;
            else --vp;
        } else if (q < 31u) {
            vr_tz = text_multiple_of_pow2(mv, q - 1u);
        }
    }
    int32_t removed = 0;
    uint32_t out;
    if (vm_tz || vr_tz) {   // rare: exact ties and interval ends need the removed digits' history
        while (vp / 10u > vm / 10u) {
            vm_tz &= vm % 10u == 0u;
            vr_tz &= last == 0u;
            last = vr % 10u;
            vr /= 10u; vp /= 10u; vm /= 10u;
            ++removed;
        }
        if (vm_tz) {
            while (vm % 10u == 0u) {
                vr_tz &= last == 0u;
                last = vr % 10u;
                vr /= 10u; vp /= 10u; vm /= 10u;
                ++removed;
            }
        }
        if (vr_tz && last == 5u && vr % 2u == 0u) last = 4u;   // exactly half: to even
        out = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5u) ? 1u : 0u);
    } else {
        while (vp / 10u > vm / 10u) {
            last = vr % 10u;
            vr /= 10u; vp /= 10u; vm /= 10u;
            ++removed;
        }
        out = vr + ((vr == vm || last >= 5u) ? 1u : 0u);
    }
    o.digits = out;
    o.exp10 = e10 + removed;
    o.nd = text_digits_of(out);
    return o;
}

// positional ("0.001", "123456790.0") for 1e-4 <= |v| < 1e16, decided on the value itself as format_f32 does (the float nearest 1e-4
// lies below it and is written "1e-04")
TEXT_HD bool text_positional(uint32_t bits) {
    const uint32_t a = bits & 0x7FFFFFFFu;
    return a >= TEXT_POS_FIRST_BITS && a < TEXT_POS_END_BITS;
}

TEXT_HD int32_t text_f32_len(uint32_t bits) {
    const TextDec d = text_decode(bits);
    if (d.cls == TEXT_NAN) return 3;
    if (d.cls != TEXT_FINITE) return 3 + d.neg;
    const int32_t e = d.exp10 + d.nd - 1;   // the scientific exponent
    if (!text_positional(bits)) return d.neg + d.nd + (d.nd > 1 ? 1 : 0) + 4;
    if (e >= 0) return d.neg + (e + 1) + 1 + (d.nd > e + 1 ? d.nd - e - 1 : 1);
    return d.neg + 2 + (-e - 1) + d.nd;
}

// the characters of one float at p (at most TEXT_F32_MAX, no terminator); returns their number
template <class P> TEXT_HD int32_t text_f32(uint32_t bits, P p) {
    const TextDec d = text_decode(bits);
    int32_t n = 0;
    if (d.cls == TEXT_NAN) { p[0] = 'n'; p[1] = 'a'; p[2] = 'n'; return 3; }
    if (d.neg) p[n++] = '-';
    if (d.cls == TEXT_INF) { p[n] = 'i'; p[n + 1] = 'n'; p[n + 2] = 'f'; return n + 3; }
    if (d.cls == TEXT_ZERO) { p[n] = '0'; p[n + 1] = '.'; p[n + 2] = '0'; return n + 3; }
    const int32_t e = d.exp10 + d.nd - 1;
    const bool pos = text_positional(bits);
    // digit k of nd goes to p[first + k], one further behind a point after digit `point`
    int32_t first = n, point, total;
    if (!pos) {
        point = 0;
        total = n + d.nd + (d.nd > 1 ? 1 : 0);
        if (d.nd > 1) p[n + 1] = '.';
        p[total] = 'e';
        p[total + 1] = e < 0 ? '-' : '+';
        const int32_t a = e < 0 ? -e : e;   // <= 45
        p[total + 2] = (char)('0' + a / 10);
        p[total + 3] = (char)('0' + a % 10);
        total += 4;
    } else if (e >= 0) {
        point = e;
        for (int32_t k = d.nd; k <= e; ++k) p[n + k] = '0';
        p[n + e + 1] = '.';
        if (d.nd > e + 1) total = n + d.nd + 1;
        else { p[n + e + 2] = '0'; total = n + e + 3; }
    } else {
        p[n] = '0'; p[n + 1] = '.';
        for (int32_t k = 0; k < -e - 1; ++k) p[n + 2 + k] = '0';
        first = n + 2 + (-e - 1);
        point = d.nd;   // no point among the digits
        total = first + d.nd;
    }
    uint32_t v = d.digits;
    for (int32_t k = d.nd - 1; k >= 0; --k) {
        const uint32_t q = v / 10u;
        p[first + k + (k > point ? 1 : 0)] = (char)('0' + (v - 10u * q));
        v = q;
    }
    return total;
}

// a 0-based index 0 <= i < 2^31 as the 1-based decimal number
TEXT_HD int32_t text_index_len(int32_t i) {
    const uint32_t v = (uint32_t)i + 1u;
    return v >= 1000000000u ? 10 : text_digits_of(v);
}
template <class P> TEXT_HD int32_t text_index(int32_t i, P p) {
    uint32_t v = (uint32_t)i + 1u;
    const int32_t n = text_index_len(i);
    for (int32_t k = n - 1; k >= 0; --k) { const uint32_t q = v / 10u; p[k] = (char)('0' + (v - 10u * q)); v = q; }
    return n;
}
