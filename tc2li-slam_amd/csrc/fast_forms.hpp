// The per-pixel arithmetic of k_fast_cells (orb_kernels.hip), two values per instruction in packed 16-bit form.  The kernel and the host
// entry tc2li_host_fast_forms (tests/test_fast_forms.py) run this same source: only the helpers of the first block differ -- on the device
// they are the 2 x 16-bit vector type and the elementwise builtins (v_pk_min_i16, v_pk_max_i16, v_pk_sub_i16, v_pk_sub_u16 clamp,
// v_pk_mad_i16, v_pk_lshrrev_b16; a half swap is an operand modifier of those), on the host plain C++ on the two halves.
// Everything below needs 0 <= th <= 255 (tc2li_orb_create refuses other thresholds): with pixel values 0 .. 255 every sum and difference
// formed here lies in [-255, 510] and fits a signed 16-bit half.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TC2LI_FF __host__ __device__ __forceinline__
#else
#define TC2LI_FF inline
#endif

namespace tc2li {
namespace fastforms {

#if defined(__HIP_DEVICE_COMPILE__)
typedef short pk16 __attribute__((ext_vector_type(2)));
typedef unsigned short pk16u __attribute__((ext_vector_type(2)));
TC2LI_FF pk16 pk_make(int lo, int hi) { return pk16{(short)lo, (short)hi}; }
TC2LI_FF pk16 pk_from_bits(uint32_t b) { return __builtin_bit_cast(pk16, b); }
TC2LI_FF uint32_t pk_bits(pk16 a) { return __builtin_bit_cast(uint32_t, a); }
TC2LI_FF int pk_lo(pk16 a) { return a.x; }
TC2LI_FF int pk_hi(pk16 a) { return a.y; }
TC2LI_FF pk16 pk_min(pk16 a, pk16 b) { return __builtin_elementwise_min(a, b); }
TC2LI_FF pk16 pk_max(pk16 a, pk16 b) { return __builtin_elementwise_max(a, b); }
TC2LI_FF pk16 pk_sub(pk16 a, pk16 b) { return a - b; }
TC2LI_FF pk16 pk_mad(pk16 a, pk16 b, pk16 c) { return a * b + c; }
TC2LI_FF pk16 pk_swap(pk16 a) { return __builtin_shufflevector(a, a, 1, 0); }
// unsigned a - b, clamped at 0
TC2LI_FF pk16 pk_sub_sat_u(pk16 a, pk16 b) {
    return __builtin_bit_cast(pk16, __builtin_elementwise_sub_sat(__builtin_bit_cast(pk16u, a), __builtin_bit_cast(pk16u, b)));
}
// the sign of each half as bit 0 / bit 16
TC2LI_FF uint32_t pk_sign_bits(pk16 a) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pk16u, a) >> (unsigned short)15); }
// bytes (b0, b2, b0, b2) of a
TC2LI_FF uint32_t bytes_0202(uint32_t a) { return __builtin_amdgcn_perm(a, a, 0x02000200u); }
// bytes 1 and 3 of w, widened to the two halves
TC2LI_FF uint32_t odd_bytes(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c030c01u); }
#else
struct pk16 { int16_t x, y; };
TC2LI_FF pk16 pk_make(int lo, int hi) { return pk16{(int16_t)lo, (int16_t)hi}; }
TC2LI_FF pk16 pk_from_bits(uint32_t b) { return pk16{(int16_t)(uint16_t)(b & 0xffffu), (int16_t)(uint16_t)(b >> 16)}; }
TC2LI_FF uint32_t pk_bits(pk16 a) { return (uint32_t)(uint16_t)a.x | ((uint32_t)(uint16_t)a.y << 16); }
TC2LI_FF int pk_lo(pk16 a) { return a.x; }
TC2LI_FF int pk_hi(pk16 a) { return a.y; }
TC2LI_FF pk16 pk_min(pk16 a, pk16 b) { return pk16{a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y}; }
TC2LI_FF pk16 pk_max(pk16 a, pk16 b) { return pk16{a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y}; }
TC2LI_FF pk16 pk_sub(pk16 a, pk16 b) { return pk_make((uint16_t)a.x - (uint16_t)b.x, (uint16_t)a.y - (uint16_t)b.y); }
TC2LI_FF pk16 pk_mad(pk16 a, pk16 b, pk16 c) { return pk_make(a.x * b.x + c.x, a.y * b.y + c.y); }
TC2LI_FF pk16 pk_swap(pk16 a) { return pk16{a.y, a.x}; }
TC2LI_FF pk16 pk_sub_sat_u(pk16 a, pk16 b) {
    const int x = (int)(uint16_t)a.x - (int)(uint16_t)b.x, y = (int)(uint16_t)a.y - (int)(uint16_t)b.y;
    return pk_make(x > 0 ? x : 0, y > 0 ? y : 0);
}
TC2LI_FF uint32_t pk_sign_bits(pk16 a) { return (a.x < 0 ? 1u : 0u) | (a.y < 0 ? 0x10000u : 0u); }
TC2LI_FF uint32_t bytes_0202(uint32_t a) { const uint32_t m = (a & 0xffu) | ((a >> 8) & 0xff00u); return m | (m << 16); }
TC2LI_FF uint32_t odd_bytes(uint32_t w) { return (w >> 8) & 0x00ff00ffu; }
#endif

TC2LI_FF pk16 pk_splat(int a) { return pk_make(a, a); }

// ---- Pass 0, the compass pre-test of four horizontally adjacent pixels.  Byte k of V is the centre of pixel k, byte k of P0 / P4 / P8 /
// P12 its circle pixel 0 (three below) / 4 (three to the right) / 8 / 12.  Nine contiguous circle pixels always hold pixel 0 or 8 and
// pixel 4 or 12, so a brighter arc needs most = min(max(p0, p8), max(p4, p12)) > v + th and a darker one least = max(min, min) < v - th.
// As saturating differences: most -. (v + th) != 0, or (v -. th) -. least != 0 -- the clamp of v - th at 0 is harmless, least >= 0.
// Pixels 0 and 2 go through one packed pair, 1 and 3 through the other.
struct Pre4 { uint32_t even, odd; };  // a non-zero half <=> that pixel passes: even = (pixel 0, pixel 2), odd = (pixel 1, pixel 3)
TC2LI_FF uint32_t pretest_pair(pk16 v, pk16 p0, pk16 p4, pk16 p8, pk16 p12, pk16 th2) {
    const pk16 most = pk_min(pk_max(p0, p8), pk_max(p4, p12)), least = pk_max(pk_min(p0, p8), pk_min(p4, p12));
    const pk16 hi = pk_from_bits(pk_bits(v) + pk_bits(th2));  // v + th <= 510: no carry between the halves
    return pk_bits(pk_sub_sat_u(most, hi)) | pk_bits(pk_sub_sat_u(pk_sub_sat_u(v, th2), least));
}
TC2LI_FF Pre4 pretest4(uint32_t V, uint32_t P0, uint32_t P4, uint32_t P8, uint32_t P12, int th) {
    const pk16 th2 = pk_splat(th);
    const uint32_t m = 0x00ff00ffu;
    Pre4 r;
    r.even = pretest_pair(pk_from_bits(V & m), pk_from_bits(P0 & m), pk_from_bits(P4 & m), pk_from_bits(P8 & m), pk_from_bits(P12 & m), th2);
    r.odd = pretest_pair(pk_from_bits(odd_bytes(V)), pk_from_bits(odd_bytes(P0)), pk_from_bits(odd_bytes(P4)), pk_from_bits(odd_bytes(P8)),
                         pk_from_bits(odd_bytes(P12)), th2);
    return r;
}
TC2LI_FF bool pretest_flag(const Pre4& r, int k) {
    const uint32_t w = (k & 1) ? r.odd : r.even;
    return ((k & 2) ? (w >> 16) : (w & 0xffffu)) != 0;
}

// ---- Pass 1, the segment test.  The circle is held as eight pairs: c[k] = (p[k], p[k + 8]).
// (v + th) - p is negative <=> p is brighter, p - (v - th) negative <=> darker: the sign bits of the packed differences are the flags, no
// compare and no select.  They are shifted into a word (bit k and bit 16 + k: pixels k and k + 8) and spread to the mask repeated twice,
// m16 | m16 << 16 with bit j of m16 = pixel j, which is what the "nine contiguous" test starts from.
TC2LI_FF void segment_words(const pk16 (&c)[8], int v, int th, uint32_t& bright, uint32_t& dark) {
    const pk16 hi = pk_splat(v + th), lo = pk_splat(v - th);
    uint32_t ab = 0, ad = 0;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        ab = (ab << 1) | pk_sign_bits(pk_sub(hi, c[k]));
        ad = (ad << 1) | pk_sign_bits(pk_sub(c[k], lo));
    }
    bright = bytes_0202(ab);
    dark = bytes_0202(ad);
}
// x = m16 | m16 << 16: are nine circularly contiguous bits of m16 set?
TC2LI_FF bool has_arc9_word(uint32_t x) {
    uint32_t r = x & (x >> 1);
    r &= r >> 2;
    r &= r >> 4;
    r &= x >> 8;
    return (r & 0xffffu) != 0;
}
// bit 0: a darker arc, bit 1: a brighter arc.  Never both: an arc has nine of the sixteen pixels, and no pixel is brighter and darker.
TC2LI_FF uint32_t polarity(const pk16 (&c)[8], int v, int th) {
    uint32_t xb, xd;
    segment_words(c, v, th, xb, xd);
    return (has_arc9_word(xd) ? 1u : 0u) | (has_arc9_word(xb) ? 2u : 0u);
}

// ---- Pass 2, the score: the largest over the 16 arcs of nine contiguous circle pixels of min(v - p) (dark) or min(p - v).
// d[k] = (d_k, d_{k+8}) is formed by one multiply-add per pair (+-1 * p -+ v), and "element k + s" of a 16-element ring is register k + s,
// past register 7 the half-swapped registers 0 ..: the min tree of spans 2, 4, 8 runs once on the pairs, the arc that starts at k is
// pixel k and the span of eight behind it.
TC2LI_FF int arc_score(const pk16 (&c)[8], int v, bool dark) {
    const pk16 sgn = pk_splat(dark ? -1 : 1), off = pk_splat(dark ? v : -v);
    pk16 d[8], m2[8], m4[8], m8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = pk_mad(c[k], sgn, off);
#pragma unroll
    for (int k = 0; k < 8; ++k) m2[k] = pk_min(d[k], k + 1 < 8 ? d[k + 1] : pk_swap(d[k + 1 - 8]));
#pragma unroll
    for (int k = 0; k < 8; ++k) m4[k] = pk_min(m2[k], k + 2 < 8 ? m2[k + 2] : pk_swap(m2[k + 2 - 8]));
#pragma unroll
    for (int k = 0; k < 8; ++k) m8[k] = pk_min(m4[k], k + 4 < 8 ? m4[k + 4] : pk_swap(m4[k + 4 - 8]));
    pk16 best = pk_min(d[7], pk_swap(m8[0]));
#pragma unroll
    for (int k = 0; k < 7; ++k) best = pk_max(best, pk_min(d[k], m8[k + 1]));
    const int a = pk_lo(best), b = pk_hi(best);
    return a > b ? a : b;
}

}  // namespace fastforms
}  // namespace tc2li
