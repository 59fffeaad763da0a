// recc_slice.hip.h -- slicer arithmetic shared by the streaming kernel of the IQ seam (recc_front.hip.h), the filter bank's slicer
// (recc_chz_slicer.hip.h) and the host entry amps_recc_debug_exact_slice: the packed arctangent discriminator of specs A / C and the
// bit-sliced winding-number words of spec D (include/amps_recc_numerics.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "amps_recc_numerics.h"

namespace amps {

typedef float f2 __attribute__((ext_vector_type(2)));

// The discriminator of include/amps_recc_numerics.h for the two samples a lane holds (A = s.xy with
// predecessor p, B = s.zw with predecessor A), written on 2-vectors so that hipcc emits v_pk_mul /
// v_pk_fma / v_pk_add: measured on MI355X a packed fp32 op issues in ~4.8 cycles per wave against
// ~4.3 for a scalar one (scripts/ubench_pk.hip), i.e. 1.8x the arithmetic per issue slot, and this
// kernel is VALU-issue bound.  ~19 instructions per sample instead of ~30.
// re, im = the real and imaginary parts of TWO conj-products (planar: element 0 in .x, element 1 in .y); every operation
// after them is packed over the two
__device__ __forceinline__ f2 fm_phase_planar(f2 re, f2 im)
{
    const float axa = __builtin_fabsf(re.x), aya = __builtin_fabsf(im.x);
    const float axb = __builtin_fabsf(re.y), ayb = __builtin_fabsf(im.y);
    const f2 mx = { __builtin_fmaxf(__builtin_fmaxf(axa, aya), AMPS_MX_FLOOR), __builtin_fmaxf(__builtin_fmaxf(axb, ayb), AMPS_MX_FLOOR) };
    const f2 mn = { __builtin_fminf(axa, aya), __builtin_fminf(axb, ayb) };
    f2 r = { __uint_as_float(AMPS_RCP_MAGIC - __float_as_uint(mx.x)), __uint_as_float(AMPS_RCP_MAGIC - __float_as_uint(mx.y)) };
    const f2 one = { 1.0f, 1.0f };
    f2 e;
    e = __builtin_elementwise_fma(-mx, r, one); r = __builtin_elementwise_fma(r, e, r);
    e = __builtin_elementwise_fma(-mx, r, one); r = __builtin_elementwise_fma(r, e, r);
    e = __builtin_elementwise_fma(-mx, r, one); r = __builtin_elementwise_fma(r, e, r);
    const f2 q = mn * r;
    const f2 z = q * q;
    f2 p = { AMPS_ATAN_C5, AMPS_ATAN_C5 };
    p = __builtin_elementwise_fma(p, z, (f2){ AMPS_ATAN_C4, AMPS_ATAN_C4 });
    p = __builtin_elementwise_fma(p, z, (f2){ AMPS_ATAN_C3, AMPS_ATAN_C3 });
    p = __builtin_elementwise_fma(p, z, (f2){ AMPS_ATAN_C2, AMPS_ATAN_C2 });
    p = __builtin_elementwise_fma(p, z, (f2){ AMPS_ATAN_C1, AMPS_ATAN_C1 });
    p = __builtin_elementwise_fma(p, z, (f2){ AMPS_ATAN_C0, AMPS_ATAN_C0 });
    f2 a = p * q;
    const f2 a_swapped = (f2){ AMPS_PI_2_F, AMPS_PI_2_F } - a;
    a.x = aya > axa ? a_swapped.x : a.x;
    a.y = ayb > axb ? a_swapped.y : a.y;
    const f2 a_reflect = (f2){ AMPS_PI_F, AMPS_PI_F } - a;
    a.x = re.x < 0.0f ? a_reflect.x : a.x;
    a.y = re.y < 0.0f ? a_reflect.y : a.y;
    return (f2){ __builtin_copysignf(a.x, im.x), __builtin_copysignf(a.y, im.y) };
}
// N independent planar evaluations written in lock step (same operations, same order per value, so every result is
// bit-identical to a separate fm_phase_planar call): the Newton and Horner chains are serial and every packed operation that
// consumes the previous one costs a wait state, so one chain at a time runs at a third of the issue rate (the compiler keeps
// the source order: it pads the single chain with s_nop instead of interleaving)
// an empty asm that "uses and redefines" the N values of one row: every chain has reached this row before any goes on
template <int N> __device__ __forceinline__ void fm_row_join(f2 (&v)[N])
{
    static_assert(N == 4 || N == 2, "rows of two or four");
    if constexpr (N == 4) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
    else asm volatile("" : "+v"(v[0]), "+v"(v[1]));
}
template <int N>
__device__ __forceinline__ void fm_phase_planar_n(const f2 (&re)[N], const f2 (&im)[N], f2 (&out)[N])
{
    f2 mx[N], mn[N], r[N], e[N], q[N], z[N], p[N], a[N];
    bool sw[N][2];
#pragma unroll
    for (int i = 0; i < N; i++) {
        const float axa = __builtin_fabsf(re[i].x), aya = __builtin_fabsf(im[i].x), axb = __builtin_fabsf(re[i].y), ayb = __builtin_fabsf(im[i].y);
        mx[i] = (f2){ __builtin_fmaxf(__builtin_fmaxf(axa, aya), AMPS_MX_FLOOR), __builtin_fmaxf(__builtin_fmaxf(axb, ayb), AMPS_MX_FLOOR) };
        mn[i] = (f2){ __builtin_fminf(axa, aya), __builtin_fminf(axb, ayb) };
        sw[i][0] = aya > axa; sw[i][1] = ayb > axb;
        r[i] = (f2){ __uint_as_float(AMPS_RCP_MAGIC - __float_as_uint(mx[i].x)), __uint_as_float(AMPS_RCP_MAGIC - __float_as_uint(mx[i].y)) };
    }
    const f2 one = { 1.0f, 1.0f };
#pragma unroll
    for (int it = 0; it < 3; it++) {
#pragma unroll
        for (int i = 0; i < N; i++) e[i] = __builtin_elementwise_fma(-mx[i], r[i], one);
    fm_row_join(e);
#pragma unroll
        for (int i = 0; i < N; i++) r[i] = __builtin_elementwise_fma(r[i], e[i], r[i]);
    fm_row_join(r);
    }
#pragma unroll
    for (int i = 0; i < N; i++) q[i] = mn[i] * r[i];
    fm_row_join(q);
#pragma unroll
    for (int i = 0; i < N; i++) z[i] = q[i] * q[i];
    fm_row_join(z);
#pragma unroll
    for (int i = 0; i < N; i++) p[i] = __builtin_elementwise_fma((f2){ AMPS_ATAN_C5, AMPS_ATAN_C5 }, z[i], (f2){ AMPS_ATAN_C4, AMPS_ATAN_C4 });
    fm_row_join(p);
#pragma unroll
    for (int i = 0; i < N; i++) p[i] = __builtin_elementwise_fma(p[i], z[i], (f2){ AMPS_ATAN_C3, AMPS_ATAN_C3 });
    fm_row_join(p);
#pragma unroll
    for (int i = 0; i < N; i++) p[i] = __builtin_elementwise_fma(p[i], z[i], (f2){ AMPS_ATAN_C2, AMPS_ATAN_C2 });
    fm_row_join(p);
#pragma unroll
    for (int i = 0; i < N; i++) p[i] = __builtin_elementwise_fma(p[i], z[i], (f2){ AMPS_ATAN_C1, AMPS_ATAN_C1 });
    fm_row_join(p);
#pragma unroll
    for (int i = 0; i < N; i++) p[i] = __builtin_elementwise_fma(p[i], z[i], (f2){ AMPS_ATAN_C0, AMPS_ATAN_C0 });
    fm_row_join(p);
#pragma unroll
    for (int i = 0; i < N; i++) a[i] = p[i] * q[i];
    fm_row_join(a);
#pragma unroll
    for (int i = 0; i < N; i++) {
        const f2 a_swapped = (f2){ AMPS_PI_2_F, AMPS_PI_2_F } - a[i];
        a[i].x = sw[i][0] ? a_swapped.x : a[i].x;
        a[i].y = sw[i][1] ? a_swapped.y : a[i].y;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        const f2 a_reflect = (f2){ AMPS_PI_F, AMPS_PI_F } - a[i];
        a[i].x = re[i].x < 0.0f ? a_reflect.x : a[i].x;
        a[i].y = re[i].y < 0.0f ? a_reflect.y : a[i].y;
        out[i] = (f2){ __builtin_copysignf(a[i].x, im[i].x), __builtin_copysignf(a[i].y, im[i].y) };
    }
}
// ta, tb = the two conj-products as (re, im) pairs
__device__ __forceinline__ f2 fm_phase_core(f2 ta, f2 tb)
{
    return fm_phase_planar((f2){ ta.x, tb.x }, (f2){ ta.y, tb.y });
}

// Bit-sliced small SIGNED integers for slicer spec D: bit i of plane k = bit k of the two's complement number that belongs to sample
// i of a 32-sample word (oldest sample at bit 0, so "j samples earlier" is a left shift); plane W - 1 is the sign.  One chain of
// signed adds for K = w'' - sum w' instead of two unsigned ones (wraps past +pi and past -pi counted apart, then compared): 63
// word operations per 32 samples at 10 samples per symbol instead of 88.  Plain C: the same functions run on the host for
// tests/test_cpu_exact_slicer.py (amps_recc_debug_exact_slice).
template <int W> struct SBits { uint32_t p[W]; };
__host__ __device__ constexpr int sbits_width(int L) { int w = 1; while ((1 << (w - 1)) <= L) w++; return w; }   // planes that hold -L .. L
template <int W> __host__ __device__ __forceinline__ SBits<W> sb_shl(const SBits<W> &a, int j)
{
    SBits<W> r;
#pragma unroll
    for (int k = 0; k < W; k++) r.p[k] = a.p[k] << j;
    return r;
}
// a + b in WR planes, both sign-extended (the caller picks WR wide enough for the sum)
template <int WR, int WA, int WB> __host__ __device__ __forceinline__ SBits<WR> sb_add(const SBits<WA> &a, const SBits<WB> &b)
{
    SBits<WR> r;
    uint32_t c = 0u;
#pragma unroll
    for (int k = 0; k < WR; k++) {
        const uint32_t pa = a.p[k < WA ? k : WA - 1], pb = b.p[k < WB ? k : WB - 1];
        const uint32_t x = pa ^ pb;
        r.p[k] = x ^ c;
        c = (pa & pb) | (x & c);
    }
    return r;
}
// sum_{j < L} (t << j) for t in {-1, 0, +1} per sample: the L samples ending at each position, by doubling (1, 2, 4, 8, 16 samples)
// and the binary digits of L
template <int L> __host__ __device__ __forceinline__ SBits<sbits_width(L)> sb_window(const SBits<2> &t)
{
    static_assert(L >= 1 && L <= 16, "window");
    constexpr int WR = sbits_width(L);
    const SBits<2> s1 = t;
    SBits<3> s2{}; SBits<4> s4{}; SBits<5> s8{}; SBits<6> s16{};
    if constexpr (L >= 2) s2 = sb_add<3>(s1, sb_shl(s1, 1));
    if constexpr (L >= 4) s4 = sb_add<4>(s2, sb_shl(s2, 2));
    if constexpr (L >= 8) s8 = sb_add<5>(s4, sb_shl(s4, 4));
    if constexpr (L >= 16) s16 = sb_add<6>(s8, sb_shl(s8, 8));
    SBits<WR> acc{};
    int off = 0;
    if constexpr (L & 16) { acc = sb_add<WR>(acc, sb_shl(s16, off)); off += 16; }
    if constexpr (L & 8) { acc = sb_add<WR>(acc, sb_shl(s8, off)); off += 8; }
    if constexpr (L & 4) { acc = sb_add<WR>(acc, sb_shl(s4, off)); off += 4; }
    if constexpr (L & 2) { acc = sb_add<WR>(acc, sb_shl(s2, off)); off += 2; }
    if constexpr (L & 1) { acc = sb_add<WR>(acc, sb_shl(s1, off)); off += 1; }
    return acc;
}
// slicer spec D (include/amps_recc_numerics.h) on one 32-sample window, oldest sample at bit 0: SX, ST, SC = the signs of Im x,
// Im(x conj(x[n-1])), Im(x conj(x[n-SPS])).  Bits >= SPS of the result are exact (the wraps need one sample of history, their
// window SPS - 1 more, the partner SPS).
template <int SPS> __host__ __device__ __forceinline__ uint32_t exact_slice_word(uint32_t SX, uint32_t ST, uint32_t SC)
{
    const uint32_t sx1 = SX << 1, sxs = SX << SPS;
    const uint32_t wp = ~SX & sx1 & ST, wm = SX & ~sx1 & ~ST;          // w'  = +1 / -1
    const uint32_t up = ~SX & sxs & SC, um = SX & ~sxs & ~SC;          // w'' = +1 / -1
    const SBits<2> t = { { wp | wm, wp } };                            // -w' per sample: -1 where the step wrapped past +pi, +1 past -pi
    const SBits<2> u = { { up | um, um } };                            // +w''
    constexpr int WK = sbits_width(SPS + 1);
    const SBits<WK> K = sb_add<WK>(sb_window<SPS>(t), u);              // K = w'' - sum w'
    uint32_t any = 0u;
#pragma unroll
    for (int k = 0; k < WK; k++) any |= K.p[k];
    return ~K.p[WK - 1] & (any | ~SC);                                 // K > 0, or K == 0 and the partner product not negative
}
// the same for the filter bank's slicer (3 frames per symbol), whose sign words are shift registers with the NEWEST frame at bit 0
// and the previous 32 frames in a second word: delay j = funnel shift.  wp_out / wm_out: the wrap words the next call needs.
__host__ __device__ __forceinline__ uint32_t exact_funnel(uint32_t prev, uint32_t cur, int j) { return (cur >> j) | (prev << (32 - j)); }
__host__ __device__ __forceinline__ uint32_t exact_slice_word3(uint32_t SX, uint32_t ST, uint32_t SC, uint32_t sx_prev, uint32_t wp_prev, uint32_t wm_prev,
                                                                uint32_t &wp_out, uint32_t &wm_out)
{
    const uint32_t sx1 = exact_funnel(sx_prev, SX, 1), sx3 = exact_funnel(sx_prev, SX, 3);
    const uint32_t wp = ~SX & sx1 & ST, wm = SX & ~sx1 & ~ST;          // the phase step crossed the cut: w' = +1 / -1
    const uint32_t up = ~SX & sx3 & SC, um = SX & ~sx3 & ~SC;          // ... of the three-frame partner: w'' = +1 / -1
    const uint32_t wp1 = exact_funnel(wp_prev, wp, 1), wp2 = exact_funnel(wp_prev, wp, 2);
    const uint32_t wm1 = exact_funnel(wm_prev, wm, 1), wm2 = exact_funnel(wm_prev, wm, 2);
    const SBits<2> t0 = { { wp | wm, wp } }, t1 = { { wp1 | wm1, wp1 } }, t2 = { { wp2 | wm2, wp2 } }, u = { { up | um, um } };
    const SBits<4> K = sb_add<4>(sb_add<3>(t0, t1), sb_add<3>(t2, u));  // K = w'' - (w'[n] + w'[n-1] + w'[n-2]), -4 .. 4
    wp_out = wp; wm_out = wm;
    return ~K.p[3] & (K.p[0] | K.p[1] | K.p[2] | ~SC);                  // K > 0, or K == 0 and Im(y conj(y[n-3])) not negative
}
// ... and two frames per symbol (the D = 768 bank): K = w'' - (w'[n] + w'[n-1]), -3 .. 3
__host__ __device__ __forceinline__ uint32_t exact_slice_word2(uint32_t SX, uint32_t ST, uint32_t SC, uint32_t sx_prev, uint32_t wp_prev, uint32_t wm_prev,
                                                                uint32_t &wp_out, uint32_t &wm_out)
{
    const uint32_t sx1 = exact_funnel(sx_prev, SX, 1), sx2 = exact_funnel(sx_prev, SX, 2);
    const uint32_t wp = ~SX & sx1 & ST, wm = SX & ~sx1 & ~ST;
    const uint32_t up = ~SX & sx2 & SC, um = SX & ~sx2 & ~SC;
    const uint32_t wp1 = exact_funnel(wp_prev, wp, 1), wm1 = exact_funnel(wm_prev, wm, 1);
    const SBits<2> t0 = { { wp | wm, wp } }, t1 = { { wp1 | wm1, wp1 } }, u = { { up | um, um } };
    const SBits<3> K = sb_add<3>(sb_add<3>(t0, t1), u);
    wp_out = wp; wm_out = wm;
    return ~K.p[2] & (K.p[0] | K.p[1] | ~SC);                           // K > 0, or K == 0 and Im(y conj(y[n-2])) not negative
}

} // namespace amps
