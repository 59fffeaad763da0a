// recc_chz_fold.hip.h -- the fold role of the filter bank (recc_channelizer.hip.h): the input samples of a frame, the polyphase delay
// lines as a register ring with their loaders and waits, the fold itself with the radix-4 pass 1 behind it -- for D = 512, and in a
// section of its own for D = 768.
#pragma once
#include "recc_chz_common.hip.h"
#include "recc_chz_fft.hip.h"     // dft4, chz_pos1

namespace amps {

// Input samples of a launch for the edge paths, by launch-relative virtual index v (frame F of this thread: F*D + t and F*D + 256 + t):
// carry, then block, zeros outside both.  Half-steps that lie inside the new block (all but the first and last of a launch) do not
// come here: they are plain coalesced buffer loads (chz_load1_ring).  The choice is made once per half-step, so the common path has
// no branch between the four folds (per-frame branches cost 8 %: they fence the scheduler).
template <typename T = float2> struct ChzIn {
    static constexpr bool SHORT = chz_is_short<T>::value;
    const T *block;
    const float2 *carry;
    int64_t hist, lead, carry_len, nsamp;
    // no branch around the load: the edge paths fetch a batch of these and wait ONCE (round 6: sixteen -- at D = 768
    // nineteen -- generic loads of a workgroup's prologue each behind its own drain were that many HBM round trips in a row)
    __device__ __forceinline__ cf2 generic_nb(int64_t v) const
    {
        const int64_t ci = v + hist, bi = v - lead;
        const bool in_carry = ci < carry_len, ok = ci >= 0 && (in_carry || bi < nsamp);
        if constexpr (SHORT) {
            // sc16 block: the two buffers differ in sample size -- two dword loads from whichever holds the sample (a block sample
            // twice: no branch around a load, no more registers in flight than the fc32 form keeps); a block sample is converted here
            typedef uint32_t __attribute__((may_alias)) raw_t;
            const bool in_block = ok && !in_carry;
            const char *p = in_block ? (const char *)(block + bi) : (const char *)(carry + (ok ? ci : 0));   // any valid address
            const uint32_t d0 = *(const raw_t *)p, d1 = *(const raw_t *)(p + (in_block ? 0 : 4));
            const cf2 b = { (float)(int16_t)(d0 & 0xffffu), (float)(int16_t)(d1 >> 16) };
            return in_block ? b : ok ? (cf2){ __uint_as_float(d0), __uint_as_float(d1) } : (cf2){ 0.f, 0.f };
        } else {
        const float2 *p = in_carry ? carry + ci : block + bi;
        p = ok ? p : carry;                                           // any valid address
        const float2 s = *p;
        return ok ? (cf2){ s.x, s.y } : (cf2){ 0.f, 0.f };
        }
    }
};

// The delay lines as a register RING: branch jb keeps P + 4 slots; at a half-step with rotation BASE the
// logical element i of the old {delay line, new samples} view is ring[jb][(BASE + i) % (P + 4)]: elements 0..P-1 the delay
// line, P and P+1 the samples of this half-step's four frames, P+2 and P+3 those of the NEXT half-step (in flight).  After
// the fold the two oldest slots are dead and receive the loads of the half-step after next, and BASE advances by two: no
// register ever moves (round 1 shifted 32 register pairs per four frames), and a load has two half-steps to land.
// The half-step loop is unrolled over the ring's period of (P + 4) / 2 rotations.
//
// Two frames at a time: eight independent accumulator chains (2 frames x 4 branches), two taps per asm block.  Measured
// (scripts/ubench_pk2.hip): a lone wave on a SIMD issues v_pk_fma_f32 with three distinct register-pair sources every 7.1
// cycles with 4 chains and one-instruction asm statements (the compiler puts an s_nop behind every group of dependent asm
// statements -- it counts an asm statement as zero wait states -- and a lone wave pays a full issue slot for it), 6.2 with 8
// chains; inside one asm block there is nothing to pad, and a dependent v_pk_fma is eight instructions away.
#define CHZ_FMA_LO(d, x, c) "v_pk_fma_f32 %" #d ", %" #x ", %" #c ", %" #d " op_sel_hi:[1,0,1]\n\t"
#define CHZ_FMA_HI(d, x, c) "v_pk_fma_f32 %" #d ", %" #x ", %" #c ", %" #d " op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
#define CHZ_MUL_LO(d, x, c) "v_pk_mul_f32 %" #d ", %" #x ", %" #c " op_sel_hi:[1,0]\n\t"
// acc[f][jb] (+)= x0[f][jb] * c[jb ^ SW_f].lo ; then += x1[f][jb] * c[jb ^ SW_f].hi   (SW_0 = 2, SW_1 = 0: frame 0 has even parity)
template <bool FIRST>
__device__ __forceinline__ void chz_fold_taps2(cf2 (&acc)[2][4], const cf2 (&x0)[2][4], const cf2 (&x1)[2][4], const cf2 (&c)[4])
{
    // operands: 0..7 acc[f][jb] (f major), 8..15 x0, 16..23 x1, 24..27 c[0..3].  Neighbouring instructions share their coefficient
    // pair: a v_pk_fma_f32 with three distinct register-pair sources issues every 6.3 cycles, 5.6 when every second one repeats a
    // source pair of its predecessor (scripts/ubench_pk3.hip, two waves per SIMD)
    if constexpr (FIRST) {
        asm(CHZ_MUL_LO(2, 10, 24) CHZ_MUL_LO(4, 12, 24) CHZ_MUL_LO(3, 11, 25) CHZ_MUL_LO(5, 13, 25)
            CHZ_MUL_LO(0, 8, 26) CHZ_MUL_LO(6, 14, 26) CHZ_MUL_LO(1, 9, 27) CHZ_MUL_LO(7, 15, 27)
            CHZ_FMA_HI(2, 18, 24) CHZ_FMA_HI(4, 20, 24) CHZ_FMA_HI(3, 19, 25) CHZ_FMA_HI(5, 21, 25)
            CHZ_FMA_HI(0, 16, 26) CHZ_FMA_HI(6, 22, 26) CHZ_FMA_HI(1, 17, 27) CHZ_FMA_HI(7, 23, 27)
            : "=&v"(acc[0][0]), "=&v"(acc[0][1]), "=&v"(acc[0][2]), "=&v"(acc[0][3]), "=&v"(acc[1][0]), "=&v"(acc[1][1]), "=&v"(acc[1][2]), "=&v"(acc[1][3])
            : "v"(x0[0][0]), "v"(x0[0][1]), "v"(x0[0][2]), "v"(x0[0][3]), "v"(x0[1][0]), "v"(x0[1][1]), "v"(x0[1][2]), "v"(x0[1][3]),
              "v"(x1[0][0]), "v"(x1[0][1]), "v"(x1[0][2]), "v"(x1[0][3]), "v"(x1[1][0]), "v"(x1[1][1]), "v"(x1[1][2]), "v"(x1[1][3]),
              "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]));
    } else {
        asm(CHZ_FMA_LO(2, 10, 24) CHZ_FMA_LO(4, 12, 24) CHZ_FMA_LO(3, 11, 25) CHZ_FMA_LO(5, 13, 25)
            CHZ_FMA_LO(0, 8, 26) CHZ_FMA_LO(6, 14, 26) CHZ_FMA_LO(1, 9, 27) CHZ_FMA_LO(7, 15, 27)
            CHZ_FMA_HI(2, 18, 24) CHZ_FMA_HI(4, 20, 24) CHZ_FMA_HI(3, 19, 25) CHZ_FMA_HI(5, 21, 25)
            CHZ_FMA_HI(0, 16, 26) CHZ_FMA_HI(6, 22, 26) CHZ_FMA_HI(1, 17, 27) CHZ_FMA_HI(7, 23, 27)
            : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3])
            : "v"(x0[0][0]), "v"(x0[0][1]), "v"(x0[0][2]), "v"(x0[0][3]), "v"(x0[1][0]), "v"(x0[1][1]), "v"(x0[1][2]), "v"(x0[1][3]),
              "v"(x1[0][0]), "v"(x1[0][1]), "v"(x1[0][2]), "v"(x1[0][3]), "v"(x1[1][0]), "v"(x1[1][1]), "v"(x1[1][2]), "v"(x1[1][3]),
              "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]));
    }
}
// frames FA, FA+1 of a half-step (FA = 0: tap windows start at SA = 1 / SB = 0 and 1 / 1; FA = 2: 2 / 1 and 2 / 2), then the
// radix-4 pass 1 of both -> A[FA], A[FA+1]
// `after_first` runs behind the first tap block (q = 0): that block holds the last uses of the two oldest elements of the
// ring's current view, so the caller refills those slots from there (chz_load1_ring)
template <int P, int BASE, int FA, typename Hook>
__device__ __forceinline__ void chz_fold2_ring(const cf2 (&ring)[4][P + 4], const cf2 (&coef)[4][P / 2], const cf2 (&tw1)[3], cf2 *bufA, int t, Hook &&after_first)
{
    constexpr int R = P + 4;
    constexpr int S[2][2] = { { FA == 0 ? 1 : 2, FA == 0 ? 0 : 1 }, { FA == 0 ? 1 : 2, FA == 0 ? 1 : 2 } };   // [frame][jb >= 2]
    cf2 acc[2][4];
#pragma unroll
    for (int q = 0; q < P; q += 2) {
        cf2 x0[2][4], x1[2][4], c[4];
#pragma unroll
        for (int f = 0; f < 2; f++)
#pragma unroll
            for (int jb = 0; jb < 4; jb++) {
                x0[f][jb] = ring[jb][(BASE + S[f][jb >> 1] + q) % R];
                x1[f][jb] = ring[jb][(BASE + S[f][jb >> 1] + q + 1) % R];
            }
#pragma unroll
        for (int j = 0; j < 4; j++) c[j] = coef[j][q / 2];
        if (q == 0) { chz_fold_taps2<true>(acc, x0, x1, c); after_first(); } else chz_fold_taps2<false>(acc, x0, x1, c);
    }
#pragma unroll
    for (int f = 0; f < 2; f++) {
        cf2 o[4];
        dft4(acc[f][0], acc[f][1], acc[f][2], acc[f][3], o);     // radix 4, p = 1: no twiddles
        // the input twiddles of pass 2 (element 4 t + k1 is its point r = t >> 4 of lane 4 (t & 15) + k1: W_64^{r k1}) are applied
        // HERE: the fold waves wait at the barriers more than half of the time, the FFT waves are the critical path of a time step
        cf2 *d = bufA + (FA + f) * CHZ_FB + t;
        d[chz_pos1(0, 0)] = o[0]; d[chz_pos1(0, 1)] = cmul(o[1], tw1[0]); d[chz_pos1(0, 2)] = cmul(o[2], tw1[1]); d[chz_pos1(0, 3)] = cmul(o[3], tw1[2]);
    }
}
// The fast loader.  The two samples frame G of the half-step two behind the one in work brings for this thread go to branches
// 2 (G & 1) + {0, 1}, logical element ELEM + (G >> 1).  For half-steps whose four frames lie inside the new block: the loads are
// issued as inline asm, so that the compiler does not track them -- its own bookkeeping puts `s_waitcnt vmcnt(0)` behind every
// barrier of the loop (the fast / generic join makes it conservative), which drains the loads issued a moment ago.  The fold waits
// with chz_ring_wait instead: vmcnt(8) = "everything but the eight youngest loads", i.e. exactly the loads of the previous
// half-step stay in flight.  The address is the workgroup's descriptor, a wave-uniform scalar byte offset and the lane's constant
// byte offset (no per-load address arithmetic on the VALU, one address dword to move instead of two: with 64-bit VGPR addresses the
// eight loads of a half-step took the fold waves ~350 cycles at the END of their step, when every other wave of the CU was already
// waiting at the barrier).
// The edge path (carry, zero padding: first and last half-steps of a launch; chz_load_half_ring) uses ordinary loads and drains
// them before it returns, so vmcnt(8) is right after either path.
template <int P, int BASE, int ELEM, int G, typename IN>
__device__ __forceinline__ void chz_load1_ring(cf2 (&ring)[4][P + 4], const IN &, int t, chz_rsrc_t rsrc, uint32_t soff)
{
    constexpr int R = P + 4;
    constexpr int E = (BASE + ELEM + (G >> 1)) % R, J = 2 * (G & 1);
    if constexpr (IN::SHORT) {
        // sc16 block: the same two loads per frame, one dword each (a 256-sample chunk is 1 KB).  The packed sample is born in the low
        // register of the slot's own pair -- the same tie -- and chz_ring_wait expands it in place once it has landed.
        const uint32_t voff = (uint32_t)t * (uint32_t)sizeof(chz_sc16);
        const uint32_t so = soff + (uint32_t)((2 * CHZ_BATCH + G) * CHZ_D * sizeof(chz_sc16));
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "+v"(ring[J][E].x) : "v"(voff), "s"(rsrc), "s"(so));
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:1024" : "+v"(ring[J + 1][E].x) : "v"(voff), "s"(rsrc), "s"(so));
    } else {
        // Round 6: raw buffer loads against the workgroup's descriptor (chz_make_rsrc) -- `soff` = byte offset of the half-step in work,
        // the frame fetched here lies 2 * CHZ_BATCH + G frames behind its first sample; the hardware's range check stands in for the
        // clamp of rounds 3-5 (frame index against the last whole frame of the block, on the scalar unit since round 5), and the
        // 64-bit base arithmetic per frame -- ~45 scalar instructions per half-step in the wave that is the kernel's critical path -- is
        // one s_add.
        // "+v": the destination is TIED to the register that holds the slot's dead value, so the new value is born in the ring's own
        // register -- with "=v" the compiler is free to load into a scratch pair and copy it into place at the next control-flow
        // join, i.e. to READ a register whose load is still in flight (it did: tests/test_cpu_inflight_loads.py scans the
        // assembly for any access to such a register before the wait that covers it)
        // (non-temporal loads change nothing here, 0.380 against 0.381 ms: the kernel is bound by VALU issue, not by its input stream)
        const uint32_t voff = (uint32_t)t * (uint32_t)sizeof(float2);
        const uint32_t so = soff + (uint32_t)((2 * CHZ_BATCH + G) * CHZ_D * sizeof(float2));
        asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "+v"(ring[J][E]) : "v"(voff), "s"(rsrc), "s"(so));
        asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen offset:2048" : "+v"(ring[J + 1][E]) : "v"(voff), "s"(rsrc), "s"(so));
    }
}
// The edge loader: the eight loads of the half-step whose first frame is F as ONE batch of bounds-checked loads -- all of them in
// flight, one drain, then into their slots through the same ties as the fast loader's, so that the two paths join with the ring
// where it is and the compiler has nothing to copy behind an in-flight load
template <int P, int BASE, int ELEM, typename IN>
__device__ __forceinline__ void chz_load_half_ring(cf2 (&ring)[4][P + 4], const IN &in, int64_t F, int t)
{
    constexpr int R = P + 4;
    cf2 v[8];
#pragma unroll
    for (int g = 0; g < 4; g++) { v[2 * g] = in.generic_nb((F + g) * CHZ_D + t); v[2 * g + 1] = in.generic_nb((F + g) * CHZ_D + 256 + t); }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]) :: "memory");
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int e = (BASE + ELEM + (g >> 1)) % R, j = 2 * (g & 1);
        asm volatile("v_mov_b64 %0, %1" : "+v"(ring[j][e]) : "v"(v[2 * g]));
        asm volatile("v_mov_b64 %0, %1" : "+v"(ring[j + 1][e]) : "v"(v[2 * g + 1]));
    }
}
// a packed sc16 sample that has landed in the low register of a ring slot -> the slot's cf2, in place: two conversions, no copy
__device__ __forceinline__ void chz_expand_short(cf2 &e)
{
    asm volatile("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t"
                 "v_cvt_f32_i32_sdwa %1, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" : "=v"(e.y), "+v"(e.x));
}
// before a fold: the samples of logical elements P and P+1 (loaded two half-steps ago) have arrived; the empty asm makes
// every use of those registers depend on the wait
// SHORT (sc16 blocks), `expand`: the elements this wait covers were loaded by the fast loader, packed, and are expanded here, behind
// the wait and before their first use (an element is read by eight taps).  `expand` is wave-uniform and false only in edge half-steps
// and in the first two fast ones behind them, which still read what the edge loader left -- converted at the load.  Both arms of
// the branch leave every register where it is: no slot with a load in flight is redefined in either.
template <int P, int BASE, bool SHORT = false>
__device__ __forceinline__ void chz_ring_wait(cf2 (&ring)[4][P + 4], bool expand = false)
{
    constexpr int R = P + 4;
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    asm volatile("" : "+v"(ring[0][(BASE + P) % R]), "+v"(ring[1][(BASE + P) % R]), "+v"(ring[2][(BASE + P) % R]), "+v"(ring[3][(BASE + P) % R]),
                      "+v"(ring[0][(BASE + P + 1) % R]), "+v"(ring[1][(BASE + P + 1) % R]), "+v"(ring[2][(BASE + P + 1) % R]), "+v"(ring[3][(BASE + P + 1) % R]));
    if constexpr (SHORT) {
        if (__builtin_expect(expand, 1)) {
#pragma unroll
            for (int j = 0; j < 4; j++) { chz_expand_short(ring[j][(BASE + P) % R]); chz_expand_short(ring[j][(BASE + P + 1) % R]); }
        }
    }
}



// ---- D = 768: the fold role of the 4/3 x oversampled bank (M = 1024, 40 ksps per channel = two samples per Manchester symbol) ----
// Everything per FRAME is what it is at D = 512 -- eight taps on each of 1024 branches, the same FFT, the same slicer work per bin --
// but a frame now consumes 768 input samples instead of 512: 1.5 x fewer frames per input byte (the D = 512 form ends at
// 0.33 of HBM, bound by VALU issue).  What changes is the bookkeeping of the fold, all of it compile-time:
//   * frame F (F = 0 mod 4 at the start of a half-step; launches and workgroup ranges start on multiples of four frames, where the
//     stream position is a multiple of M) brings the chunks k = 0, 1, 2 of 256 samples; chunk k belongs to branch j = (k - g) & 3,
//     g = F & 3: per half-step of four frames every branch receives THREE samples -- branch j in the frames g with (j + g) & 3 != 3;
//   * branch j of frame g is weighted with coefficient set (j + g + 1) & 3 (the prototype is indexed by the sample's distance from
//     the frame's start, (r - n0) mod M with n0 = (F + 1) D - L = 256 (g + 1) mod M) -- the same 32 coefficients per thread as at
//     D = 512, where the set alternates between j and j ^ 2;
//   * the register ring keeps P + 4 = 12 slots per branch, as at D = 512, and advances by three per half-step: period FOUR
//     half-steps.  In the view of a half-step, elements 0..7 are the delay line, 8..10 its own three samples, 11 the first sample of
//     the next one.  Frame g reads the window [cnt(j, g), cnt(j, g) + 8) of branch j, cnt = samples received so far; every element
//     0..3 dies in the FIRST tap block of a frame pair (position 0 of its last window), and the slot takes a load at once:
//        after the first tap block of frames 0 / 1:  element 0 of branch 3, element 1 of every branch, element 2 of branch 0
//        after the first tap block of frames 2 / 3:  element 2 of branches 1..3, element 3 of branches 0..2
//     The slot of element e receives element e + 12: the samples of the next half-step (9, 10 there) and of the one after (8, 9
//     there), issued in the order they will be needed, so ONE counter serves: s_waitcnt vmcnt(13) in front of either frame pair
//     leaves exactly the thirteen loads issued behind the last one that pair reads.  A load has five to seven frames to land
//     (D = 512: four to eight), 13 x 512 B x 4 waves = 26 KB per CU are in flight at the least.
__host__ __device__ constexpr int chz768_recv(int j, int g) { return ((j + g) & 3) != 3; }           // branch j receives a sample in frame g
__host__ __device__ constexpr int chz768_cnt(int j, int g) { int c = 0; for (int q = 0; q <= g; q++) c += chz768_recv(j, q); return c; }
static_assert(chz768_cnt(0, 0) == 1 && chz768_cnt(0, 3) == 3 && chz768_cnt(1, 2) == 2 && chz768_cnt(2, 1) == 1 && chz768_cnt(3, 0) == 0 && chz768_cnt(3, 3) == 3, "reception table");
constexpr int CHZ768_R = 12;
// frames FA, FA + 1 of a half-step (FA = 0 or 2), then the radix-4 pass 1 of both -> A[FA], A[FA + 1].  The asm block of
// chz_fold_taps2 is the D = 512 one -- its first frame's accumulator jb uses coefficient pair c[jb ^ 2], its second frame's c[jb] --
// handed permuted operands: c[m] = set (m + FA + 2) & 3, second frame = branch jb, first frame = branch (jb + 3) & 3 (all
// indices compile-time: no register moves)
template <int P, int BASE, int FA, typename Hook>
__device__ __forceinline__ void chz768_fold2_ring(const cf2 (&ring)[4][CHZ768_R], const cf2 (&coef)[4][P / 2], const cf2 (&tw1)[3], cf2 *bufA, int t, Hook &&after_first)
{
    static_assert(P == 8 && (FA == 0 || FA == 2), "eight taps per branch, frame pairs 0 / 1 and 2 / 3");
    constexpr int R = CHZ768_R;
    cf2 acc[2][4];
#pragma unroll
    for (int q = 0; q < P; q += 2) {
        cf2 x0[2][4], x1[2][4], c[4];
#pragma unroll
        for (int jb = 0; jb < 4; jb++) {
            const int j0 = (jb + 3) & 3, s0 = chz768_cnt(j0, FA), s1 = chz768_cnt(jb, FA + 1);
            x0[0][jb] = ring[j0][(BASE + s0 + q) % R]; x1[0][jb] = ring[j0][(BASE + s0 + q + 1) % R];
            x0[1][jb] = ring[jb][(BASE + s1 + q) % R]; x1[1][jb] = ring[jb][(BASE + s1 + q + 1) % R];
        }
#pragma unroll
        for (int m = 0; m < 4; m++) c[m] = coef[(m + FA + 2) & 3][q / 2];
        if (q == 0) { chz_fold_taps2<true>(acc, x0, x1, c); after_first(); } else chz_fold_taps2<false>(acc, x0, x1, c);
    }
#pragma unroll
    for (int f = 0; f < 2; f++) {
        cf2 o[4];
        if (f == 0) dft4(acc[0][1], acc[0][2], acc[0][3], acc[0][0], o);     // branch j of the first frame sits in accumulator (j + 1) & 3
        else dft4(acc[1][0], acc[1][1], acc[1][2], acc[1][3], o);
        cf2 *d = bufA + (FA + f) * CHZ_FB + t;
        d[chz_pos1(0, 0)] = o[0]; d[chz_pos1(0, 1)] = cmul(o[1], tw1[0]); d[chz_pos1(0, 2)] = cmul(o[2], tw1[1]); d[chz_pos1(0, 3)] = cmul(o[3], tw1[2]);
    }
}
// The fast loader: the sample branch J receives in frame G of the half-step X half-steps behind the one in work (ring rotation BASE):
// chunk K = (J + G) & 3 of that frame's 768 new samples, into the slot its reception number says.  As at D = 512 (chz_load1_ring):
// one untracked raw buffer load (chz_make_rsrc) tied to the slot's own registers.  `soff` = byte offset of the half-step in work
// inside the workgroup's descriptor; the chunks a half-step fetches are the CONSECUTIVE 2 KB chunks 19 .. 30 behind its own first
// sample -- the stream is read in order -- so chunk c is soff + 2048 (c & ~1) with the odd ones on the 12-bit immediate.
template <int BASE, int X, int G, int J, typename IN>
__device__ __forceinline__ void chz768_load1(cf2 (&ring)[4][CHZ768_R], const IN &, int t, chz_rsrc_t rsrc, uint32_t soff)
{
    constexpr int K = (J + G) & 3;
    static_assert(K != 3, "branch J receives nothing in frame G");
    constexpr int SLOT = (BASE + 7 + chz768_cnt(J, G) + 3 * X) % CHZ768_R;
    if constexpr (IN::SHORT) {
        // sc16 block: the chunks are 1 KB, chunk c at soff + 1024 (c & ~1), the odd ones on the immediate; one dword into the low
        // register of the slot's own pair, expanded in place by chz768_ring_wait
        constexpr int CH = 3 * (4 * X + G) + K;
        const uint32_t voff = (uint32_t)t * (uint32_t)sizeof(chz_sc16);
        const uint32_t so = soff + 1024u * (uint32_t)(CH & ~1);
        if constexpr (CH & 1) asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:1024" : "+v"(ring[J][SLOT].x) : "v"(voff), "s"(rsrc), "s"(so));
        else asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "+v"(ring[J][SLOT].x) : "v"(voff), "s"(rsrc), "s"(so));
    } else {
        constexpr int CH = 3 * (4 * X + G) + K;                      // chunk of 256 samples behind the half-step's first sample
        const uint32_t voff = (uint32_t)t * (uint32_t)sizeof(float2);
        const uint32_t so = soff + 2048u * (uint32_t)(CH & ~1);
        // "+v": the new value is born in the ring's own register (see chz_load1_ring)
        if constexpr (CH & 1) asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen offset:2048" : "+v"(ring[J][SLOT]) : "v"(voff), "s"(rsrc), "s"(so));
        else asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "+v"(ring[J][SLOT]) : "v"(voff), "s"(rsrc), "s"(so));
    }
}
// the edge form (bounds-checked loads against carry and block; F0 = first frame of the half-step in work) in two halves, so that a
// batch of fetches shares one drain
template <int X, int G, int J, typename IN>
__device__ __forceinline__ cf2 chz768_fetch(const IN &in, int64_t F0, int t) { return in.generic_nb((F0 + 4 * X + G) * CHZ_D768 + 256 * ((J + G) & 3) + t); }
template <int BASE, int X, int G, int J>
__device__ __forceinline__ void chz768_put(cf2 (&ring)[4][CHZ768_R], cf2 v)
{
    constexpr int SLOT = (BASE + 7 + chz768_cnt(J, G) + 3 * X) % CHZ768_R;
    asm volatile("v_mov_b64 %0, %1" : "+v"(ring[J][SLOT]) : "v"(v));
}
// the twelve loads of an EDGE half-step (both lists below), one drain
template <int BASE, typename IN>
__device__ __forceinline__ void chz768_loads_generic(cf2 (&ring)[4][CHZ768_R], const IN &in, int64_t F0, int t)
{
    cf2 v[12] = { chz768_fetch<1, 2, 3>(in, F0, t), chz768_fetch<1, 2, 0>(in, F0, t), chz768_fetch<1, 3, 1>(in, F0, t), chz768_fetch<1, 3, 2>(in, F0, t),
                  chz768_fetch<1, 3, 3>(in, F0, t), chz768_fetch<2, 0, 0>(in, F0, t), chz768_fetch<2, 0, 1>(in, F0, t), chz768_fetch<2, 0, 2>(in, F0, t),
                  chz768_fetch<2, 1, 3>(in, F0, t), chz768_fetch<2, 1, 0>(in, F0, t), chz768_fetch<2, 1, 1>(in, F0, t), chz768_fetch<2, 2, 2>(in, F0, t) };
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]) :: "memory");
    chz768_put<BASE, 1, 2, 3>(ring, v[0]); chz768_put<BASE, 1, 2, 0>(ring, v[1]); chz768_put<BASE, 1, 3, 1>(ring, v[2]); chz768_put<BASE, 1, 3, 2>(ring, v[3]);
    chz768_put<BASE, 1, 3, 3>(ring, v[4]); chz768_put<BASE, 2, 0, 0>(ring, v[5]); chz768_put<BASE, 2, 0, 1>(ring, v[6]); chz768_put<BASE, 2, 0, 2>(ring, v[7]);
    chz768_put<BASE, 2, 1, 3>(ring, v[8]); chz768_put<BASE, 2, 1, 0>(ring, v[9]); chz768_put<BASE, 2, 1, 1>(ring, v[10]); chz768_put<BASE, 2, 2, 2>(ring, v[11]);
}
// what the half-steps -2 and -1 would have left in flight when half-step 0 (first frame F0, BASE 0) begins: its own three samples per
// branch (slots 8..10), the first of half-step 1 (slot 11) and -- branches 0..2, whose element 0 is dead already -- the second (slot 0)
template <typename IN>
__device__ __forceinline__ void chz768_prime(cf2 (&ring)[4][CHZ768_R], const IN &in, int64_t F0, int t)
{
    cf2 a[12] = { chz768_fetch<0, 0, 0>(in, F0, t), chz768_fetch<0, 0, 1>(in, F0, t), chz768_fetch<0, 0, 2>(in, F0, t), chz768_fetch<0, 1, 3>(in, F0, t),
                  chz768_fetch<0, 1, 0>(in, F0, t), chz768_fetch<0, 1, 1>(in, F0, t), chz768_fetch<0, 2, 2>(in, F0, t), chz768_fetch<0, 2, 3>(in, F0, t),
                  chz768_fetch<0, 2, 0>(in, F0, t), chz768_fetch<0, 3, 1>(in, F0, t), chz768_fetch<0, 3, 2>(in, F0, t), chz768_fetch<0, 3, 3>(in, F0, t) };
    cf2 b[7] = { chz768_fetch<1, 0, 0>(in, F0, t), chz768_fetch<1, 0, 1>(in, F0, t), chz768_fetch<1, 0, 2>(in, F0, t), chz768_fetch<1, 1, 3>(in, F0, t),
                 chz768_fetch<1, 1, 0>(in, F0, t), chz768_fetch<1, 1, 1>(in, F0, t), chz768_fetch<1, 2, 2>(in, F0, t) };
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]) :: "memory");
    asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]));
    chz768_put<0, 0, 0, 0>(ring, a[0]); chz768_put<0, 0, 0, 1>(ring, a[1]); chz768_put<0, 0, 0, 2>(ring, a[2]); chz768_put<0, 0, 1, 3>(ring, a[3]);
    chz768_put<0, 0, 1, 0>(ring, a[4]); chz768_put<0, 0, 1, 1>(ring, a[5]); chz768_put<0, 0, 2, 2>(ring, a[6]); chz768_put<0, 0, 2, 3>(ring, a[7]);
    chz768_put<0, 0, 2, 0>(ring, a[8]); chz768_put<0, 0, 3, 1>(ring, a[9]); chz768_put<0, 0, 3, 2>(ring, a[10]); chz768_put<0, 0, 3, 3>(ring, a[11]);
    chz768_put<0, 1, 0, 0>(ring, b[0]); chz768_put<0, 1, 0, 1>(ring, b[1]); chz768_put<0, 1, 0, 2>(ring, b[2]); chz768_put<0, 1, 1, 3>(ring, b[3]);
    chz768_put<0, 1, 1, 0>(ring, b[4]); chz768_put<0, 1, 1, 1>(ring, b[5]); chz768_put<0, 1, 2, 2>(ring, b[6]);
}
// the six fast loads behind the first tap block of frames 0 / 1, and the six behind that of frames 2 / 3, in the order they are needed
template <int BASE, typename IN>
__device__ __forceinline__ void chz768_loads_a(cf2 (&ring)[4][CHZ768_R], const IN &in, int t, chz_rsrc_t rs, uint32_t so)
{
    chz768_load1<BASE, 1, 2, 3>(ring, in, t, rs, so); chz768_load1<BASE, 1, 2, 0>(ring, in, t, rs, so);
    chz768_load1<BASE, 1, 3, 1>(ring, in, t, rs, so); chz768_load1<BASE, 1, 3, 2>(ring, in, t, rs, so);
    chz768_load1<BASE, 1, 3, 3>(ring, in, t, rs, so); chz768_load1<BASE, 2, 0, 0>(ring, in, t, rs, so);
}
template <int BASE, typename IN>
__device__ __forceinline__ void chz768_loads_b(cf2 (&ring)[4][CHZ768_R], const IN &in, int t, chz_rsrc_t rs, uint32_t so)
{
    chz768_load1<BASE, 2, 0, 1>(ring, in, t, rs, so); chz768_load1<BASE, 2, 0, 2>(ring, in, t, rs, so);
    chz768_load1<BASE, 2, 1, 3>(ring, in, t, rs, so); chz768_load1<BASE, 2, 1, 0>(ring, in, t, rs, so);
    chz768_load1<BASE, 2, 1, 1>(ring, in, t, rs, so); chz768_load1<BASE, 2, 2, 2>(ring, in, t, rs, so);
}
// in front of frames 0 / 1: element 8 of every branch and element 9 of branches 0, 1 have arrived (everything but the thirteen
// youngest loads); in front of frames 2 / 3: element 9 of branches 2, 3 and element 10 of every branch (again thirteen)
// SHORT (sc16 blocks; chz_expand_short, see chz_ring_wait), `age` = fast half-steps run before this one (wave-uniform): a half-step
// meets the packed elements of the one before it (element 9 of branch 3 and element 10 of every branch: the samples of frames 2 / 3)
// and of the one before that (element 8 of every branch, element 9 of branches 0..2); whatever an edge half-step or the prologue
// loaded arrived converted.  age < 0 in edge half-steps.
template <int BASE, int FA, bool SHORT = false>
__device__ __forceinline__ void chz768_ring_wait(cf2 (&ring)[4][CHZ768_R], int age = 0)
{
    constexpr int R = CHZ768_R;
    asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
    if constexpr (FA == 0) {
        asm volatile("" : "+v"(ring[0][(BASE + 8) % R]), "+v"(ring[1][(BASE + 8) % R]), "+v"(ring[2][(BASE + 8) % R]), "+v"(ring[3][(BASE + 8) % R]),
                          "+v"(ring[0][(BASE + 9) % R]), "+v"(ring[1][(BASE + 9) % R]));
        if constexpr (SHORT) {
            if (__builtin_expect(age >= 2, 1)) {
#pragma unroll
                for (int j = 0; j < 4; j++) chz_expand_short(ring[j][(BASE + 8) % R]);
                chz_expand_short(ring[0][(BASE + 9) % R]); chz_expand_short(ring[1][(BASE + 9) % R]);
            }
        }
    } else {
        asm volatile("" : "+v"(ring[2][(BASE + 9) % R]), "+v"(ring[3][(BASE + 9) % R]),
                          "+v"(ring[0][(BASE + 10) % R]), "+v"(ring[1][(BASE + 10) % R]), "+v"(ring[2][(BASE + 10) % R]), "+v"(ring[3][(BASE + 10) % R]));
        if constexpr (SHORT) {
            if (__builtin_expect(age >= 1, 1)) {
                if (__builtin_expect(age >= 2, 1)) chz_expand_short(ring[2][(BASE + 9) % R]);
                chz_expand_short(ring[3][(BASE + 9) % R]);
#pragma unroll
                for (int j = 0; j < 4; j++) chz_expand_short(ring[j][(BASE + 10) % R]);
            }
        }
    }
}

} // namespace amps
