// recc_chz_fft.hip.h -- the FFT-1024 of the filter bank (recc_channelizer.hip.h) as 4 x 16 x 16: the radix-4 butterfly the fold role
// runs on its own registers, the LDS layouts of a frame buffer, and the two radix-16 passes, one frame per wave.
#pragma once
#include "recc_chz_common.hip.h"

namespace amps {

__device__ __forceinline__ void dft4(cf2 a0, cf2 a1, cf2 a2, cf2 a3, cf2 (&o)[4])
{
    const cf2 v0 = a0 + a2, v1 = a0 - a2, v2 = a1 + a3, d = a1 - a3;
    o[0] = v0 + v2; o[1] = add_mi(v1, d); o[2] = v0 - v2; o[3] = sub_mi(v1, d);
}

// e^{-2 pi i num / den}, argument reduced exactly (sincospif)
__device__ __forceinline__ cf2 chz_twiddle(int num, int den)
{
    float sn, cs;
    sincospif(-2.0f * (float)num / (float)den, &sn, &cs);
    return (cf2){ cs, sn };
}


// LDS layouts of a frame buffer (cf2 elements unless noted); every access of the pipeline is bank-conflict free (PMC:
// SQ_LDS_BANK_CONFLICT = 0; a one-pad-per-16 layout cost 17 % of the LDS cycles):
//   chz_pos1: pass-1 output, element 4 t + k1 at t + 260 k1 -- the fold's stores are stride 1 across lanes, and pass 2's gather
//             (the compiler pairs its reads into ds_read2_b64: 16-lane groups, 16 bank pairs) hits (i >> 2) + 4 (i & 3) mod 16;
//   chz_pos2: pass-2 output, n + 4 (n >> 6): no padding inside 64 consecutive elements (reads i + 64 r of consecutive lanes are
//             consecutive), and the stride-64 write-back of pass 2 advances 8 banks per four lanes;
//   planar  : pass-3 output = the spectrum in natural order, as FLOATS, in blocks of 128 bins: [re of the block's first 64 bins |
//             re of its last 64 | im of the first 64 | im of the last 64] -- the slicer role owns bins l and l + 64 of a block per
//             lane, so one ds_read2st64_b32 delivers (re of its two channels) as the register PAIR that packed fp32
//             instructions take as it is, the next one (im, im); 64 consecutive lanes read 64 consecutive floats.
__host__ __device__ constexpr int chz_pos1(int t, int k1) { return t + 260 * k1; }
__host__ __device__ constexpr int chz_pos2(int n) { return n + 4 * (n >> 6); }
__host__ __device__ constexpr int chz_planar(int n) { return 256 * (n >> 7) + (n & 127); }   // real part; the imaginary part is 128 floats further
static_assert(chz_pos1(255, 3) < CHZ_FB && chz_pos2(1023) < CHZ_FB && chz_planar(1023) + 128 < CHZ_FBF, "frame buffer too small for the layouts");

// pass 2, radix 16, p = 4, one frame per wave, in place.  lane i: k = i & 3, u[r] = A[i + 64 r] e^{-2 pi i r k / 64},
// X = DFT16(u), A[16 (i - k) + k + 4 r] = X[r].  The input twiddles W_64^{r k} have already been applied by the fold role
// (chz_fold2_ring): read from an LDS table here, one pair at a time between the multiplies, they cost eight exposed LDS
// latencies per pass (measured with s_memtime: 2950 cycles per frame against 1780 for pass 3).
__device__ __forceinline__ void chz_p2(cf2 *A, int lane)
{
    const int k = lane & 3;
    cf2 u[16];
    // pass 1 left element 4 t + k1 at chz_pos1(t, k1): lane i wants 4 t + k1 = i + 64 r, i.e. t = (i >> 2) + 16 r, k1 = i & 3
    const cf2 *src = A + chz_pos1(lane >> 2, k);
#pragma unroll
    for (int r = 0; r < 16; r++) u[r] = src[16 * r];
    // DFT16 = 4 x DFT4 over a (s = 4a + b), twiddle W16^{bc}, 4 x DFT4 over b -> X[c + 4d]
    cf2 v[4][4];
#pragma unroll
    for (int b = 0; b < 4; b++) dft4(u[b], u[4 + b], u[8 + b], u[12 + b], v[b]);
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
    v[1][1] = cmul_s(v[1][1], (cf2){ C1, -S1 });                // W16^1
    v[1][2] = cmul_s(v[1][2], (cf2){ R2, -R2 });                // W16^2
    v[1][3] = cmul_s(v[1][3], (cf2){ S1, -C1 });                // W16^3
    v[2][1] = cmul_s(v[2][1], (cf2){ R2, -R2 });                // W16^2
    v[2][2] = mul_mi(v[2][2]);                                  // W16^4 = -i
    v[2][3] = cmul_s(v[2][3], (cf2){ -R2, -R2 });               // W16^6
    v[3][1] = cmul_s(v[3][1], (cf2){ S1, -C1 });                // W16^3
    v[3][2] = cmul_s(v[3][2], (cf2){ -R2, -R2 });               // W16^6
    v[3][3] = cmul_s(v[3][3], (cf2){ -C1, S1 });                // W16^9
    // all reads of this wave precede its writes in program order; nobody else touches this frame during pass 2
    cf2 *dst = A + 17 * (lane - k) + k;                         // chz_pos2(16 (i-k) + k + 4 r) = 17 (i-k) + k + 4 r   (k + 4 r < 64)
#pragma unroll
    for (int c = 0; c < 4; c++) {
        cf2 X[4];
        dft4(v[0][c], v[1][c], v[2][c], v[3][c], X);
#pragma unroll
        for (int d = 0; d < 4; d++) dst[4 * (c + 4 * d)] = X[d];
    }
}

// pass 3 of the 4 x 16 x 16 factorisation, radix 16, p = 64, one frame per wave:
//   lane i: u[r] = A[i + 64 r] W_1024^{r i};  bin i + 64 q = DFT16(u)[q]   (natural order, planar layout over the same buffer:
//   every output depends on all sixteen inputs, so the reads have returned before the first store is issued)
template <int NT>
__device__ __forceinline__ void chz_p3(cf2 *A, const cf2 (&tw)[NT], int lane)
{
    static_assert(NT == 15 || NT == 1, "fifteen twiddles (NT = 1: the role that does not run pass 3)");
    if constexpr (NT == 15) {
    cf2 u[16];
    const cf2 *src = A + lane;                                  // chz_pos2(lane + 64 r) = lane + 68 r
#pragma unroll
    for (int r = 0; r < 16; r++) u[r] = src[68 * r];
#pragma unroll
    for (int r = 1; r < 16; r++) u[r] = cmul(u[r], tw[r - 1]);
    cf2 v[4][4];
#pragma unroll
    for (int b = 0; b < 4; b++) dft4(u[b], u[4 + b], u[8 + b], u[12 + b], v[b]);
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
    v[1][1] = cmul_s(v[1][1], (cf2){ C1, -S1 });
    v[1][2] = cmul_s(v[1][2], (cf2){ R2, -R2 });
    v[1][3] = cmul_s(v[1][3], (cf2){ S1, -C1 });
    v[2][1] = cmul_s(v[2][1], (cf2){ R2, -R2 });
    v[2][2] = mul_mi(v[2][2]);
    v[2][3] = cmul_s(v[2][3], (cf2){ -R2, -R2 });
    v[3][1] = cmul_s(v[3][1], (cf2){ S1, -C1 });
    v[3][2] = cmul_s(v[3][2], (cf2){ -R2, -R2 });
    v[3][3] = cmul_s(v[3][3], (cf2){ -C1, S1 });
    float *dst = (float *)A + lane;                             // chz_planar(lane + 64 q) = chz_planar(64 q) + lane
#pragma unroll
    for (int c = 0; c < 4; c++) {
        cf2 X[4];
        dft4(v[0][c], v[1][c], v[2][c], v[3][c], X);
#pragma unroll
        for (int d = 0; d < 4; d++) { dst[chz_planar(64 * (c + 4 * d))] = X[d].x; dst[chz_planar(64 * (c + 4 * d)) + 128] = X[d].y; }
    }
    }
}

} // namespace amps
