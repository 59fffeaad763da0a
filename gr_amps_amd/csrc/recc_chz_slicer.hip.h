// recc_chz_slicer.hip.h -- the slicer fused behind the filter bank's FFT (recc_channelizer.hip.h, pass-3 role): the stream state of a
// lane's channel pairs under the four slicer specs, and the half-batch step that reads the planar spectrum and writes ring words (or,
// unfused, the channel-major block).
#pragma once
#include "amps_recc_numerics.h"   // AMPS_SLICER_*
#include "recc_chz_common.hip.h"
#include "recc_slice.hip.h"       // f2, fm_phase_planar, fm_phase_planar_n, exact_slice_word2 / 3

namespace amps {

// Slicer state of TWO channels of one lane, planar (.x = the first channel, .y = the second): the specs of
// include/amps_recc_numerics.h, operation by operation, two channels per packed instruction.
// SPS = frames per Manchester symbol: 3 behind the D = 512 bank, 2 behind the D = 768 one (the partner of specs B / D is SPS frames
// back, the boxcar of specs A / C is SPS long -- at SPS = 2 its ordered sum is d[n-1] + d[n] whatever the parity)
template <int SL, int SPS = 3> struct ChzSlicePair {
    static_assert(SPS == 2 || SPS == 3, "frames per symbol");
    f2 pr, pi;               // spec A / C: the bins one frame earlier
    f2 d1, d2;               // spec A / C: the last two discriminator outputs
    f2 h1r, h1i, h2r, h2i, h3r, h3i;   // spec B: the bins one, two and three frames earlier
    uint32_t gw[2];          // SIGN bits of the statistic, newest at bit 0 (the slicer bit is the inverted sign)
    // spec D: three sign streams per channel as shift registers (newest at bit 0) -- Im y, Im(y conj(y[n-1])), Im(y conj(y[n-3])) --
    // and, latched every 32 frames, the previous word of Im y's signs and of the two wrap words (exact_word)
    uint32_t sx[2], st[2], sxp[2], wpp[2], wmp[2];   // (the third stream's signs live in gw)
    __device__ __forceinline__ void reset()
    {
        const f2 z = { 0.f, 0.f };
        pr = pi = d1 = d2 = h1r = h1i = h2r = h2i = h3r = h3i = z;
        gw[0] = gw[1] = 0u;                                           // "ones before the stream": sign bits clear
        sx[0] = sx[1] = st[0] = st[1] = sxp[0] = sxp[1] = wpp[0] = wpp[1] = wmp[0] = wmp[1] = 0u;
    }
    // Spec D, once per 32 frames and channel: the slicer bits of the word just completed (newest at bit 0) from the sign words,
    // 32 frames per instruction.  delay(W, Wprev, j) = the stream j frames earlier.
    __device__ __forceinline__ uint32_t exact_word(int e)
    {
        uint32_t wp, wm;
        const uint32_t g = SPS == 3 ? exact_slice_word3(sx[e], st[e], gw[e], sxp[e], wpp[e], wmp[e], wp, wm)    // recc_slice.hip.h
                                    : exact_slice_word2(sx[e], st[e], gw[e], sxp[e], wpp[e], wmp[e], wp, wm);
        sxp[e] = sx[e]; wpp[e] = wp; wmp[e] = wm;
        return g;
    }
    template <int PAR> __device__ __forceinline__ void step(f2 yr, f2 yi)   // PAR = parity of the absolute frame index
    {
        if constexpr (SL == AMPS_SLICER_EXACT) {
            const f2 it = __builtin_elementwise_fma(yi, pr, -(yr * pi));       // Im(y conj(y[n-1]))
            const f2 qr = SPS == 3 ? h3r : h2r, qi = SPS == 3 ? h3i : h2i;
            const f2 ic = __builtin_elementwise_fma(yi, qr, -(yr * qi));       // Im(y conj(y[n-SPS]))
            sx[0] = __builtin_amdgcn_alignbit(sx[0], __float_as_uint(yi.x), 31);
            sx[1] = __builtin_amdgcn_alignbit(sx[1], __float_as_uint(yi.y), 31);
            st[0] = __builtin_amdgcn_alignbit(st[0], __float_as_uint(it.x), 31);
            st[1] = __builtin_amdgcn_alignbit(st[1], __float_as_uint(it.y), 31);
            gw[0] = __builtin_amdgcn_alignbit(gw[0], __float_as_uint(ic.x), 31);
            gw[1] = __builtin_amdgcn_alignbit(gw[1], __float_as_uint(ic.y), 31);
            h3r = h2r; h3i = h2i; h2r = pr; h2i = pi; pr = yr; pi = yi;
        } else if constexpr (SL == AMPS_SLICER_PRODUCT) {
            // g = !signbit(yi * pr3 - yr * pi3), the partner SPS frames (one Manchester symbol) earlier
            const f2 sd = SPS == 3 ? yi * h3r - yr * h3i : yi * h2r - yr * h2i;
            gw[0] = __builtin_amdgcn_alignbit(gw[0], __float_as_uint(sd.x), 31);
            gw[1] = __builtin_amdgcn_alignbit(gw[1], __float_as_uint(sd.y), 31);
            h3r = h2r; h3i = h2i; h2r = h1r; h2i = h1i; h1r = yr; h1i = yi;
        } else {
            f2 d;
            if constexpr (SL == AMPS_SLICER_SINE) d = __builtin_elementwise_fma(yi, pr, -(yr * pi));     // Im(y conj(prev))
            else {
                const f2 re = __builtin_elementwise_fma(yr, pr, yi * pi);                                 // y conj(prev)
                const f2 im = __builtin_elementwise_fma(yi, pr, -(yr * pi));
                d = fm_phase_planar(re, im);
            }
            // window [n-2, n]: n even -> (d[n-2] + d[n-1]) + d[n];  n odd -> d[n-2] + (d[n-1] + d[n])
            const f2 s = SPS == 2 ? d1 + d : PAR == 0 ? (d2 + d1) + d : d2 + (d1 + d);
            const f2 sp = SL == AMPS_SLICER_SINE ? s : s + (f2){ 0.0f, 0.0f };   // spec A: g = (S >= 0), i.e. -0 counts as +0 (see step4)
            gw[0] = __builtin_amdgcn_alignbit(gw[0], __float_as_uint(sp.x), 31);
            gw[1] = __builtin_amdgcn_alignbit(gw[1], __float_as_uint(sp.y), 31);
            d2 = d1; d1 = d;
            pr = yr; pi = yi;
        }
    }
    // the four frames of a half-batch (frame 0 has even parity).  Spec A: the four arctangents are independent of the stream
    // state, so they are evaluated in lock step (fm_phase_planar_n) before the sequential boxcar / slicer part
    __device__ __forceinline__ void step4(const f2 (&yr)[4], const f2 (&yi)[4])
    {
        if constexpr (SL == AMPS_SLICER_ATAN_BOXCAR) {
            f2 re[4], im[4], d[4];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f2 qr = g ? yr[g - 1] : pr, qi = g ? yi[g - 1] : pi;
                re[g] = __builtin_elementwise_fma(yr[g], qr, yi[g] * qi);                                   // y conj(prev)
                im[g] = __builtin_elementwise_fma(yi[g], qr, -(yr[g] * qi));
            }
            fm_phase_planar_n<4>(re, im, d);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f2 s = SPS == 2 ? d1 + d[g] : (g & 1) == 0 ? (d2 + d1) + d[g] : d2 + (d1 + d[g]);
                // g = (S >= 0): S + (+0) turns the one negative-signed value that counts as >= 0, -0, into +0 (and leaves every
                // other finite S alone), after which the bit is the inverted sign -- one packed add and two funnel shifts for
                // the pair instead of two compares, two selects and two shifts
                const f2 sp = s + (f2){ 0.0f, 0.0f };
                gw[0] = __builtin_amdgcn_alignbit(gw[0], __float_as_uint(sp.x), 31);
                gw[1] = __builtin_amdgcn_alignbit(gw[1], __float_as_uint(sp.y), 31);
                d2 = d1; d1 = d[g];
            }
            pr = yr[3]; pi = yi[3];
        } else {
#pragma unroll
            for (int g = 0; g < 4; g++) { if (g & 1) step<1>(yr[g], yi[g]); else step<0>(yr[g], yi[g]); }
        }
    }
    // Spec D with the three frames of history handed in instead of kept: hr[0] / hi[0] = the bins one frame before yr[0], hr[1] two,
    // hr[2] three.  Nothing is copied at the end -- the caller's four frames ARE the next step's history (ChzSlicer::half: two
    // buffers used alternately, the parity a compile-time constant).  Round 4 kept (pr, pi, h2, h3) as members: six v_mov_b64 per
    // channel pair and time step across the loop's back edge, 12 of the kernel's 528 VALU instructions per frame.
    __device__ __forceinline__ void step4_hist(const f2 (&yr)[4], const f2 (&yi)[4], const f2 (&hr)[3], const f2 (&hi)[3])
    {
        static_assert(SL == AMPS_SLICER_EXACT, "spec D only");
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const f2 p1r = g >= 1 ? yr[g - 1] : hr[0], p1i = g >= 1 ? yi[g - 1] : hi[0];
            const f2 p3r = g >= SPS ? yr[g - SPS] : hr[SPS - 1 - g], p3i = g >= SPS ? yi[g - SPS] : hi[SPS - 1 - g];
            const f2 it = __builtin_elementwise_fma(yi[g], p1r, -(yr[g] * p1i));       // Im(y conj(y[n-1]))
            const f2 ic = __builtin_elementwise_fma(yi[g], p3r, -(yr[g] * p3i));       // Im(y conj(y[n-SPS]))
            sx[0] = __builtin_amdgcn_alignbit(sx[0], __float_as_uint(yi[g].x), 31);
            sx[1] = __builtin_amdgcn_alignbit(sx[1], __float_as_uint(yi[g].y), 31);
            st[0] = __builtin_amdgcn_alignbit(st[0], __float_as_uint(it.x), 31);
            st[1] = __builtin_amdgcn_alignbit(st[1], __float_as_uint(it.y), 31);
            gw[0] = __builtin_amdgcn_alignbit(gw[0], __float_as_uint(ic.x), 31);
            gw[1] = __builtin_amdgcn_alignbit(gw[1], __float_as_uint(ic.y), 31);
        }
    }
    // the ring word of the 32 frames just completed (oldest frame at bit 0)
    __device__ __forceinline__ uint32_t word(int e)
    {
        if constexpr (SL == AMPS_SLICER_EXACT) return __builtin_bitreverse32(exact_word(e));
        else return ~__builtin_bitreverse32(gw[e]);
    }
};

// The slicer of the pass-3 role: NP = 2 channel pairs per lane (pairs J0 .. J0 + NP - 1 of the wave's eight).
// Bin ownership.  The planar layout keeps a frame in eight blocks of 128 bins, [re of bins 0..63 | re of 64..127 | im | im]; a lane's
// PAIR is two bins 64 apart in one block, so the four floats a frame brings for it sit at base + {0, 64, 128, 192} (two
// ds_read2st64_b32) and arrive as the register pairs (re, re) and (im, im) of its two channels.  With W = grp_w residues per
// block belonging to this handle (64 = all of them) a frame holds 8 W pairs, numbered vp = W * block + i'; pair j of (wave wf, lane)
// is vp = 64 (4 (J0 + j) + wf) + lane.  W = 64: pair j holds bins 512 j + 128 wf + lane and + 64, consecutive lanes read consecutive
// floats.  A pair-wave none of whose bins is decoded by this handle is skipped (wave-uniform).
template <int SL, bool IQ, int SPS = 3> struct ChzSlicer {
    static constexpr int NB = CHZ_BATCH, M = CHZ_M, J0 = 0, NP = 2;   // channel pairs of a lane
    ChzSlicePair<SL, SPS> S[NP];
    uint32_t ch[NP][2];                                           // row of the bin (>= n_channels: not decoded by this handle)
    uint32_t pbase[NP];                                           // float offset of the pair's first real part in a planar frame
    bool pair_on[NP];
    uint32_t hold[NP][2][4];                                      // finished ring words waiting for their 16-byte store
    int nheld;
    uint64_t mask32;
    // spec D: the four frames of the half-batch in work and of the one before it, per channel pair (step4_hist); only frames 1..3 of
    // the older buffer are ever read again, so what stays live across a time step is what the members (pr, pi, h2, h3) used to hold
    static constexpr bool PINGPONG = !IQ && SL == AMPS_SLICER_EXACT;
    f2 Yr[PINGPONG ? 2 : 1][NP][NB], Yi[PINGPONG ? 2 : 1][NP][NB];
    __device__ __forceinline__ void clear_frames()
    {
        if constexpr (PINGPONG) {
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int j = 0; j < NP; j++)
#pragma unroll
                    for (int g = 0; g < NB; g++) { Yr[b][j][g] = (f2){ 0.f, 0.f }; Yi[b][j][g] = (f2){ 0.f, 0.f }; }
        }
    }
    __device__ __forceinline__ void init(const ChzArgs &a, int wf, int lane)
    {
        nheld = 0;
        mask32 = 2ull * a.ring_words - 1;
        clear_frames();
#pragma unroll
        for (int j = 0; j < NP; j++) {
            S[j].reset();
            const uint32_t vp = 64u * (4u * (J0 + j) + (uint32_t)wf) + (uint32_t)lane;
            const bool valid = vp < 8u * a.grp_w;
            const uint32_t blk = vp / a.grp_w, ip = vp - blk * a.grp_w, k0 = 128u * blk + a.grp_r * a.grp_w + ip;
            pbase[j] = valid ? 256u * blk + a.grp_r * a.grp_w + ip : 0u;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                ch[j][e] = valid ? (uint32_t)a.bin2row[(k0 + 64u * e) & (M - 1)] : 0xffffu;
#pragma unroll
                for (int k = 0; k < 4; k++) hold[j][e][k] = 0u;
            }
            pair_on[j] = __ballot(ch[j][0] < a.n_channels || ch[j][1] < a.n_channels) != 0;   // wave-uniform
        }
    }
    // the four frames of half-batch hs: slice (or, unfused, store) this lane's bins.
    // KIND 0 = any half-batch (pre-roll, frames before the stream, the range's last one: every rare case behind a dynamic test);
    // KIND 1 / 2 = a STEADY half-batch -- real frames (F >= f0), not the range's last, no stream-start reset -- that does not /
    // does complete a 32-frame word.  Round 4: with the rare cases tested inside the hot loop every one of them was a control-flow
    // merge through which the compiler carried the whole slicer state in a second register set: ~50 v_mov per time step and wave
    // (8 % of the kernel's VALU instructions) for branches taken once in eight steps or twice per launch.  The role's loop now runs
    // seven KIND-1 steps and one KIND-2 step per word, and KIND 0 only at the two ends of a workgroup's range.
    // PAR = parity of the time step (spec D: which of the two frame buffers this half-batch is read into; the other one holds
    // the half-batch before it.  Every half-batch between the first and the last sliced one is sliced, in consecutive time steps.)
    template <int KIND = 0, int PAR = 0>
    __device__ __forceinline__ void half(const ChzArgs &a, const cf2 *buf, int64_t fs, int64_t f0, int64_t f1, int hs)
    {
        const int64_t F = fs + (int64_t)NB * hs;          // first frame of the half-batch (multiple of 4)
        const float *Af = (const float *)(buf + (hs & (CHZ_SLOTS - 1)) * NB * CHZ_FB);
#pragma unroll
        for (int j = 0; j < NP; j++) {
            if (!pair_on[j]) continue;
            if constexpr (PINGPONG) {
                f2 (&yr)[NB] = Yr[PAR][j];
                f2 (&yi)[NB] = Yi[PAR][j];
#pragma unroll
                for (int g = 0; g < NB; g++) {
                    const float *q = Af + pbase[j] + g * CHZ_FBF;
                    yr[g] = (f2){ q[0], q[64] };
                    yi[g] = (f2){ q[128], q[192] };
                }
                const f2 hr[3] = { Yr[PAR ^ 1][j][3], Yr[PAR ^ 1][j][2], Yr[PAR ^ 1][j][1] };
                const f2 hi[3] = { Yi[PAR ^ 1][j][3], Yi[PAR ^ 1][j][2], Yi[PAR ^ 1][j][1] };
                S[j].step4_hist(yr, yi, hr, hi);
                continue;
            }
            f2 yr[NB], yi[NB];
#pragma unroll
            for (int g = 0; g < NB; g++) {
                const float *q = Af + pbase[j] + g * CHZ_FBF;
                yr[g] = (f2){ q[0], q[64] };
                yi[g] = (f2){ q[128], q[192] };
            }
            if constexpr (IQ) {
                // four frames of a bin leave as one 32-byte run of the channel-major block
                const int ng = KIND != 0 ? NB : (int)(f1 - F < (int64_t)NB ? f1 - F : (int64_t)NB);
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    if (ch[j][e] < a.n_channels) {
                        float2 *dstp = a.out + (uint64_t)ch[j][e] * a.ld + F;
                        if (ng == NB) {
#pragma unroll
                            for (int g = 0; g < NB; g += 2)
                                *(float4 *)(dstp + g) = make_float4(yr[g][e], yi[g][e], yr[g + 1][e], yi[g + 1][e]);
                        } else {
#pragma unroll
                            for (int g = 0; g < NB; g++)
                                if (g < ng) dstp[g] = make_float2(yr[g][e], yi[g][e]);
                        }
                    }
                }
            } else {
                S[j].step4(yr, yi);
            }
        }
        if constexpr (!IQ && KIND != 1) {
            if (KIND == 0 && a.stream_start && F < 0) {   // frames before the stream are exactly +0 (the FFT of zeros may hold -0):
                asm volatile("" ::: "memory");            // the state they leave is that of a fresh stream (a real branch, twice per launch)
#pragma unroll
                for (int j = 0; j < NP; j++) S[j].reset();
                clear_frames();
            }
            if constexpr (SL == AMPS_SLICER_EXACT) {
                // the word boundary inside the pre-roll (f0 - 1): latch the previous-word state the first real word needs
                if (KIND == 0 && F < f0 && ((F + NB - 1) & 31) == 31) {
#pragma unroll
                    for (int j = 0; j < NP; j++) { S[j].exact_word(0); S[j].exact_word(1); }
                }
            }
            if (KIND == 2 || (F >= f0 && ((F + NB - 1) & 31) == 31)) {   // 32 real frames collected (f0 is a multiple of 64)
                // A channel's words leave as ONE 16-byte store per 128 frames (aligned group of four ring dwords): single
                // dwords scattered over the channels' ring rows are counted -- and written -- as 32-byte sectors, 8x the 27 MB
                // of slicer bits per GiB of input (round 1: 215 MB of 1.36 GB traffic).  Ranges start and end on 64-frame
                // boundaries, so a run that is not a whole group is exactly two words.
                const uint64_t w = (a.n_done + (uint64_t)(F + NB - 1)) >> 5;   // absolute ring dword of the finished word
                const bool last = KIND == 0 && F + NB >= f1;
#pragma unroll
                for (int j = 0; j < NP; j++)
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        uint32_t word = S[j].word(e);
                        if ((SL == AMPS_SLICER_PRODUCT || SL == AMPS_SLICER_EXACT) && a.stream_start && F + NB - 1 == 31) word |= (1u << SPS) - 1u;   // no partner yet: g = 1
                        hold[j][e][0] = hold[j][e][1]; hold[j][e][1] = hold[j][e][2]; hold[j][e][2] = hold[j][e][3]; hold[j][e][3] = word;
                    }
                nheld++;
                if ((w & 3) == 3 || last) {
#pragma unroll
                    for (int j = 0; j < NP; j++)
#pragma unroll
                        for (int e = 0; e < 2; e++) {
                            if (ch[j][e] < a.n_channels) {
                                uint32_t *row = (uint32_t *)(a.gring + (uint64_t)ch[j][e] * a.ring_words);
                                if (nheld == 4 && (w & 3) == 3) *(uint4 *)(row + ((w - 3) & mask32)) = make_uint4(hold[j][e][0], hold[j][e][1], hold[j][e][2], hold[j][e][3]);
                                else if (nheld == 2) *(uint2 *)(row + ((w - 1) & mask32)) = make_uint2(hold[j][e][2], hold[j][e][3]);
                                else {                                             // not reached (ranges are multiples of 64 frames); constant register indices
#pragma unroll
                                    for (int k = 0; k < 4; k++)
                                        if (k >= 4 - nheld) row[(w - (uint64_t)(3 - k)) & mask32] = hold[j][e][k];
                                }
                            }
                        }
                    nheld = 0;
                }
            }
        }
    }
};

} // namespace amps
