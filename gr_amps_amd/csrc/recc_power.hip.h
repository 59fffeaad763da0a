// recc_power.hip.h -- per-channel received power of the wideband seam (AMPS_RECC_FLAG_CHANNEL_POWER; include/amps_recc.h:
// amps_recc_channel_power / amps_recc_burst_power).
//
// The fused filter bank (chz12_kernel) lets nothing but slicer bits leave the CU.  What a receiver also wants to know -- how strong a
// mobile was, which channels carry energy -- needs |Y_k[m]|^2 of a frame now and then, not of every frame: a POWER SNAPSHOT is taken at
// every channel-rate sample index s with s % AMPS_RECC_POWER_STRIDE == 0 (absolute numbering, amps_recc_set_origin counted: the
// numbering of amps_recc_burst_t.position).  One frame in 256 is 0.4 % of the filter bank's arithmetic, so the snapshots are computed
// by a small kernel of their own BEHIND the filter-bank launch, from the same arguments: the block and the carry that launch read are
// still there (the carry buffers swap afterwards) and the carry reaches L - D + 4 D samples back, so every frame of the launch can be
// folded again from scratch.  chz12_kernel is not touched and runs the instructions it always ran.
//
//   chz_power_kernel<T, DEC>   one 256-thread workgroup per snapshot frame: fold (8 taps x 4 branches per thread, every load of the
//                              frame's 32 KB window in flight at once), the radix-4 pass, chz_p2 and chz_p3 in one LDS frame buffer,
//                              then re^2 + im^2 of the handle's bins into the power ring, snapshot-major ([slot][row]: coalesced)
//
// The ring and the queries are recc_block_ring.hip.h, its window recc_ring_window.h: this header is the ring's producer on the wideband seam.
#pragma once
#include "amps_recc.h"
#include "recc_chz_common.hip.h"
#include "recc_chz_fft.hip.h"
#include "recc_chz_fold.hip.h"
#include "recc_block_ring.hip.h"

namespace amps {

struct ChzPowerArgs {
    float *ring;             // [slots][n_channels] linear power, fp32
    uint32_t slot_mask;      // slots - 1 (a power of two)
    uint32_t first_frame;    // launch-relative frame of the launch's first snapshot (a multiple of 64)
};

// Frame F of the launch covers the virtual samples [n0, n0 + L), n0 = (F + 1) D - L; virtual sample 0 is the stream position the launch
// starts at, a multiple of M, so sample v belongs to branch v mod M.  Thread t folds the window elements i = t + 256 j + 1024 q (tap
// h[i]): its four sums are the branches t + 256 ((j + n0 / 256) & 3), and n0 mod M = D mod M for every F that is a multiple of four.
template <typename T, int DEC>
__global__ __launch_bounds__(256) void chz_power_kernel(ChzArgs a, ChzPowerArgs p)
{
    static_assert(DEC == CHZ_D || DEC == CHZ_D768, "input samples per frame");
    constexpr int M = CHZ_M, P = 8, L = P * M;
    constexpr int SH = (DEC / 256) & 3;                           // (n0 mod M) / 256
    __shared__ cf2 buf[CHZ_FB];
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63;
    const int64_t F = (int64_t)p.first_frame + (int64_t)AMPS_RECC_POWER_STRIDE * blockIdx.x;
    const int64_t lead0 = (int64_t)a.carry_len - (int64_t)a.hist;
    const ChzIn<T> in{ (const T *)a.block, a.carry, (int64_t)a.hist, lead0, (int64_t)a.carry_len, (int64_t)a.nsamp };
    const int64_t n0 = (F + 1) * DEC - L;                         // >= -hist: the carry holds it
    // the whole window first: 32 independent loads (64 dwords of an sc16 block), consecutive lanes on consecutive samples
    cf2 x[4][P];
    float h[4][P];
#pragma unroll
    for (int q = 0; q < P; q++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            x[j][q] = in.generic_nb(n0 + t + 256 * j + M * q);
            h[j][q] = a.taps[t + 256 * j + M * q];
        }
    cf2 u[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        cf2 acc = { h[j][0] * x[j][0].x, h[j][0] * x[j][0].y };
#pragma unroll
        for (int q = 1; q < P; q++) { acc.x = __builtin_fmaf(h[j][q], x[j][q].x, acc.x); acc.y = __builtin_fmaf(h[j][q], x[j][q].y, acc.y); }
        u[(j + SH) & 3] = acc;
    }
    // radix-4 pass 1 with pass 2's input twiddles, into the layout chz_p2 reads (chz_fold2_ring)
    {
        cf2 o[4];
        dft4(u[0], u[1], u[2], u[3], o);
        cf2 *d = buf + t;
        d[chz_pos1(0, 0)] = o[0];
#pragma unroll
        for (int k1 = 1; k1 < 4; k1++) d[chz_pos1(0, k1)] = cmul(o[k1], chz_twiddle((t >> 4) * k1, 64));
    }
    __syncthreads();
    // the two radix-16 passes are one frame per wave
    if (wave == 0) chz_p2(buf, lane);
    __syncthreads();
    if (wave == 0) {
        cf2 tw3[15];
#pragma unroll
        for (int r = 1; r < 16; r++) tw3[r - 1] = chz_twiddle(r * lane, 1024);
        chz_p3(buf, tw3, lane);
    }
    __syncthreads();
    // the spectrum lies planar in natural order: bins t + 256 q, rows by bin2row (rows follow the bins: neighbouring lanes, neighbouring floats)
    const float *Af = (const float *)buf;
    const uint64_t snap = (a.n_done + (uint64_t)F) / AMPS_RECC_POWER_STRIDE;
    float *dst = p.ring + (size_t)((uint32_t)snap & p.slot_mask) * a.n_channels;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int bin = t + 256 * q;
        const uint32_t row = a.bin2row[bin];
        const float re = Af[chz_planar(bin)], im = Af[chz_planar(bin) + 128];
        if (row < a.n_channels) dst[row] = __builtin_fmaf(im, im, re * re);
    }
}

typedef void (*chz_power_kernel_t)(ChzArgs, ChzPowerArgs);
inline chz_power_kernel_t chz_power_kernel_for(int D, bool sc16)
{
    if (D == CHZ_D768) return sc16 ? chz_power_kernel<chz_sc16, CHZ_D768> : chz_power_kernel<float2, CHZ_D768>;
    return sc16 ? chz_power_kernel<chz_sc16, CHZ_D> : chz_power_kernel<float2, CHZ_D>;
}

// behind the filter-bank launch `a` of channelizer_run (fused form, D input samples per frame): the snapshot frames of that launch, if it has any
inline void chz_power_launch(const PowerRing &p, int D, const ChzArgs &a, bool sc16, hipStream_t s)
{
    const uint32_t first = (uint32_t)((0ull - a.n_done) & (uint64_t)(AMPS_RECC_POWER_STRIDE - 1));
    if (first >= a.nframes) return;                               // e.g. a 64-frame launch that covers s in [64, 128)
    const uint32_t nsnap = (a.nframes - first + AMPS_RECC_POWER_STRIDE - 1) / AMPS_RECC_POWER_STRIDE;
    ChzPowerArgs pa{ p.ring.get(), p.slots - 1, first };
    hipLaunchKernelGGL(chz_power_kernel_for(D, sc16), dim3(nsnap), dim3(256), 0, s, a, pa);
}

} // namespace amps
