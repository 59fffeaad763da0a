// recc_stream_power.hip.h -- per-channel received power of the IQ and translate seams (AMPS_RECC_FLAG_STREAM_POWER; include/amps_recc.h:
// amps_recc_channel_power / amps_recc_burst_power on a handle without a filter bank).
//
// Every IQ-side seam ends in capture_run_iq (recc_capture.hip.h) with the channel-rate stream in device memory for the length of the
// push: the caller's [C][ld] block, its staged copy, or the translate stage's output.  So the power of a channel is a true block mean:
//     P[c][j] = 2^-8 * sum over s in [256 j, 256 j + 256) of |y_c[s]|^2          (s absolute, amps_recc_set_origin counted)
// taken by one more read of what the streaming kernel (recc_front_kernel) has just read, by a kernel of its own BEHIND that launch and
// from the same arguments.  A launch processes P samples, a multiple of 64 and not of 256, so a block usually begins up to 192 samples
// before the launch: those are in the carry the streaming kernel READS (the last 1024 samples and the unprocessed remainder), which is
// intact until the host swaps the two carry buffers after the push's last launch.  The ring is the only state.
//
//   stream_power_kernel          one wave per (block, channel), the four waves of a workgroup on neighbouring channels; no LDS
//
// The ring and the queries are recc_block_ring.hip.h, its window recc_ring_window.h: this header is the power ring's producer on the IQ
// and translate seams, and holds the one launch behind the streaming kernel (stream_block_launch) that the carrier-offset kernels of
// recc_stream_offset.hip.h share.
//
// THE SUMMATION ORDER OF A BLOCK (include/amps_recc.h states it; values are bit-identical however the stream was cut into pushes):
//   term(s)  = fma(im, im, re * re)                                                  fp32, one rounding in the product, one in the fma
//   lane l   : a_l = ((term(256 j + l) + term(256 j + l + 64)) + term(256 j + l + 128)) + term(256 j + l + 192)
//   wave     : for o = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_(l xor o)                  every lane ends with the same sum
//   P[c][j]  = a_0 * 2^-8                                                            exact
// The ring keeps R / 256 blocks per channel, R = 64 * ring_words the span of the slicer-bit ring: both rings hold the same window.
#pragma once
#include "recc_front.hip.h"
#include "recc_block_ring.hip.h"

namespace amps {

struct StreamPowerArgs {
    const float2 *block;     // FrontArgs::block, ::carry, ::ld, ::r_prev, ::n_done, ::n_channels of the launch in front
    const float2 *carry;
    uint64_t ld;
    uint64_t n_done;
    uint32_t r_prev;
    uint32_t n_channels;
    uint64_t first_block;    // floor(n_done / 256): the first block that ends inside the launch
    float *ring;             // [slots][n_channels] linear power, fp32
    uint32_t slot_mask;      // slots - 1 (a power of two)
    uint32_t groups;         // ceil(n_channels / 4): workgroups per block
};

// grid: blocks of the launch x ceil(C / 4), channel groups fastest (one dimension: neither factor is bounded by 65535).
// Launch-relative sample i (absolute n_done + i) is carry[HALO + i] for i < r_prev and block[i - r_prev] from there on
// (recc_front_kernel's `fetch`); a block begins at i0 = 256 j - n_done >= -255 > -HALO and ends at i0 + 256 <= P <= avail, so every
// index read exists.
__global__ __launch_bounds__(256) void stream_power_kernel(StreamPowerArgs a)
{
    const uint32_t b = blockIdx.x / a.groups, g = blockIdx.x - b * a.groups;
    const uint32_t c = g * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= a.n_channels) return;                                // wave-uniform
    const uint64_t j = a.first_block + b;
    const int64_t i0 = (int64_t)(j * AMPS_RECC_POWER_STRIDE) - (int64_t)a.n_done + lane;
    const float2 *car = a.carry + (uint64_t)c * CARRY_CAP + HALO;
    const float2 *blk = a.block + (uint64_t)c * a.ld - a.r_prev;
    float2 x[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {                                 // four independent loads, consecutive lanes on consecutive samples
        const int64_t i = i0 + 64 * k;
        x[k] = i < (int64_t)a.r_prev ? car[i] : blk[i];
    }
    float acc = __builtin_fmaf(x[0].y, x[0].y, x[0].x * x[0].x);
#pragma unroll
    for (int k = 1; k < 4; k++) acc += __builtin_fmaf(x[k].y, x[k].y, x[k].x * x[k].x);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) a.ring[(size_t)((uint32_t)j & a.slot_mask) * a.n_channels + c] = acc * (1.0f / AMPS_RECC_POWER_STRIDE);
}

// The one launch of the block kernels (this header's and the two of recc_stream_offset.hip.h), each with its own argument struct of
// the members above: behind the streaming-kernel launch `fa` of capture_run_iq (fa.P > 0), the blocks j with
// n_done < 256 (j + 1) <= n_done + P, if any, into ring p
template <class Args, class Ring> void stream_block_launch(void (*kernel)(Args), const Ring &p, const FrontArgs &fa, hipStream_t s)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    const uint64_t first = fa.n_done / S, nblk = (fa.n_done + fa.P) / S - first;
    if (nblk == 0) return;                                        // e.g. a 64-sample launch that ends at s = 128 mod 256
    const uint32_t groups = (fa.n_channels + 3) / 4;
    const Args a{ fa.block, fa.carry, fa.ld, fa.n_done, fa.r_prev, fa.n_channels, first, p.ring.get(), p.slots - 1, groups };
    hipLaunchKernelGGL(kernel, dim3((uint32_t)(nblk * groups)), dim3(256), 0, s, a);
}
inline void stream_power_launch(const PowerRing &p, const FrontArgs &fa, hipStream_t s) { stream_block_launch(stream_power_kernel, p, fa, s); }

} // namespace amps
