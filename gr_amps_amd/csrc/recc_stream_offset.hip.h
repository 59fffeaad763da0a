// recc_stream_offset.hip.h -- per-channel carrier offset of the IQ and translate seams (AMPS_RECC_FLAG_STREAM_OFFSET; include/amps_recc.h:
// amps_recc_channel_autocorr / amps_recc_burst_autocorr / amps_recc_burst_offset).
//
// The measurement is the lag-one autocorrelation (pulse-pair) sum of the channel-rate stream capture_run_iq (recc_capture.hip.h) hands
// to the streaming kernel, in the blocks and the numbering of AMPS_RECC_FLAG_STREAM_POWER (recc_stream_power.hip.h):
//     A[c][j] = 2^-8 * sum over s in [256 j, 256 j + 256) of y_c[s] * conj(y_c[s - 1])      (s absolute, amps_recc_set_origin counted;
//                                                                                             y_c[origin - 1] = 0)
// taken by one more read of what the streaming kernel (recc_front_kernel) has just read, by a kernel of its own BEHIND that launch and
// from the same arguments.  Manchester FM is balanced over every bit, so the argument of a burst's sum is 2 pi f / fs, f the offset of
// the mobile's carrier from the channel centre; the ring keeps the complex sums and never an angle: they add correctly across blocks.
//
//   stream_autocorr_kernel       one wave per (block, channel), the four waves of a workgroup on neighbouring channels; no LDS
//   stream_unit_autocorr_kernel  the same body with every product brought to unit amplitude first (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT:
//                                U[c][j] = 2^-8 * sum of p / |p|, the statistic that survives a narrow channel filter); a handle keeps
//                                one ring with one of the two statistics
//   autocorr_ring_gather_kernel  the complex twin of power_ring_gather_kernel: one wave per record, the sum over a capture's blocks
//
// The ring is AutocorrRing below: the BlockRing of recc_block_ring.hip.h with float2 entries ([slots][C], block j in slot j mod slots,
// slots = 64 * ring_words / 256: the slicer-bit ring's window), PowerRule::BLOCK, channel = row and this header's gather kernel.  Create,
// reset, the copy-out of whole rows and the queries by record are that header's, the window recc_ring_window.h's, the launch geometry
// stream_block_launch's (recc_stream_power.hip.h): this header keeps the numeric statement, the kernels and which of the two producers
// is launched.
//
// THE SUMMATION ORDER OF A BLOCK (include/amps_recc.h states it; values are bit-identical however the stream was cut into pushes).
// With a = y[s] and b = y[s - 1], fp32, re and im summed separately and in the same order:
//   re(s)    = fma(a.x, b.x, a.y * b.y)          im(s) = fma(a.y, b.x, -(a.x * b.y))    one rounding in the product, one in the fma
//   lane l   : r_l = ((re(256 j + l) + re(256 j + l + 64)) + re(256 j + l + 128)) + re(256 j + l + 192)        likewise i_l
//   wave     : for o = 32, 16, 8, 4, 2, 1:  r_l = r_l + r_(l xor o)                     every lane ends with the same sum
//   A[c][j]  = (r_0 * 2^-8, i_0 * 2^-8)                                                 exact
// A sample's predecessor is the value of the lane below, or lane 63's value of the quarter before; for the first quarter lane 0 loads
// sample 256 j - 1 itself.  Launch-relative that is i0 - 1 >= -256, inside the carry's halo: after a reset the carry is zeros, which
// is y[origin - 1] = 0.
//
// THE SUMMATION ORDER of a burst sum (autocorr_ring_gather_kernel): that of power_ring_gather_kernel on each component, no division:
//   lane l   : r_l = 0 + re(A[j0 + l]) + re(A[j0 + l + 64]) + ...                       ascending, fp32; likewise i_l
//   wave     : for o = 32, 16, 8, 4, 2, 1:  r_l = r_l + r_(l xor o)
//   sum      = (r_0, i_0), with the count
// A record whose capture is not wholly inside the held window goes to the kernel with count = 0 and comes back {0, 0}, 0.
#pragma once
#include <cmath>
#include "recc_stream_power.hip.h"

namespace amps {

struct StreamAutocorrArgs {
    const float2 *block;     // FrontArgs::block, ::carry, ::ld, ::r_prev, ::n_done, ::n_channels of the launch in front
    const float2 *carry;
    uint64_t ld;
    uint64_t n_done;
    uint32_t r_prev;
    uint32_t n_channels;
    uint64_t first_block;    // floor(n_done / 256): the first block that ends inside the launch
    float2 *ring;            // [slots][n_channels] complex sums, fp32 pairs
    uint32_t slot_mask;      // slots - 1 (a power of two)
    uint32_t groups;         // ceil(n_channels / 4): workgroups per block
};

// AMPS_RECC_FLAG_STREAM_OFFSET_UNIT: a product (re, im) to unit amplitude, in the sequence include/amps_recc.h states.  e = the binary
// exponent of the larger magnitude (frexp: that magnitude = f 2^e, 0.5 <= f < 1); both components times 2^-e, which is exact (a
// component more than 2^100 times smaller than the other may lose bits or vanish below the subnormals: far below u); m = fma(im', im',
// re' re') lies in [0.25, 2), so nothing overflows or underflows whatever |p| was; one v_rsq_f32 (1 ulp); two multiplies.  A product that
// is (0, 0) or has a component that is not finite gives (0, 0).
__device__ __forceinline__ void unit_phasor(float &re, float &im)
{
    const float big = fmaxf(fabsf(re), fabsf(im));                // a NaN in one component leaves the other: the test below sees it
    const bool live = fabsf(re) < INFINITY && fabsf(im) < INFINITY && big > 0.f;
    const int e = __builtin_amdgcn_frexp_expf(big);
    const float sr = __builtin_ldexpf(re, -e), si = __builtin_ldexpf(im, -e);
    const float r = __builtin_amdgcn_rsqf(__builtin_fmaf(si, si, sr * sr));
    re = live ? sr * r : 0.f;
    im = live ? si * r : 0.f;
}

// grid: blocks of the launch x ceil(C / 4), channel groups fastest (one dimension: neither factor is bounded by 65535).
// Launch-relative sample i (absolute n_done + i) is carry[HALO + i] for i < r_prev and block[i - r_prev] from there on
// (recc_front_kernel's `fetch`); the select is made per sample: sample s can be the block's first while s - 1 is the carry's last.
// A block begins at i0 = 256 j - n_done >= -255, its first predecessor is i0 - 1 >= -256 > -HALO, and it ends at i0 + 256 <= P <= avail,
// so every index read exists.
__global__ __launch_bounds__(256) void stream_autocorr_kernel(StreamAutocorrArgs a)
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
    float2 before = make_float2(0.f, 0.f);                        // sample 256 j - 1: lane 0 only
    if (lane == 0) before = i0 - 1 < (int64_t)a.r_prev ? car[i0 - 1] : blk[i0 - 1];
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float2 p = make_float2(__shfl_up(x[k].x, 1), __shfl_up(x[k].y, 1));           // lane l - 1's sample of this quarter
        const int kq = k ? k - 1 : 0;
        const float2 last = k ? make_float2(__shfl(x[kq].x, 63), __shfl(x[kq].y, 63)) : before;
        if (lane == 0) p = last;                                                       // lane 63's sample of the quarter before
        const float tr = __builtin_fmaf(x[k].x, p.x, x[k].y * p.y);
        const float ti = __builtin_fmaf(x[k].y, p.x, -(x[k].x * p.y));
        re = k ? re + tr : tr;
        im = k ? im + ti : ti;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { re += __shfl_xor(re, o); im += __shfl_xor(im, o); }
    if (lane == 0)
        a.ring[(size_t)((uint32_t)j & a.slot_mask) * a.n_channels + c] = make_float2(re * (1.0f / AMPS_RECC_POWER_STRIDE), im * (1.0f / AMPS_RECC_POWER_STRIDE));
}

// The unit-amplitude twin: stream_autocorr_kernel line for line but for unit_phasor on every product.  A kernel of its own and not the
// same body behind a template switch: with the body shared, the compiler scheduled stream_autocorr_kernel's scalar loads in another
// order, and that kernel has to stay instruction for instruction what it was (profiles/stream_offset_unit/isa_identity.txt).
__global__ __launch_bounds__(256) void stream_unit_autocorr_kernel(StreamAutocorrArgs a)
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
    float2 before = make_float2(0.f, 0.f);                        // sample 256 j - 1: lane 0 only
    if (lane == 0) before = i0 - 1 < (int64_t)a.r_prev ? car[i0 - 1] : blk[i0 - 1];
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float2 p = make_float2(__shfl_up(x[k].x, 1), __shfl_up(x[k].y, 1));           // lane l - 1's sample of this quarter
        const int kq = k ? k - 1 : 0;
        const float2 last = k ? make_float2(__shfl(x[kq].x, 63), __shfl(x[kq].y, 63)) : before;
        if (lane == 0) p = last;                                                       // lane 63's sample of the quarter before
        float tr = __builtin_fmaf(x[k].x, p.x, x[k].y * p.y);
        float ti = __builtin_fmaf(x[k].y, p.x, -(x[k].x * p.y));
        unit_phasor(tr, ti);
        re = k ? re + tr : tr;
        im = k ? im + ti : ti;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { re += __shfl_xor(re, o); im += __shfl_xor(im, o); }
    if (lane == 0)
        a.ring[(size_t)((uint32_t)j & a.slot_mask) * a.n_channels + c] = make_float2(re * (1.0f / AMPS_RECC_POWER_STRIDE), im * (1.0f / AMPS_RECC_POWER_STRIDE));
}

// Burst sums: record i asks for `count` entries of ring row `row` from entry j0 on (the host has found them held; count = 0: one of
// them is not); the answer is {re, im, count}.  The summation order is stated at the top of this file.
struct AutocorrBurstSum { float re, im; uint32_t count; };
__global__ __launch_bounds__(256) void autocorr_ring_gather_kernel(const float2 *ring, uint32_t n_channels, uint32_t slot_mask, const PowerBurstQuery *q,
                                                                   uint32_t n, AutocorrBurstSum *out)
{
    const uint32_t rec = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (rec >= n) return;                                         // wave-uniform
    const uint64_t j0 = q[rec].j0;
    const uint32_t row = q[rec].row, count = q[rec].count;
    float re = 0.f, im = 0.f;
    for (uint32_t k = lane; k < count; k += 64u) {
        const float2 e = ring[(size_t)((uint32_t)(j0 + k) & slot_mask) * n_channels + row];
        re += e.x; im += e.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { re += __shfl_xor(re, o); im += __shfl_xor(im, o); }
    if (lane == 0) out[rec] = AutocorrBurstSum{ re, im, count };  // count = 0: nothing was added to the zeros
}

// ---- host side ----
// the handle's carrier-offset ring: created under PowerRule::BLOCK with channel = row, `unit` says which statistic it keeps
typedef BlockRing<float2, AutocorrBurstSum, autocorr_ring_gather_kernel> AutocorrRing;

// behind the streaming-kernel launch `fa` of capture_run_iq: the ring's one producer
inline void stream_autocorr_launch(const AutocorrRing &p, const FrontArgs &fa, hipStream_t s)
{
    stream_block_launch(p.unit ? stream_unit_autocorr_kernel : stream_autocorr_kernel, p, fa, s);
}

// amps_recc_burst_offset: the argument of a burst sum as a frequency, fs = 20000 * samples per symbol; in double, rounded to float
// once.  Nothing held, or a sum of exactly zero: 0.0f
inline float autocorr_offset_hz(float re, float im, uint32_t count, uint32_t sps)
{
    if (count == 0 || (re == 0.f && im == 0.f)) return 0.0f;
    return (float)(std::atan2((double)im, (double)re) * (20000.0 * (double)sps) / (2.0 * 3.14159265358979323846));
}

} // namespace amps
