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
//   stream_power_gather_kernel   one wave per record: the mean of the blocks inside the record's capture
//
// THE SUMMATION ORDER (include/amps_recc.h states it; values are bit-identical however the stream was cut into pushes):
//   term(s)  = fma(im, im, re * re)                                                  fp32, one rounding in the product, one in the fma
//   lane l   : a_l = ((term(256 j + l) + term(256 j + l + 64)) + term(256 j + l + 128)) + term(256 j + l + 192)
//   wave     : for o = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_(l xor o)                  every lane ends with the same sum
//   P[c][j]  = a_0 * 2^-8                                                            exact
// The ring keeps R / 256 blocks per channel, R = 64 * ring_words the span of the slicer-bit ring: both rings hold the same window.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "recc_devmem.hip.h"
#include "recc_front.hip.h"

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

// Burst power: record i asks for `count` blocks of ring row `row` from block j0 on (the host has found them held; count = 0: one of
// them is not); the answer is {mean as float bits, count}.  Lane l sums the blocks j0 + l, j0 + l + 64, ... ascending, then the xor
// butterfly 32 ... 1, then one division.
struct StreamBurstQuery { uint64_t j0; uint32_t row, count; };
__global__ __launch_bounds__(256) void stream_power_gather_kernel(const float *ring, uint32_t n_channels, uint32_t slot_mask, const StreamBurstQuery *q,
                                                                  uint32_t n, uint2 *out)
{
    const uint32_t rec = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (rec >= n) return;                                         // wave-uniform
    const uint64_t j0 = q[rec].j0;
    const uint32_t row = q[rec].row, count = q[rec].count;
    float sum = 0.f;
    for (uint32_t k = lane; k < count; k += 64u) sum += ring[(size_t)((uint32_t)(j0 + k) & slot_mask) * n_channels + row];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) out[rec] = make_uint2(count ? __float_as_uint(sum / (float)count) : 0u, count);
}

// ---- host side ----
struct StreamPowerState {
    DevBuf<float> ring;                       // [slots][C]; null: the handle was created without AMPS_RECC_FLAG_STREAM_POWER
    uint32_t slots = 0, C = 0;
    DevBuf<StreamBurstQuery> pq_dev;          // amps_recc_burst_power scratch (grow-only)
    DevBuf<uint2> pq_out;
};

// ring_words: of the slicer-bit ring, whose window the power ring shares (a power of two, >= 32)
inline int stream_power_create(StreamPowerState &p, uint32_t C, uint32_t ring_words)
{
    p.slots = 64u * ring_words / AMPS_RECC_POWER_STRIDE;
    p.C = C;
    return p.ring.alloc((size_t)p.slots * C);
}

// with the seam (capture_reset puts n_done back to 0, which empties the window; the ring's floats are cleared for tidiness)
inline int stream_power_reset(StreamPowerState &p, hipStream_t s)
{
    if (!p.ring) return 0;
    HIP_TRY(hipMemsetAsync(p.ring.get(), 0, sizeof(float) * (size_t)p.slots * p.C, s));
    return 0;
}

// behind the streaming-kernel launch `fa` of capture_run_iq (fa.P > 0): the blocks j with n_done < 256 (j + 1) <= n_done + P, if any
inline void stream_power_launch(const StreamPowerState &p, const FrontArgs &fa, hipStream_t s)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    const uint64_t first = fa.n_done / S, nblk = (fa.n_done + fa.P) / S - first;
    if (nblk == 0) return;                                        // e.g. a 64-sample launch that ends at s = 128 mod 256
    const uint32_t groups = (fa.n_channels + 3) / 4;
    const StreamPowerArgs a{ fa.block, fa.carry, fa.ld, fa.n_done, fa.r_prev, fa.n_channels, first, p.ring.get(), p.slots - 1, groups };
    hipLaunchKernelGGL(stream_power_kernel, dim3((uint32_t)(nblk * groups)), dim3(256), 0, s, a);
}

// the blocks the ring holds once the stream is idle at n_done: [lo, hi), hi = one past the newest (block j exists iff 256 (j + 1) <= n_done)
inline void stream_power_window(const StreamPowerState &p, uint64_t n_done, uint64_t origin, uint64_t *lo, uint64_t *hi)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    *hi = n_done / S;
    *lo = std::max<uint64_t>((origin + S - 1) / S, *hi > p.slots ? *hi - p.slots : 0);
    if (*lo > *hi) *lo = *hi;                                     // nothing yet: a stream that has not reached its first whole block
}

// amps_recc_channel_power on an idle stream at position n_done
inline int stream_power_channels(const StreamPowerState &p, uint64_t n_done, uint64_t origin, hipStream_t s, uint64_t first_snap, size_t n, float *out,
                                 size_t out_ld, uint32_t *rows, uint64_t *produced_snaps)
{
    uint64_t lo, hi;
    stream_power_window(p, n_done, origin, &lo, &hi);
    if (rows) *rows = p.C;
    if (produced_snaps) *produced_snaps = hi;
    if (n == 0) return 0;
    if (first_snap < lo || first_snap > hi || n > hi - first_snap) return -ERANGE;
    // the ring is block-major: n slots (two runs where the range wraps) to the host, transposed there
    const size_t C = p.C, s0 = (size_t)(first_snap & (p.slots - 1)), n1 = std::min<size_t>(n, p.slots - s0);
    std::vector<float> snap(n * C);
    HIP_TRY(hipMemcpyAsync(snap.data(), p.ring.get() + s0 * C, sizeof(float) * n1 * C, hipMemcpyDeviceToHost, s));
    if (n > n1) HIP_TRY(hipMemcpyAsync(snap.data() + n1 * C, p.ring.get(), sizeof(float) * (n - n1) * C, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t c = 0; c < C; c++)
        for (size_t i = 0; i < n; i++) out[c * out_ld + i] = snap[i * C + c];
    return 0;
}

// amps_recc_burst_power: -EINVAL for a foreign channel comes before any wait; idle() makes the device current and waits for the
// stream; span = samples of a capture.  The blocks wholly inside [position, position + span) are j0 = ceil(position / 256) ...
// j1 = floor((position + span) / 256) - 1; a record with one of them outside the held window gets count 0.
template <class Idle> int stream_power_bursts(StreamPowerState &p, uint64_t n_done, uint64_t origin, uint32_t span, hipStream_t s, Idle &&idle,
                                              const amps_recc_burst_t *recs, size_t n, float *mean_power, uint32_t *n_snaps)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    for (size_t i = 0; i < n; i++) if (recs[i].channel >= p.C) return -EINVAL;
    if (int rc = idle()) return rc;
    if (p.pq_dev.reserve(n) || p.pq_out.reserve(n)) return -ENOMEM;
    uint64_t lo, hi;
    stream_power_window(p, n_done, origin, &lo, &hi);
    std::vector<StreamBurstQuery> q(n);
    for (size_t i = 0; i < n; i++) {
        const uint64_t pos = recs[i].position, j0 = (pos + S - 1) / S, j1 = (pos + span) / S;          // blocks [j0, j1)
        const bool held = j1 > j0 && j0 >= lo && j1 <= hi;
        q[i] = StreamBurstQuery{ j0, recs[i].channel, held ? (uint32_t)(j1 - j0) : 0u };
    }
    HIP_TRY(hipMemcpy(p.pq_dev.get(), q.data(), sizeof(StreamBurstQuery) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(stream_power_gather_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, p.ring.get(), p.C, p.slots - 1, p.pq_dev.get(),
                       (uint32_t)n, p.pq_out.get());
    HIP_TRY(hipGetLastError());
    std::vector<uint2> res(n);
    HIP_TRY(hipMemcpyAsync(res.data(), p.pq_out.get(), sizeof(uint2) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) { std::memcpy(&mean_power[i], &res[i].x, sizeof(float)); n_snaps[i] = res[i].y; }
    return 0;
}

} // namespace amps
