// recc_block_ring.hip.h -- the one ring type behind the per-block statistics of a handle and its two queries: whole rows
// (amps_recc_channel_power / amps_recc_channel_autocorr) and the sum or mean over a record's capture (amps_recc_burst_power /
// amps_recc_burst_autocorr).
//
// A ring is [slots][rows] entries, entry j in slot j mod slots; R / 256 entries per row, R = 64 * ring_words the span of the slicer-bit
// ring, so every ring of a handle holds the same window.  BlockRing is parameterised by the entry, by what a query by record answers
// and by the gather kernel that computes it; a handle keeps up to two:
//   PowerRing (below)                           float entries, power_ring_gather_kernel.  Received power under one of two flags, never
//                                               both (amps_recc_create), each with one PRODUCER that fills the ring:
//     AMPS_RECC_FLAG_CHANNEL_POWER              wideband seam: chz_power_kernel (recc_power.hip.h), a SNAPSHOT |Y_k|^2 of the frame at
//                                               every sample s = 256 j; records carry channel numbers, rows by chan2row
//     AMPS_RECC_FLAG_STREAM_POWER               IQ and translate seams: stream_power_kernel (recc_stream_power.hip.h), the mean of |y|^2
//                                               over the BLOCK of samples [256 j, 256 j + 256)
//   AutocorrRing (recc_stream_offset.hip.h)     float2 entries, autocorr_ring_gather_kernel.  Carrier offset of the IQ and translate
//                                               seams: blocks, channel = row, and one of two producers (`unit`)
// Everything behind the producers is here, once: create, reset, the copy-out of whole rows and the query by record.  Which entries
// exist, which of them a capture takes (PowerRule: the only place where snapshots and blocks differ) and how a range leaves the ring
// is recc_ring_window.h, free of HIP.  Unpacking a query's answers into the caller's arrays stays with the entry points (amps_recc.hip).
//
// THE SUMMATION ORDER of a burst mean (power_ring_gather_kernel; the values of both power flags come from it): of the `count` entries
// j0 ... j0 + count - 1 of one row
//   lane l   : a_l = 0 + e(j0 + l) + e(j0 + l + 64) + ...                ascending, fp32
//   wave     : for o = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_(l xor o)      every lane ends with the same sum
//   mean     = a_0 / (float)count                                         one division, correctly rounded
// A record whose capture is not wholly inside the held window goes to the kernel with count = 0 and comes back {0, 0}.
#pragma once
#include <hip/hip_runtime.h>
#include <cerrno>
#include <vector>
#include "recc_devmem.hip.h"
#include "recc_ring_window.h"

namespace amps {

// Burst power: record i asks for `count` entries of ring row `row` from entry j0 on (the host has found them held; count = 0: one of
// them is not); the answer is {mean as float bits, count}.  The summation order is stated at the top of this file.
struct PowerBurstQuery { uint64_t j0; uint32_t row, count; };
__global__ __launch_bounds__(256) void power_ring_gather_kernel(const float *ring, uint32_t n_channels, uint32_t slot_mask, const PowerBurstQuery *q,
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
// E: an entry, one or more floats; R: a gather kernel's answer for one record; GATHER: that kernel
template <class E, class R, void (*GATHER)(const E *, uint32_t, uint32_t, const PowerBurstQuery *, uint32_t, R *)> struct BlockRing {
    typedef R result_t;
    static constexpr size_t WIDTH = sizeof(E) / sizeof(float);
    static_assert(sizeof(E) == WIDTH * sizeof(float), "an entry is whole floats");
    DevBuf<E> ring;                           // [slots][rows]; null: the handle was created without the ring's flag
    uint32_t slots = 0, rows = 0;             // slots: a power of two
    PowerRule rule = PowerRule::SNAPSHOT;
    bool unit = false;                        // AutocorrRing: the ring's one statistic is U (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT) instead of A
    std::vector<int32_t> chan2row;            // a record's channel number -> ring row, -1 for a channel this handle does not decode
                                              // (wideband seam: from row2chan); empty: channel = row (IQ and translate seams)
    DevBuf<PowerBurstQuery> q_dev;            // block_ring_bursts scratch (grow-only), the ring's own
    DevBuf<R> q_out;
    void gather(size_t n, hipStream_t s) const   // one wave per query of q_dev, n <= 2^32 - 1
    {
        hipLaunchKernelGGL(GATHER, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, ring.get(), rows, slots - 1, q_dev.get(), (uint32_t)n, q_out.get());
    }
};
typedef BlockRing<float, uint2, power_ring_gather_kernel> PowerRing;

// ring_words: of the slicer-bit ring, whose window the ring shares (a power of two, >= 32); row2chan: of a wideband handle,
// its channel numbers out of n_channels, else null
template <class Ring> int block_ring_create(Ring &p, PowerRule rule, uint32_t rows, uint32_t ring_words, bool unit = false,
                                            const std::vector<uint32_t> *row2chan = nullptr, uint32_t n_channels = 0)
{
    p.rule = rule;
    p.unit = unit;
    p.slots = 64u * ring_words / AMPS_RECC_POWER_STRIDE;
    p.rows = rows;
    p.chan2row.clear();
    if (row2chan) {
        p.chan2row.assign(n_channels, -1);
        for (size_t r = 0; r < row2chan->size(); r++) p.chan2row[(*row2chan)[r]] = (int32_t)r;
    }
    return p.ring.alloc((size_t)p.slots * rows);
}

// with the seam (capture_reset puts n_done back to 0, which empties the window; the ring's floats are cleared for tidiness)
template <class Ring> int block_ring_reset(Ring &p, hipStream_t s)
{
    if (!p.ring) return 0;
    HIP_TRY(hipMemsetAsync(p.ring.get(), 0, sizeof(float) * Ring::WIDTH * p.slots * p.rows, s));
    return 0;
}

// amps_recc_channel_power / _channel_autocorr on an idle stream at position n_done: out is [rows][out_ld][WIDTH]
template <class Ring> int block_ring_channels(const Ring &p, uint64_t n_done, uint64_t origin, hipStream_t s, uint64_t first, size_t n, float *out,
                                              size_t out_ld, uint32_t *rows, uint64_t *produced)
{
    const PowerWindow w = power_ring_window(p.rule, p.slots, n_done, origin);
    if (rows) *rows = p.rows;
    if (produced) *produced = w.hi;
    if (n == 0) return 0;
    if (!power_ring_holds(w, first, n)) return -ERANGE;
    // the ring is entry-major: n slots (two runs where the range wraps) to the host, transposed there
    const RingRuns r = ring_runs(first, n, p.slots);
    const size_t ew = (size_t)p.rows * Ring::WIDTH;              // floats of one slot
    std::vector<float> snap(n * ew);
    HIP_TRY(hipMemcpyAsync(snap.data(), p.ring.get() + r.s0 * p.rows, sizeof(float) * r.n1 * ew, hipMemcpyDeviceToHost, s));
    if (n > r.n1) HIP_TRY(hipMemcpyAsync(snap.data() + r.n1 * ew, p.ring.get(), sizeof(float) * (n - r.n1) * ew, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ring_transpose(snap.data(), n, p.rows, Ring::WIDTH, out, out_ld);
    return 0;
}

// amps_recc_burst_power / _burst_autocorr: -EINVAL for a foreign channel comes before any wait; idle() makes the device current and
// waits for the stream (the window is that of an idle stream; the copies below are synchronous); span = samples of a capture; res: the
// gather kernel's answer for each of the n records
template <class Ring, class Idle> int block_ring_bursts(Ring &p, uint64_t n_done, uint64_t origin, uint32_t span, hipStream_t s, Idle &&idle,
                                                        const amps_recc_burst_t *recs, size_t n, std::vector<typename Ring::result_t> &res)
{
    std::vector<PowerBurstQuery> q(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t ch = recs[i].channel;
        if (p.chan2row.empty() ? ch >= p.rows : (ch >= p.chan2row.size() || p.chan2row[ch] < 0)) return -EINVAL;
        q[i].row = p.chan2row.empty() ? ch : (uint32_t)p.chan2row[ch];
    }
    if (int rc = idle()) return rc;
    if (p.q_dev.reserve(n) || p.q_out.reserve(n)) return -ENOMEM;
    const PowerWindow w = power_ring_window(p.rule, p.slots, n_done, origin);
    for (size_t i = 0; i < n; i++) {
        const PowerRange r = power_ring_range(p.rule, recs[i].position, span, w);
        q[i].j0 = r.j0; q[i].count = r.count;
    }
    HIP_TRY(hipMemcpy(p.q_dev.get(), q.data(), sizeof(PowerBurstQuery) * n, hipMemcpyHostToDevice));
    p.gather(n, s);
    HIP_TRY(hipGetLastError());
    res.resize(n);
    HIP_TRY(hipMemcpyAsync(res.data(), p.q_out.get(), sizeof(typename Ring::result_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

} // namespace amps
