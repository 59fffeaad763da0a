// recc_power_ring.hip.h -- the one power ring of a handle and the two queries behind amps_recc_channel_power / amps_recc_burst_power.
//
// A handle keeps received power under one of two flags, never both (amps_recc_create), and each flag has one PRODUCER that fills the ring:
//   AMPS_RECC_FLAG_CHANNEL_POWER   wideband seam: chz_power_kernel (recc_power.hip.h), a SNAPSHOT |Y_k|^2 of the frame at every sample
//                                  s = 256 j
//   AMPS_RECC_FLAG_STREAM_POWER    IQ and translate seams: stream_power_kernel (recc_stream_power.hip.h), the mean of |y|^2 over the
//                                  BLOCK of samples [256 j, 256 j + 256)
// Everything behind the producer is here, once: the ring ([slots][rows] fp32, entry j in slot j mod slots; R / 256 entries per row,
// R = 64 * ring_words the span of the slicer-bit ring, so both rings hold the same window), its reset, which entries exist and which
// of them a capture takes (PowerRule: the only place where the two producers differ), the copy-out of whole rows, and the mean over a
// capture.
//
// THE SUMMATION ORDER of a burst mean (power_ring_gather_kernel; the values of both flags come from it): of the `count` entries
// j0 ... j0 + count - 1 of one row
//   lane l   : a_l = 0 + e(j0 + l) + e(j0 + l + 64) + ...                ascending, fp32
//   wave     : for o = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_(l xor o)      every lane ends with the same sum
//   mean     = a_0 / (float)count                                         one division, correctly rounded
// A record whose capture is not wholly inside the held window goes to the kernel with count = 0 and comes back {0, 0}.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <vector>
#include "amps_recc.h"
#include "recc_devmem.hip.h"

namespace amps {

// which entries exist and which belong to a capture.  One "entry width" does not say both: a snapshot AT sample position + span still
// counts, a block must END at or before it.
enum class PowerRule { SNAPSHOT, BLOCK };

struct PowerWindow { uint64_t lo, hi; };          // entries [lo, hi) are held, hi = one past the newest
struct PowerRange { uint64_t j0; uint32_t count; };   // entries j0 ... j0 + count - 1; count = 0: not (all) held

// the entries the ring holds once the stream is idle at n_done: snapshot j exists iff 256 j < n_done, block j iff 256 (j + 1) <= n_done;
// nothing from before the origin, and no more than `slots`
constexpr PowerWindow power_ring_window(PowerRule rule, uint32_t slots, uint64_t n_done, uint64_t origin)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    const uint64_t hi = rule == PowerRule::SNAPSHOT ? (n_done + S - 1) / S : n_done / S;
    uint64_t lo = std::max<uint64_t>((origin + S - 1) / S, hi > slots ? hi - slots : 0);
    if (lo > hi) lo = hi;                         // nothing yet: a stream that has not reached its first whole block (never a snapshot stream: origin <= n_done)
    return PowerWindow{ lo, hi };
}

// the entries inside a capture of `span` samples at `position`: the snapshots j with position <= 256 j <= position + span, the blocks
// wholly inside [position, position + span); count = 0 unless every one of them is inside the window
constexpr PowerRange power_ring_range(PowerRule rule, uint64_t position, uint32_t span, PowerWindow w)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    const uint64_t j0 = (position + S - 1) / S, j1 = (position + span) / S;
    if (rule == PowerRule::SNAPSHOT) {            // snapshots [j0, j1]
        const bool held = j1 >= j0 && j0 >= w.lo && j1 < w.hi;
        return PowerRange{ j0, held ? (uint32_t)(j1 - j0 + 1) : 0u };
    }
    const bool held = j1 > j0 && j0 >= w.lo && j1 <= w.hi;   // blocks [j0, j1)
    return PowerRange{ j0, held ? (uint32_t)(j1 - j0) : 0u };
}

// the documented counts (include/amps_recc.h): a capture is AMPS_RECC_CAPTURE_SYMS symbols
namespace power_ring_check {
constexpr PowerWindow ALL{ 0, 1u << 20 };
constexpr uint32_t count(PowerRule r, uint64_t pos, uint32_t sps) { return power_ring_range(r, pos, (uint32_t)AMPS_RECC_CAPTURE_SYMS * sps, ALL).count; }
static_assert(count(PowerRule::SNAPSHOT, 512, 2) == 27 && count(PowerRule::SNAPSHOT, 513, 2) == 26, "snapshots at 2 samples per symbol");
static_assert(count(PowerRule::SNAPSHOT, 512, 3) == 40 && count(PowerRule::SNAPSHOT, 513, 3) == 39, "snapshots at 3 samples per symbol");
static_assert(count(PowerRule::BLOCK, 512, 10) == 131 && count(PowerRule::BLOCK, 513, 10) == 130, "blocks at 10 samples per symbol");
static_assert(count(PowerRule::BLOCK, 512, 12) == 158 && count(PowerRule::BLOCK, 513, 12) == 157, "blocks at 12 samples per symbol");
static_assert(power_ring_range(PowerRule::SNAPSHOT, 512, 6748, ALL).j0 == 2 && power_ring_range(PowerRule::BLOCK, 513, 33740, ALL).j0 == 3, "first entry");
} // namespace power_ring_check

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
struct PowerRing {
    DevBuf<float> ring;                       // [slots][rows] linear power; null: the handle was created without either flag
    uint32_t slots = 0, rows = 0;             // slots: a power of two
    PowerRule rule = PowerRule::SNAPSHOT;
    std::vector<int32_t> chan2row;            // a record's channel number -> ring row, -1 for a channel this handle does not decode
                                              // (wideband seam: from row2chan); empty: channel = row (IQ and translate seams)
    DevBuf<PowerBurstQuery> pq_dev;           // amps_recc_burst_power scratch (grow-only)
    DevBuf<uint2> pq_out;
};

// ring_words: of the slicer-bit ring, whose window the power ring shares (a power of two, >= 32); row2chan: of a wideband handle,
// its channel numbers out of n_channels, else null
inline int power_ring_create(PowerRing &p, PowerRule rule, uint32_t rows, uint32_t ring_words, const std::vector<uint32_t> *row2chan = nullptr,
                             uint32_t n_channels = 0)
{
    p.rule = rule;
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
inline int power_ring_reset(PowerRing &p, hipStream_t s)
{
    if (!p.ring) return 0;
    HIP_TRY(hipMemsetAsync(p.ring.get(), 0, sizeof(float) * (size_t)p.slots * p.rows, s));
    return 0;
}

// amps_recc_channel_power on an idle stream at position n_done
inline int power_ring_channels(const PowerRing &p, uint64_t n_done, uint64_t origin, hipStream_t s, uint64_t first_snap, size_t n, float *out,
                               size_t out_ld, uint32_t *rows, uint64_t *produced_snaps)
{
    const PowerWindow w = power_ring_window(p.rule, p.slots, n_done, origin);
    if (rows) *rows = p.rows;
    if (produced_snaps) *produced_snaps = w.hi;
    if (n == 0) return 0;
    if (first_snap < w.lo || first_snap > w.hi || n > w.hi - first_snap) return -ERANGE;
    // the ring is entry-major: n slots (two runs where the range wraps) to the host, transposed there
    const size_t C = p.rows, s0 = (size_t)(first_snap & (p.slots - 1)), n1 = std::min<size_t>(n, p.slots - s0);
    std::vector<float> snap(n * C);
    HIP_TRY(hipMemcpyAsync(snap.data(), p.ring.get() + s0 * C, sizeof(float) * n1 * C, hipMemcpyDeviceToHost, s));
    if (n > n1) HIP_TRY(hipMemcpyAsync(snap.data() + n1 * C, p.ring.get(), sizeof(float) * (n - n1) * C, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t c = 0; c < C; c++)
        for (size_t i = 0; i < n; i++) out[c * out_ld + i] = snap[i * C + c];
    return 0;
}

// amps_recc_burst_power: -EINVAL for a foreign channel comes before any wait; idle() makes the device current and waits for the
// stream (the window is that of an idle stream; the copies below are synchronous); span = samples of a capture
template <class Idle> int power_ring_bursts(PowerRing &p, uint64_t n_done, uint64_t origin, uint32_t span, hipStream_t s, Idle &&idle,
                                            const amps_recc_burst_t *recs, size_t n, float *mean_power, uint32_t *n_snaps)
{
    std::vector<PowerBurstQuery> q(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t ch = recs[i].channel;
        if (p.chan2row.empty() ? ch >= p.rows : (ch >= p.chan2row.size() || p.chan2row[ch] < 0)) return -EINVAL;
        q[i].row = p.chan2row.empty() ? ch : (uint32_t)p.chan2row[ch];
    }
    if (int rc = idle()) return rc;
    if (p.pq_dev.reserve(n) || p.pq_out.reserve(n)) return -ENOMEM;
    const PowerWindow w = power_ring_window(p.rule, p.slots, n_done, origin);
    for (size_t i = 0; i < n; i++) {
        const PowerRange r = power_ring_range(p.rule, recs[i].position, span, w);
        q[i].j0 = r.j0; q[i].count = r.count;
    }
    HIP_TRY(hipMemcpy(p.pq_dev.get(), q.data(), sizeof(PowerBurstQuery) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(power_ring_gather_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, p.ring.get(), p.rows, p.slots - 1, p.pq_dev.get(),
                       (uint32_t)n, p.pq_out.get());
    HIP_TRY(hipGetLastError());
    std::vector<uint2> res(n);
    HIP_TRY(hipMemcpyAsync(res.data(), p.pq_out.get(), sizeof(uint2) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) { std::memcpy(&mean_power[i], &res[i].x, sizeof(float)); n_snaps[i] = res[i].y; }
    return 0;
}

} // namespace amps
