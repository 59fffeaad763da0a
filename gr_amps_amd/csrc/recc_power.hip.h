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
//   chz_power_gather_kernel    one wave per record: the mean of the snapshots inside the record's capture
//
// The ring keeps R / 256 snapshots per row, R = 64 * ring_words the span of the slicer-bit ring: both rings hold the same window.
#pragma once
#include "recc_channelizer.hip.h"

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

// behind the filter-bank launch `a` of channelizer_run (fused form, z.pow_ring set): the snapshot frames of that launch, if it has any
inline void chz_power_launch(const ChannelizerState &z, const ChzArgs &a, bool sc16, hipStream_t s)
{
    const uint32_t first = (uint32_t)((0ull - a.n_done) & (uint64_t)(AMPS_RECC_POWER_STRIDE - 1));
    if (first >= a.nframes) return;                               // e.g. a 64-frame launch that covers s in [64, 128)
    const uint32_t nsnap = (a.nframes - first + AMPS_RECC_POWER_STRIDE - 1) / AMPS_RECC_POWER_STRIDE;
    ChzPowerArgs p{ z.pow_ring.get(), z.pow_slots - 1, first };
    hipLaunchKernelGGL(chz_power_kernel_for(z.D, sc16), dim3(nsnap), dim3(256), 0, s, a, p);
}

// Burst power: record i asks for the snapshots j with position <= 256 j <= position + span of ring row `row`; the answer is
// {mean as float bits, count}, or {0, 0} when one of them lies outside the held window [snap_lo, snap_hi).
struct ChzBurstQuery { uint64_t position; uint32_t row, _pad; };
__global__ __launch_bounds__(256) void chz_power_gather_kernel(const float *ring, uint32_t n_channels, uint32_t slot_mask, uint64_t snap_lo,
                                                               uint64_t snap_hi, uint32_t span, const ChzBurstQuery *q, uint32_t n, uint2 *out)
{
    const uint32_t rec = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (rec >= n) return;                                         // wave-uniform
    const uint64_t pos = q[rec].position;
    const uint64_t j0 = (pos + AMPS_RECC_POWER_STRIDE - 1) / AMPS_RECC_POWER_STRIDE, j1 = (pos + span) / AMPS_RECC_POWER_STRIDE;
    const bool held = j1 >= j0 && j0 >= snap_lo && j1 < snap_hi;
    const uint32_t count = held ? (uint32_t)(j1 - j0 + 1) : 0u;
    float sum = 0.f;
    for (uint32_t k = lane; k < count; k += 64u) sum += ring[(size_t)((uint32_t)(j0 + k) & slot_mask) * n_channels + q[rec].row];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) out[rec] = make_uint2(count ? __float_as_uint(sum / (float)count) : 0u, count);
}

// ---- host side: the queries behind amps_recc_channel_power / amps_recc_burst_power.  The ring itself is z.pow_ring: the filter
// bank's launches fill it. ----
struct PowerState {
    std::vector<int32_t> chan2row;            // whole-band channel number -> ring row, -1 for a channel this handle does not decode
    DevBuf<ChzBurstQuery> pq_dev;             // amps_recc_burst_power scratch (grow-only)
    DevBuf<uint2> pq_out;
};

// ring_words: of the slicer-bit ring, whose window the power ring shares (a power of two, >= 32)
inline int power_create(PowerState &p, ChannelizerState &z, uint32_t n_channels, uint32_t ring_words)
{
    z.pow_slots = 64u * ring_words / AMPS_RECC_POWER_STRIDE;
    p.chan2row.assign(n_channels, -1);
    for (size_t r = 0; r < z.row2chan.size(); r++) p.chan2row[z.row2chan[r]] = (int32_t)r;
    return z.pow_ring.alloc((size_t)z.pow_slots * z.C);
}

// the snapshots the power ring holds once the stream is idle: [lo, hi), hi = one past the newest (snapshot j exists iff 256 j < n_done)
inline void power_window(const ChannelizerState &z, uint64_t n_done, uint64_t origin, uint64_t *lo, uint64_t *hi)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    *hi = (n_done + S - 1) / S;
    *lo = std::max<uint64_t>((origin + S - 1) / S, *hi > z.pow_slots ? *hi - z.pow_slots : 0);
}

// amps_recc_channel_power on an idle stream at position n_done
inline int power_channels(const ChannelizerState &z, uint64_t n_done, uint64_t origin, hipStream_t s, uint64_t first_snap, size_t n, float *out,
                          size_t out_ld, uint32_t *rows, uint64_t *produced_snaps)
{
    uint64_t lo, hi;
    power_window(z, n_done, origin, &lo, &hi);
    if (rows) *rows = z.C;
    if (produced_snaps) *produced_snaps = hi;
    if (n == 0) return 0;
    if (first_snap < lo || first_snap > hi || n > hi - first_snap) return -ERANGE;
    // the ring is snapshot-major: n slots (two runs where the range wraps) to the host, transposed there
    const uint32_t slots = z.pow_slots;
    const size_t C = z.C, s0 = (size_t)(first_snap & (slots - 1)), n1 = std::min<size_t>(n, slots - s0);
    std::vector<float> snap(n * C);
    HIP_TRY(hipMemcpyAsync(snap.data(), z.pow_ring.get() + s0 * C, sizeof(float) * n1 * C, hipMemcpyDeviceToHost, s));
    if (n > n1) HIP_TRY(hipMemcpyAsync(snap.data() + n1 * C, z.pow_ring.get(), sizeof(float) * (n - n1) * C, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t c = 0; c < C; c++)
        for (size_t i = 0; i < n; i++) out[c * out_ld + i] = snap[i * C + c];
    return 0;
}

// amps_recc_burst_power: idle() makes the device current and waits for the stream (the window is that of an idle stream; the copies
// below are synchronous) once the records have been found to name channels of this handle, which keeps the entry point's order of
// answers: -EINVAL for a foreign channel comes before any wait; span = samples of a capture
template <class Idle> int power_bursts(PowerState &p, const ChannelizerState &z, uint64_t n_done, uint64_t origin, uint32_t span, hipStream_t s, Idle &&idle,
                                       const amps_recc_burst_t *recs, size_t n, float *mean_power, uint32_t *n_snaps)
{
    std::vector<ChzBurstQuery> q(n);
    for (size_t i = 0; i < n; i++) {
        if (recs[i].channel >= p.chan2row.size() || p.chan2row[recs[i].channel] < 0) return -EINVAL;
        q[i] = ChzBurstQuery{ recs[i].position, (uint32_t)p.chan2row[recs[i].channel], 0u };
    }
    if (int rc = idle()) return rc;
    if (p.pq_dev.reserve(n) || p.pq_out.reserve(n)) return -ENOMEM;
    uint64_t lo, hi;
    power_window(z, n_done, origin, &lo, &hi);
    HIP_TRY(hipMemcpy(p.pq_dev.get(), q.data(), sizeof(ChzBurstQuery) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(chz_power_gather_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, z.pow_ring.get(), z.C, z.pow_slots - 1, lo, hi,
                       span, p.pq_dev.get(), (uint32_t)n, p.pq_out.get());
    HIP_TRY(hipGetLastError());
    std::vector<uint2> res(n);
    HIP_TRY(hipMemcpyAsync(res.data(), p.pq_out.get(), sizeof(uint2) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) { std::memcpy(&mean_power[i], &res[i].x, sizeof(float)); n_snaps[i] = res[i].y; }
    return 0;
}

} // namespace amps
