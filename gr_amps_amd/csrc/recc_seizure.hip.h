// recc_seizure.hip.h -- seizure events (AMPS_RECC_FLAG_SEIZURE_EVENTS; the contract stands in include/amps_recc_seizure.h at
// amps_recc_drain_seizures): one event per seizure, after the push in which its trigger was accepted.  The resolve kernel parks an
// accepted trigger whose tail has not arrived in pending[channel] (recc_resolve.hip.h); the kernel here, launched behind every
// resolve, reports each such capture once.  One state: what was reported per channel, the device list with its header, and what a
// drain has taken off the device but not yet handed out.  A handle without the flag has none of it and launches nothing.
#pragma once
#include <vector>
#include "amps_recc_seizure.h"
#include "recc_devmem.hip.h"

namespace amps {

static_assert(sizeof(amps_recc_seizure_t) == AMPS_RECC_SEIZURE_BYTES && AMPS_RECC_SEIZURE_BYTES == 32, "event layout is part of the ABI");

constexpr int SEIZURE_THREADS = 256;       // channels per tile of the ordered scan
constexpr int SEIZURE_DCC_SYMS = 14;       // the coded DCC: 7 bits, 2 Manchester symbols each

struct SeizureArgs {
    const uint64_t *pending;   // [C], ~0 = none: what the resolve of this push left (read only)
    uint64_t *reported;        // [C], ~0 = none: the capture last reported for the channel
    const uint64_t *gring;     // [C][ring_words] slicer bits (read only)
    uint32_t ring_words, ring_mask;
    uint32_t n_channels, sps;
    uint64_t n_proc;           // absolute samples processed after this push
    uint64_t *events;          // [cap] amps_recc_seizure_t as four 8-byte words each
    uint32_t *hdr;             // {events held, 1 = events were dropped}
    uint32_t cap;              // events the device list may hold until the next drain
};

// One workgroup walks the channels in tiles of SEIZURE_THREADS and compacts the tile's events in channel order: ballot + prefix inside
// a wave, the wave totals through LDS.  No per-thread atomics: the order of the list, and what an overflow keeps, are deterministic.
__global__ __launch_bounds__(SEIZURE_THREADS) void recc_seizure_kernel(SeizureArgs a)
{
    __shared__ uint32_t s_tot[SEIZURE_THREADS / 64];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    uint32_t base = a.hdr[0];                                           // uniform
    const uint32_t held = base;
    for (uint32_t c0 = 0; c0 < a.n_channels; c0 += SEIZURE_THREADS) {
        const uint32_t c = c0 + (uint32_t)tid;
        uint64_t p = ~0ull;
        bool ev = false;
        if (c < a.n_channels) {
            p = a.pending[c];
            ev = p != ~0ull && p != a.reported[c];
        }
        const unsigned long long m = __ballot(ev);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_tot[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < SEIZURE_THREADS / 64; w++) {
            if (w < wv) off += s_tot[w];
            tot += s_tot[w];
        }
        if (ev) {
            a.reported[c] = p;                                          // reported or dropped: never looked at again
            const uint32_t slot = base + off + rank;
            if (slot < a.cap) {
                // the coded DCC at the trigger's own timing: symbol i = the slicer bit at p + sps (i + 1)
                const bool complete = p + (uint64_t)SEIZURE_DCC_SYMS * a.sps < a.n_proc;
                uint64_t dcc = 0ull;
                if (complete) {
                    const uint64_t *ring = a.gring + (uint64_t)c * a.ring_words;
                    uint32_t sym = 0u, bad = 0u;
                    for (int i = 0; i < SEIZURE_DCC_SYMS; i++) {
                        const uint64_t n = p + (uint64_t)a.sps * (uint32_t)(i + 1);
                        sym |= (uint32_t)((ring[(n >> 6) & a.ring_mask] >> (n & 63)) & 1ull) << i;
                    }
                    for (int j = 0; j < SEIZURE_DCC_SYMS / 2; j++) {
                        const uint32_t s0 = (sym >> (2 * j)) & 1u, s1 = (sym >> (2 * j + 1)) & 1u;
                        dcc |= (uint64_t)(s0 ^ 1u) << (8 * j);              // dcc[j] = !s_2j
                        bad += s0 == s1 ? 1u : 0u;
                    }
                    dcc |= (uint64_t)bad << 56;                             // dcc_bad
                }
                uint64_t *e = a.events + (size_t)slot * (AMPS_RECC_SEIZURE_BYTES / 8);
                e[0] = (uint64_t)c | ((uint64_t)(complete ? AMPS_SEIZURE_FLAG_DCC_COMPLETE : 0u) << 32);   // {channel, flags}
                e[1] = p;
                e[2] = dcc;
                e[3] = a.n_proc;
            }
        }
        base += tot;
        __syncthreads();                                                // s_tot is written again by the next tile
    }
    if (tid == 0 && base != held) {
        a.hdr[0] = base < a.cap ? base : a.cap;
        if (base > a.cap) a.hdr[1] = 1u;
    }
}

struct SeizureState {
    DevBuf<uint64_t> reported;                // [C]
    DevBuf<uint64_t> events;                  // [max_bursts] events of four words
    DevBuf<uint32_t> hdr;                     // {held, dropped}
    std::vector<amps_recc_seizure_t> held;    // taken off the device by a drain whose caller had room for fewer: oldest first
    bool dropped = false;                     // events were dropped since the last drain that said so
    uint32_t C = 0, cap = 0;
    bool enabled = false;
};

inline int seizure_create(SeizureState &z, uint32_t C, uint32_t max_bursts)
{
    z.C = C; z.cap = max_bursts;
    if (z.reported.alloc(C) | z.events.alloc((size_t)max_bursts * (AMPS_RECC_SEIZURE_BYTES / 8)) | z.hdr.alloc(2)) return -ENOMEM;
    z.enabled = true;
    return 0;
}

inline int seizure_reset(SeizureState &z, hipStream_t s)
{
    if (!z.enabled) return 0;
    z.held.clear(); z.dropped = false;
    HIP_TRY(hipMemsetAsync(z.reported.get(), 0xff, sizeof(uint64_t) * z.C, s));
    HIP_TRY(hipMemsetAsync(z.hdr.get(), 0, 2 * sizeof(uint32_t), s));
    return 0;
}

// behind the resolve (and, in the queue form, the capture kernel) of a push that processed the stream up to n_proc.  The device list
// may hold what the handle's capacity leaves beside the events a drain has still to hand out; `held` changes only in a drain, which
// has waited for the stream.
inline void seizure_launch(const SeizureState &z, const uint64_t *pending, const uint64_t *gring, uint32_t ring_words, uint32_t sps, uint64_t n_proc, hipStream_t s)
{
    SeizureArgs a{};
    a.pending = pending; a.reported = z.reported.get(); a.gring = gring; a.ring_words = ring_words; a.ring_mask = ring_words - 1;
    a.n_channels = z.C; a.sps = sps; a.n_proc = n_proc;
    a.events = z.events.get(); a.hdr = z.hdr.get();
    a.cap = z.cap - (uint32_t)std::min<size_t>(z.held.size(), z.cap);
    hipLaunchKernelGGL(recc_seizure_kernel, dim3(1), dim3(SEIZURE_THREADS), 0, s, a);
}

// The drain, once the caller has waited for the stream: the device list moves behind what is held, the oldest min(cap, held) go out.
inline int seizure_drain(SeizureState &z, hipStream_t s, amps_recc_seizure_t *out, size_t cap, size_t *nout, size_t *nleft)
{
    uint32_t hdr[2] = { 0u, 0u };
    HIP_TRY(hipMemcpy(hdr, z.hdr.get(), sizeof(hdr), hipMemcpyDeviceToHost));
    const size_t n = std::min<size_t>(hdr[0], z.cap), had = z.held.size();
    if (n) {
        z.held.resize(had + n);
        if (hipMemcpy(z.held.data() + had, z.events.get(), n * sizeof(amps_recc_seizure_t), hipMemcpyDeviceToHost) != hipSuccess) { z.held.resize(had); return -EIO; }
    }
    if (hdr[0] || hdr[1]) HIP_TRY(hipMemsetAsync(z.hdr.get(), 0, sizeof(hdr), s));
    if (hdr[1]) z.dropped = true;
    const size_t take = std::min(cap, z.held.size());
    if (take) std::memcpy(out, z.held.data(), take * sizeof(amps_recc_seizure_t));
    z.held.erase(z.held.begin(), z.held.begin() + (std::ptrdiff_t)take);
    *nout = take;
    if (nleft) *nleft = z.held.size();
    const int rc = z.dropped ? -ENOSPC : 0;
    z.dropped = false;
    return rc;
}

} // namespace amps
