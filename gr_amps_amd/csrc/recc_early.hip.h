// recc_early.hip.h -- early messages (AMPS_RECC_FLAG_EARLY_MESSAGES; the contract stands in include/amps_recc_early.h at
// amps_recc_drain_early): the record of a message's announced words, after the push in which the last repeat of the last of them
// arrived.  The resolve kernel parks an accepted trigger whose tail has not arrived in pending[channel] (recc_resolve.hip.h); the two
// kernels here, launched behind every resolve (and behind the seizure kernel), look at each such capture:
//   recc_early_wave_kernel   one wave per channel.  Once word A is in, it walks the capture's first six blocks, decodes word A and
//                            keeps the announced length in the channel's state; once the last announced word is in, it walks the
//                            prefix of 1 + 5 n_words blocks, runs the decode core and stages the event in the channel's own slot.
//   recc_early_scan_kernel   one workgroup.  It appends the staged events of the push to the list in channel order: ballot + prefix
//                            as the seizure kernel, no per-event atomics, so the order of the list and what an overflow keeps are
//                            deterministic; the 744 bytes of every event are moved by the whole workgroup.
// One state: per channel the capture looked at and how far, the staged events, the device list with its header, and what a drain has
// taken off the device but not yet handed out.  A handle without the flag has none of it and launches nothing.
#pragma once
#include <vector>
#include "amps_recc_early.h"
#include "recc_devmem.hip.h"
#include "recc_resolve.hip.h"

namespace amps {

static_assert(sizeof(amps_recc_early_t) == AMPS_RECC_EARLY_BYTES && AMPS_RECC_EARLY_BYTES == sizeof(amps_recc_burst_t) + 16, "event layout is part of the ABI");

constexpr int EARLY_WAVES = 4;                         // channels per workgroup of the wave kernel
constexpr int EARLY_SCAN_THREADS = 256;                // channels per tile of the ordered scan
constexpr int EARLY_DWORDS = AMPS_RECC_EARLY_BYTES / 4;
constexpr uint32_t EARLY_MAX_WORDS = AMPS_RECC_WORDS - 1;   // a message of seven words has no event: its record is there in the same push
// the channel's state: 0 = word A of its pending capture has not been looked at, 1 ... 6 = the words it announced (waiting for the last
// of them), or one of:
constexpr uint32_t EARLY_NEVER = 0xffu;                // word A invalid, or seven words announced
constexpr uint32_t EARLY_DONE = 0xfeu;                 // staged (reported, or dropped by a full list): never looked at again

// samples that must have been processed for the first n words of capture p to be in: T(n) < n_proc
__host__ __device__ constexpr uint64_t early_due(uint64_t p, uint32_t sps, uint32_t n, bool track)
{
    return p + (uint64_t)sps * (15u + 2u * AMPS_RECC_WORD_BITS * AMPS_RECC_REPEATS * n) + (track ? AMPS_TRACK_BLOCKS : 0);
}

struct EarlyArgs {
    const uint64_t *pending;   // [C], ~0 = none: what the resolve of this push left (read only)
    const uint64_t *gring;     // [C][ring_words] slicer bits (read only)
    uint32_t ring_words, ring_mask;
    uint32_t cap_words;        // ring words one wave's LDS window holds (resolve_cap_words)
    uint32_t n_channels, sps, track, majority;
    uint64_t n_proc;           // absolute samples processed after this push
    uint64_t *cap_p;           // [C], ~0 = none: the capture the channel's state speaks of
    uint32_t *state;           // [C]: see above
    uint32_t *due;             // [C]: n_words of the event staged in this push, 0 = none (cleared by the scan)
    uint32_t *stage;           // [C][EARLY_DWORDS]
    uint32_t *events;          // [cap][EARLY_DWORDS]
    uint32_t *hdr;             // {events held, 1 = events were dropped}
    uint32_t cap;              // events the device list may hold until the next drain
};

// The capture walk of manchester_from_ring (recc_decode.hip.h) limited to its first nblocks = 1 + 5 n blocks: the trigger, the coded
// DCC with repeat 0 of word A, and the other repeats of the first n words.  Same windows, same statistics, same decisions in the same
// order -- block b's delay depends on blocks <= b only, so what this writes is the prefix of what the full walk writes.  A function of
// its own, as stream_unit_autocorr_kernel is: a bound passed into the shared body would change the resolve and capture kernels, whose
// loop has a constant trip count.  The window of the block BEHIND the last is not fetched (the stream may not have written it): the
// last round fetches nothing it uses, as the full walk's does.  The bits of the words >= n are cleared, and so are their counts.
template <class Sync, bool TWO>
__device__ __forceinline__ void manchester_prefix_from_ring(DecodeCore &s, const uint64_t *ring, uint64_t nc, uint64_t w0, uint32_t sps, int lane, bool track,
                                                            int nblocks)
{
    constexpr int EARLY = TWO ? 2 : 1;
    decode_core_begin(s, lane);
    for (int i = BOFF + 7 + AMPS_RECC_WORD_BITS * (nblocks - 1) + lane; i < (int)sizeof(s.bits); i += 64) s.bits[i] = 0;
    Sync::sync();
    const uint32_t *r32 = (const uint32_t *)ring;
    const int32_t base = (int32_t)(nc - (w0 << 6));
    const uint32_t midmask = (1u << (sps - 1)) - 1u;
    uint32_t f_lo = 0u, f_hi = 0u, f_sh = 0u;
    int dly = 0, dly_fetched = 0;
    uint32_t badacc = 0u;
    auto fetch = [&](int k, int d, bool on) {
        const uint32_t na = (uint32_t)(base + (int32_t)sps * (2 * k + 1) + d - EARLY);
        const uint32_t q = on ? na >> 5 : 0u;
        f_lo = r32[q]; f_hi = r32[q + 1]; f_sh = na & 31u;
    };
    auto measure = [&](uint32_t w, bool on) {
        const uint32_t sa = w & 1u, sb = (w >> sps) & 1u;
        const uint32_t mid = (w >> 1) & midmask;
        const uint32_t cnt = (uint32_t)__popc(sa ? mid : (~mid & midmask));
        const uint32_t contrib = (on && sa != sb) ? ((cnt | (1u << 10)) << (sa ? 0 : 16)) : 0u;
        const uint32_t tot = wave_sum_u32(contrib);
        const int sum1 = (int)(tot & 0x3ffu), n1 = (int)((tot >> 10) & 0x3fu), sum0 = (int)((tot >> 16) & 0x3ffu), n0 = (int)(tot >> 26);
        const int E1 = 2 * sum1 - (int)(sps - 1) * n1, E0 = 2 * sum0 - (int)(sps - 1) * n0;
        const int lhs = E1 * n0 + E0 * n1, rhs = 2 * n0 * n1;
        if (rhs > 0) dly += lhs > rhs ? 1 : lhs < -rhs ? -1 : 0;
    };
    auto choose2 = [&](uint32_t w, bool on) -> int {
        const uint32_t e = w ^ (w >> 2);
        const uint32_t contrib = on ? ((~e & 1u) | ((~e & 2u) << 7) | ((~e & 4u) << 14)) : 0u;
        const uint32_t tot = wave_sum_u32(contrib);
        const uint32_t vm = tot & 0xffu, v0 = (tot >> 8) & 0xffu, vp = tot >> 16;
        int mv = 0;
        uint32_t best = v0;
        if (vm < v0) { mv = -1; best = vm; }
        if (vp < v0 && vp < best) mv = 1;
        return mv;
    };
    // ---- block 0: the 37 bits of the trigger, measured only; what lies in front of the stream reads 1
    {
        const int k = -TRACK_PRE_BITS + lane;
        const bool on = lane < TRACK_PRE_BITS;
        const int32_t nas = base + (int32_t)sps * (2 * k + 1) - 1;
        const uint32_t na = nas < 0 ? 0u : (uint32_t)nas, q = on ? na >> 5 : 0u;
        const int32_t sh = -nas - 1;
        const uint32_t w = nas >= 0 ? __builtin_amdgcn_alignbit(r32[q + 1], r32[q], na & 31u) >> 1
                                    : sh >= 32 ? ~0u : ((r32[0] << (uint32_t)sh) | ((1u << (uint32_t)sh) - 1u));
        fetch(lane, 0, lane < 7 + AMPS_RECC_WORD_BITS);
        if constexpr (TWO) {
            const uint32_t w2 = nas >= 0 ? __builtin_amdgcn_alignbit(r32[q + 1], r32[q], na & 31u)
                                         : sh + 1 >= 32 ? ~0u : ((r32[0] << (uint32_t)(sh + 1)) | ((1u << (uint32_t)(sh + 1)) - 1u));
            if (track) dly += choose2(w2, on);
        } else {
            if (track) measure(w, on);
        }
    }
    // ---- block 1: the coded DCC (bits 0..6) and repeat 0 of word 0
    {
        const int k = lane;
        const bool on = lane < 7 + AMPS_RECC_WORD_BITS;
        uint32_t w = __builtin_amdgcn_alignbit(f_hi, f_lo, f_sh) >> (uint32_t)(dly + 1);
        const int d1 = dly;
        fetch(7 + AMPS_RECC_WORD_BITS + lane, d1, lane < AMPS_RECC_WORD_BITS);
        if constexpr (TWO) {
            const int mv = track ? choose2(w, on) : 0;
            dly += mv;
            w >>= (uint32_t)(mv + 1);
        }
        const uint32_t sa = w & 1u, sb = (w >> sps) & 1u;
        if (on) s.bits[BOFF + k] = (uint8_t)(sa == sb ? (sa ^ 1u) : sb);
        const uint64_t bad = __ballot(on && sa == sb);
        if (lane == 0) s.bad[0] = (uint32_t)__popcll(bad & 0x7full);
        badacc = (uint32_t)__popcll(bad >> 7);
        if constexpr (!TWO) { if (track) measure(w, on); }
        dly_fetched = d1;
    }
    // ---- blocks 2 .. nblocks - 1: repeat r of word w (block = 1 + 5 w + r), 48 bits each
    const bool on48 = lane < AMPS_RECC_WORD_BITS;
    uint8_t *bitp = &s.bits[BOFF + 7 + AMPS_RECC_WORD_BITS + lane];
    int kn = 7 + 2 * AMPS_RECC_WORD_BITS + lane;
    int rep = 1, word = 0;
#pragma unroll 1
    for (int b = 2; b < nblocks; b++) {
        uint32_t w = __builtin_amdgcn_alignbit(f_hi, f_lo, f_sh) >> (uint32_t)(dly - dly_fetched + 1);
        dly_fetched = dly;
        fetch(kn, dly, on48 && b + 1 < nblocks);
        kn += AMPS_RECC_WORD_BITS;
        if constexpr (TWO) {
            const int mv = track ? choose2(w, on48) : 0;
            dly += mv;
            w >>= (uint32_t)(mv + 1);
        }
        const uint32_t sa = w & 1u, sb = (w >> sps) & 1u;
        if (on48) *bitp = (uint8_t)(sa == sb ? (sa ^ 1u) : sb);
        bitp += AMPS_RECC_WORD_BITS;
        badacc += (uint32_t)__popcll(__ballot(on48 && sa == sb));
        if (++rep == AMPS_RECC_REPEATS) {
            if (lane == 0) s.bad[1 + word] = badacc;
            badacc = 0u; rep = 0; word++;
        }
        if constexpr (!TWO) { if (track) measure(w, on48); }
    }
    Sync::sync();
}

// One wave per channel; the waves of a workgroup share nothing but the dynamic LDS allocation ([EARLY_WAVES][resolve_cap_stride]) and
// leave independently: no workgroup barrier anywhere.  Everything a wave decides on is uniform across its lanes.
template <bool TWO>
__global__ __launch_bounds__(EARLY_WAVES * 64) void recc_early_wave_kernel(EarlyArgs a)
{
    extern __shared__ uint64_t s_early[];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * EARLY_WAVES + (uint32_t)wv;
    if (c >= a.n_channels) return;
    const uint64_t p = a.pending[c];
    if (p == ~0ull) return;
    const bool fresh = a.cap_p[c] != p;
    const uint32_t st0 = fresh ? 0u : a.state[c];
    uint32_t st = st0;
    uint64_t *scratch = s_early + (size_t)wv * resolve_cap_stride(a.cap_words);
    DecodeCore &k = *(DecodeCore *)scratch;
    uint64_t *s_ring = scratch + (sizeof(DecodeCore) + 7) / 8;
    const uint64_t *ring = a.gring + (uint64_t)c * a.ring_words;
    const uint64_t w0 = capture_first_word(p, a.sps);
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {                              // word A, then (possibly in the same push) the message
        if (st > EARLY_MAX_WORDS) break;
        const uint32_t n = st ? st : 1u;
        const uint64_t T = early_due(p, a.sps, n, a.track != 0);
        if (!(T < a.n_proc)) break;
        // the window: from the trigger's first symbol to the last sampling instant of word n - 1 at the latest delay (< T), and the
        // funnel shift's second dword.  Every word lies inside the channel's ring (the index is masked) and inside the LDS window
        // (fewer words than a whole capture's, which cap_words holds).
        int nw = (int)(((T + 32) >> 6) - w0) + 2;
        if (nw > (int)a.cap_words) nw = (int)a.cap_words;
        for (int i = lane; i < nw; i += 64) s_ring[i] = ring[(w0 + (uint64_t)i) & a.ring_mask];
        WaveSync::sync();
        manchester_prefix_from_ring<WaveSync, TWO>(k, s_ring, p, w0, a.sps, lane, a.track != 0, 1 + AMPS_RECC_REPEATS * (int)n);
        decode_core_wave<WaveSync>(k, c, p, nullptr, a.majority != 0, lane);
        if (st == 0u) {
            const uint32_t valid = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.rec.valid[0]);
            const uint32_t words = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.rec.a_NAWC) + 1u;
            st = (!valid || words > EARLY_MAX_WORDS) ? EARLY_NEVER : words;
            WaveSync::sync();                                           // the next pass writes the scratch again
            continue;
        }
        if (lane >= (int)n && lane < AMPS_RECC_WORDS) { k.rec.valid[lane] = 0; k.rec.first_valid_rep[lane] = (uint8_t)AMPS_RECC_REPEATS; }
        WaveSync::sync();
        uint32_t *dst = a.stage + (size_t)c * EARLY_DWORDS;
        for (int i = lane; i < (int)(sizeof(amps_recc_burst_t) / 4); i += 64) dst[i] = ((const uint32_t *)&k.rec)[i];
        if (lane == 0) {
            dst[EARLY_DWORDS - 4] = (uint32_t)a.n_proc; dst[EARLY_DWORDS - 3] = (uint32_t)(a.n_proc >> 32);
            dst[EARLY_DWORDS - 2] = n; dst[EARLY_DWORDS - 1] = 0u;
            a.due[c] = n;
        }
        st = EARLY_DONE;
    }
    if (lane == 0 && (fresh || st != st0)) { a.cap_p[c] = p; a.state[c] = st; }
}

// One workgroup walks the channels in tiles of EARLY_SCAN_THREADS and compacts the tile's staged events in channel order (ballot +
// prefix inside a wave, the wave totals through LDS), then moves them, all threads together, a dword per thread and round.
__global__ __launch_bounds__(EARLY_SCAN_THREADS) void recc_early_scan_kernel(EarlyArgs a)
{
    __shared__ uint32_t s_tot[EARLY_SCAN_THREADS / 64];
    __shared__ uint32_t s_src[EARLY_SCAN_THREADS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    uint32_t base = a.hdr[0];                                           // uniform
    const uint32_t held = base;
    for (uint32_t c0 = 0; c0 < a.n_channels; c0 += EARLY_SCAN_THREADS) {
        const uint32_t c = c0 + (uint32_t)tid;
        const bool ev = c < a.n_channels && a.due[c] != 0u;
        const unsigned long long m = __ballot(ev);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_tot[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < EARLY_SCAN_THREADS / 64; w++) {
            if (w < wv) off += s_tot[w];
            tot += s_tot[w];
        }
        if (ev) {
            a.due[c] = 0u;                                              // appended or dropped
            s_src[off + rank] = c;
        }
        __syncthreads();
        const uint32_t room = base < a.cap ? a.cap - base : 0u, take = tot < room ? tot : room;
        for (uint32_t i = (uint32_t)tid; i < take * EARLY_DWORDS; i += EARLY_SCAN_THREADS) {
            const uint32_t e = i / EARLY_DWORDS, d = i % EARLY_DWORDS;
            a.events[(size_t)(base + e) * EARLY_DWORDS + d] = a.stage[(size_t)s_src[e] * EARLY_DWORDS + d];
        }
        base += tot;
        __syncthreads();                                                // s_tot and s_src are written again by the next tile
    }
    if (tid == 0 && base != held) {
        a.hdr[0] = base < a.cap ? base : a.cap;
        if (base > a.cap) a.hdr[1] = 1u;
    }
}

struct EarlyState {
    DevBuf<uint64_t> cap_p;                   // [C]
    DevBuf<uint32_t> state, due;              // [C]
    DevBuf<uint32_t> stage;                   // [C] events
    DevBuf<uint32_t> events;                  // [max_bursts] events
    DevBuf<uint32_t> hdr;                     // {held, dropped}
    std::vector<amps_recc_early_t> held;      // taken off the device by a drain whose caller had room for fewer: oldest first
    bool dropped = false;                     // events were dropped since the last drain that said so
    uint32_t C = 0, cap = 0;
    bool enabled = false;
};

inline int early_create(EarlyState &z, uint32_t C, uint32_t max_bursts)
{
    z.C = C; z.cap = max_bursts;
    if (z.cap_p.alloc(C) | z.state.alloc(C) | z.due.alloc(C) | z.stage.alloc((size_t)C * EARLY_DWORDS)
        | z.events.alloc((size_t)max_bursts * EARLY_DWORDS) | z.hdr.alloc(2)) return -ENOMEM;
    z.enabled = true;
    return 0;
}

inline int early_reset(EarlyState &z, hipStream_t s)
{
    if (!z.enabled) return 0;
    z.held.clear(); z.dropped = false;
    HIP_TRY(hipMemsetAsync(z.cap_p.get(), 0xff, sizeof(uint64_t) * z.C, s));
    HIP_TRY(hipMemsetAsync(z.state.get(), 0, sizeof(uint32_t) * z.C, s));
    HIP_TRY(hipMemsetAsync(z.due.get(), 0, sizeof(uint32_t) * z.C, s));
    HIP_TRY(hipMemsetAsync(z.hdr.get(), 0, 2 * sizeof(uint32_t), s));
    return 0;
}

// behind the resolve (and, in the queue form, the capture kernel) of a push that processed the stream up to n_proc, outside its
// timing span.  The device list may hold what the handle's capacity leaves beside the events a drain has still to hand out; `held`
// changes only in a drain, which has waited for the stream.
inline void early_launch(const EarlyState &z, const uint64_t *pending, const uint64_t *gring, uint32_t ring_words, uint32_t sps, uint32_t track,
                         uint32_t majority, uint64_t n_proc, hipStream_t s)
{
    EarlyArgs a{};
    a.pending = pending; a.gring = gring; a.ring_words = ring_words; a.ring_mask = ring_words - 1; a.cap_words = resolve_cap_words(sps);
    a.n_channels = z.C; a.sps = sps; a.track = track; a.majority = majority; a.n_proc = n_proc;
    a.cap_p = z.cap_p.get(); a.state = z.state.get(); a.due = z.due.get(); a.stage = z.stage.get();
    a.events = z.events.get(); a.hdr = z.hdr.get();
    a.cap = z.cap - (uint32_t)std::min<size_t>(z.held.size(), z.cap);
    const size_t lds = (size_t)EARLY_WAVES * resolve_cap_stride(a.cap_words) * 8;
    const dim3 grid((z.C + EARLY_WAVES - 1) / EARLY_WAVES);
    if (sps == 2) hipLaunchKernelGGL(recc_early_wave_kernel<true>, grid, dim3(EARLY_WAVES * 64), lds, s, a);
    else hipLaunchKernelGGL(recc_early_wave_kernel<false>, grid, dim3(EARLY_WAVES * 64), lds, s, a);
    hipLaunchKernelGGL(recc_early_scan_kernel, dim3(1), dim3(EARLY_SCAN_THREADS), 0, s, a);
}

// The drain, once the caller has waited for the stream: the device list moves behind what is held, the oldest min(cap, held) go out.
inline int early_drain(EarlyState &z, hipStream_t s, amps_recc_early_t *out, size_t cap, size_t *nout, size_t *nleft)
{
    uint32_t hdr[2] = { 0u, 0u };
    HIP_TRY(hipMemcpy(hdr, z.hdr.get(), sizeof(hdr), hipMemcpyDeviceToHost));
    const size_t n = std::min<size_t>(hdr[0], z.cap), had = z.held.size();
    if (n) {
        z.held.resize(had + n);
        if (hipMemcpy(z.held.data() + had, z.events.get(), n * sizeof(amps_recc_early_t), hipMemcpyDeviceToHost) != hipSuccess) { z.held.resize(had); return -EIO; }
    }
    if (hdr[0] || hdr[1]) HIP_TRY(hipMemsetAsync(z.hdr.get(), 0, sizeof(hdr), s));
    if (hdr[1]) z.dropped = true;
    const size_t take = std::min(cap, z.held.size());
    if (take) std::memcpy(out, z.held.data(), take * sizeof(amps_recc_early_t));
    z.held.erase(z.held.begin(), z.held.begin() + (std::ptrdiff_t)take);
    *nout = take;
    if (nleft) *nleft = z.held.size();
    const int rc = z.dropped ? -ENOSPC : 0;
    z.dropped = false;
    return rc;
}

} // namespace amps
