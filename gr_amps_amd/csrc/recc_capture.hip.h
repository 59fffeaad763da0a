// recc_capture.hip.h -- host side of the capture seam: the trigger search and the resolve / capture / decode tail behind both the IQ
// seam (streaming kernel on channel-major IQ, recc_front.hip.h) and the wideband seam (slicer bits already in the ring: the search
// stage of the resolve kernel, recc_resolve.hip.h, or the same search as a launch of its own, recc_bits.hip.h).  One state: the
// buffers, the launch geometry fixed at create, and the position in the stream.  Records go to the handle's record lists
// (recc_records.hip.h).
#pragma once
#include "recc_resolve.hip.h"
#include "recc_records.hip.h"
#include "recc_timing.hip.h"
#include "recc_stream_power.hip.h"
#include "recc_stream_offset.hip.h"
#include "recc_seizure.hip.h"
#include "recc_early.hip.h"

namespace amps {

constexpr uint64_t MIN_SPAN = 16;   // tiles per wave at least: bounds the 2-tile halo overhead to 12.5 % on tiny pushes

inline uint32_t next_pow2(uint64_t v) { uint64_t p = 1; while (p < v) p <<= 1; return (uint32_t)p; }

struct CaptureState {
    DevBuf<float2> carry[2];
    DevBuf<uint64_t> gring, det;
    DevBuf<uint32_t> detcount;
    DevBuf<uint64_t> next_allowed, pending;
    DevBuf<unsigned long long> done_blocks;   // {resolve workgroups of the launch in flight that have finished, record slots they reserved}
    DevBuf<uint64_t> capq;                    // queue form of the capture (few channels: resolve_uses_queue)
    DevBuf<uint32_t> capq_count;
    DevBuf<float> dbg_d, dbg_S;               // debug taps (amps_recc_debug_demod)
    HostStage stage_iq;                       // host-resident IQ: [C][max_samples_per_push], allocated by the first host push
    // launch geometry
    uint32_t ring_words = 0;
    uint32_t max_waves = 0, max_chunks = 0, det_cap = 0;   // front-launch geometry bounds (see front_geometry)
    uint32_t max_waves_bits = 0;                           // the same for the bit-domain search kernel (more waves fit: it holds no samples)
    // position in the stream
    int carry_cur = 0;
    uint64_t n_done = 0, origin = 0;  // origin: absolute index of the stream's first sample (amps_recc_set_origin)
    uint32_t r_prev = 0;
    bool origin_locked = false;       // a push has happened since the last reset
    // fixed at create
    uint32_t C = 0, sps = 0, tol = 0, majority = 0, track = 1;
    int slicer = AMPS_SLICER_DEFAULT;
    bool wideband = false;            // the handle has a filter bank: its pushes arrive through the wideband seam
};

// AMPS_RECC_DEBUG_SYNC=1: synchronise after every launch and say which kernel ran (fault isolation)
inline bool debug_sync_enabled() { return env_is("AMPS_RECC_DEBUG_SYNC", env_one); }
inline int debug_sync(hipStream_t s, const char *what)
{
    if (!debug_sync_enabled()) return 0;
    std::fprintf(stderr, "amps_recc[debug]: %s ...", what); std::fflush(stderr);
    hipError_t e = hipStreamSynchronize(s);
    std::fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e)); std::fflush(stderr);
    return e == hipSuccess ? 0 : -EIO;
}

typedef void (*front_kernel_t)(FrontArgs);
// The streaming kernel for one slicer spec.  Its tile depth (tiles in flight per wave beyond the one being processed) is part of
// the choice: tolerant sync always takes depth 1, and without it specs A and D take depth 1, specs B and C depth 2.  Measured
// with the non-temporal tile loads (832 x 2^18, ms): spec A 0.329 at depth 1 / 0.342 at depth 2 (its discriminator needs the
// registers: depth 2 costs a wave per SIMD); specs B / C 0.298 / 0.286: with the arctangent gone the kernel only waits for HBM.
// Round 4: depth 2 is compiled for four waves per SIMD too (a handful of prologue spills, none in the tile loop).  Same box, ms:
// spec A 0.3336 at depth 1 / 0.3343 at depth 2; D 0.3208 / 0.3174; B 0.3118 (three waves) -> 0.3038; C 0.3122 -> 0.3055.  The
// default spec keeps depth 1 -- 1 % slower and no scratch at all; the opt-in specs B and C take depth 2.
template <int SPS, int SL> front_kernel_t front_kernel_of(bool tol)
{
    constexpr int DEPTH = (SL == AMPS_SLICER_ATAN_BOXCAR || SL == AMPS_SLICER_EXACT) ? 1 : 2;
    return tol ? recc_front_kernel<SPS, 1, true, SL> : recc_front_kernel<SPS, DEPTH, false, SL>;
}
template <int SPS> front_kernel_t front_kernel_of(int slicer, bool tol)
{
    switch (slicer) {
    case AMPS_SLICER_PRODUCT: return front_kernel_of<SPS, AMPS_SLICER_PRODUCT>(tol);
    case AMPS_SLICER_SINE: return front_kernel_of<SPS, AMPS_SLICER_SINE>(tol);
    case AMPS_SLICER_EXACT: return front_kernel_of<SPS, AMPS_SLICER_EXACT>(tol);
    default: return front_kernel_of<SPS, AMPS_SLICER_ATAN_BOXCAR>(tol);
    }
}
// The streaming kernel for (samples per symbol, slicer spec, tolerant sync); nullptr for a rate it is not built for.  This switch
// is the one table of the rates the streaming kernel supports.  sps = 2 is launchable but not supported (sps_supported): only the
// two-kernel form of the wideband seam at D = 3 M / 4 reaches it -- the unfused 1024 bank at D = 768 and every narrow bank (512, 256,
// 128 branches) at its default ratio, which has no other form -- never a handle of the IQ seam.
inline front_kernel_t front_kernel_for(uint32_t sps, int slicer, bool tol)
{
    static const struct { uint32_t sps; front_kernel_t (*of)(int, bool); } rates[] = {
        { 2, front_kernel_of<2> }, { 3, front_kernel_of<3> }, { 4, front_kernel_of<4> }, { 5, front_kernel_of<5> },
        { 6, front_kernel_of<6> }, { 8, front_kernel_of<8> }, { 10, front_kernel_of<10> }, { 12, front_kernel_of<12> } };
    for (const auto &r : rates) if (r.sps == sps) return r.of(slicer, tol);
    return nullptr;
}
inline bool sps_supported(uint32_t sps) { return sps != 2 && front_kernel_for(sps, AMPS_SLICER_DEFAULT, false) != nullptr; }

// Which of its two forms the wideband seam's trigger search takes: true = the search stage inside the resolve kernel, which serves
// the many-channel form (no capture queue) at the wideband seam's two rates; false = the search as a launch of its own in front of it
// (recc_bits_kernel, rounds 2-5).  AMPS_RECC_BITS_KERNEL (read here and nowhere else) set to exactly "separate" asks for the second
// everywhere -- an independent launch structure the GPU suite checks the default against; any other value means the default.
inline bool search_in_resolve(bool wideband, bool queue, uint32_t sps)
{
    const bool separate = env_is("AMPS_RECC_BITS_KERNEL", [](const char *v) { return std::strcmp(v, "separate") == 0; });
    return wideband && !queue && !separate && (sps == 2 || sps == 3);
}

// The bit-domain search kernel for (samples per symbol, tolerant sync): capture_run_bits launches it, and capture_create sizes
// max_waves_bits by its occupancy.
inline front_kernel_t bits_kernel_for(uint32_t sps, bool tol)
{
    if (sps == 2) return tol ? recc_bits_kernel<2, true> : recc_bits_kernel<2, false>;
    return tol ? recc_bits_kernel<3, true> : recc_bits_kernel<3, false>;
}

// workgroups of 256 threads of kernel k that fit a CU, or `fallback` where the runtime cannot say
inline uint32_t blocks_per_cu(front_kernel_t k, uint32_t fallback)
{
    int n = 0;
    return (k && hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 256, 0) == hipSuccess && n > 0) ? (uint32_t)n : fallback;
}

typedef void (*resolve_kernel_t)(ResolveArgs);
struct ResolveLaunch { resolve_kernel_t resolve; int threads; resolve_kernel_t capture; };
// The resolve kernel (and its block size) and the capture kernel of the queue form for (a channel cut into more wave segments than
// one batch compacts, trigger search in the resolve kernel, two samples per symbol, tolerant search).  Two samples per symbol (the
// wideband seam at D = 768) have their own capture rule: a second instantiation of the kernels, so that the default ones carry
// nothing of it.
template <bool TWO> ResolveLaunch resolve_kernels_of(bool wide, bool search, bool stol)
{
    constexpr int SPS = TWO ? 2 : 3;
    const resolve_kernel_t capture = recc_capture_kernel<TWO>;
    if (wide) return { recc_resolve_kernel<RESOLVE_THREADS_WIDE, RESOLVE_LDS_HITS_WIDE, TWO>, RESOLVE_THREADS_WIDE, capture };
    if (search && stol) return { recc_resolve_kernel<RESOLVE_THREADS, RESOLVE_LDS_HITS, TWO, SPS, true>, RESOLVE_THREADS, capture };
    if (search) return { recc_resolve_kernel<RESOLVE_THREADS, RESOLVE_LDS_HITS, TWO, SPS, false>, RESOLVE_THREADS, capture };
    return { recc_resolve_kernel<RESOLVE_THREADS, RESOLVE_LDS_HITS, TWO>, RESOLVE_THREADS, capture };
}

// buffers and launch geometry for pushes of at most cfg.max_samples_per_push samples of each of C channels (the caller has made
// `device` current); the state is reset by capture_reset
inline int capture_create(CaptureState &c, const amps_recc_cfg_t &cfg, uint32_t C, int slicer, bool wideband, int device)
{
    c.C = C; c.sps = cfg.samples_per_symbol; c.slicer = slicer; c.wideband = wideband; c.tol = cfg.sync_tolerance;
    c.majority = (cfg.flags & AMPS_RECC_FLAG_MAJORITY) ? 1u : 0u;
    c.track = (cfg.flags & AMPS_RECC_FLAG_FIXED_TIMING) ? 0u : 1u;
    const uint64_t maxs = cfg.max_samples_per_push;
    c.ring_words = next_pow2(maxs + (uint64_t)c.sps * (AMPS_RECC_CAPTURE_SYMS + 2 * AMPS_RECC_TRIGGER_SYMS + 64) + 2 * TILE) / 64;
    // Front launch = one round of resident waves: 4 workgroups (16 waves) per CU, each wave owning an equal
    // span of the flattened (channel, tile) space.  A channel is covered by at most max_waves/C + 2 segments.
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return -ENODEV;
    const bool queue = resolve_uses_queue(C);
    const uint32_t cu_waves = (uint32_t)prop.multiProcessorCount * 4u;
    c.max_waves = cu_waves * blocks_per_cu(front_kernel_for(c.sps, slicer, c.tol != 0), 2);   // exactly one resident round of the kernel capture_run_iq will pick
    // (max_chunks below assumes at most 32 waves per CU)
    c.max_waves_bits = cu_waves * std::min(blocks_per_cu(bits_kernel_for(c.sps, c.tol != 0), 4), 8u);
    const uint64_t max_tiles = (maxs + 63 + TILE - 1) / TILE;
    const uint64_t max_span = std::max<uint64_t>(MIN_SPAN, (C * max_tiles + c.max_waves - 1) / c.max_waves);
    c.max_chunks = (uint32_t)(prop.multiProcessorCount * 32u / C + 3);   // bound for any occupancy
    c.det_cap = (uint32_t)(max_span * TILE / ((uint64_t)AMPS_RECC_TRIGGER_SYMS * c.sps) + 4);
    int rc = c.carry[0].alloc((size_t)C * CARRY_CAP) | c.carry[1].alloc((size_t)C * CARRY_CAP) | c.gring.alloc((size_t)C * c.ring_words)
           | c.det.alloc((size_t)C * c.max_chunks * c.det_cap) | c.detcount.alloc((size_t)C * c.max_chunks) | c.next_allowed.alloc(C)
           | c.pending.alloc(C) | c.done_blocks.alloc(1 + DONE_GROUPS);
    if (queue) rc |= c.capq.alloc(cfg.max_bursts) | c.capq_count.alloc(1);
    return rc;
}

inline int capture_reset(CaptureState &c, hipStream_t s)
{
    c.carry_cur = 0; c.n_done = 0; c.origin = 0; c.origin_locked = false; c.r_prev = 0;
    if (!c.carry[0]) return 0;                        // no IQ seam on this handle
    HIP_TRY(hipMemsetAsync(c.carry[0].get(), 0, sizeof(float2) * (size_t)c.C * CARRY_CAP, s));
    HIP_TRY(hipMemsetAsync(c.carry[1].get(), 0, sizeof(float2) * (size_t)c.C * CARRY_CAP, s));
    HIP_TRY(hipMemsetAsync(c.gring.get(), 0xff, sizeof(uint64_t) * (size_t)c.C * c.ring_words, s));
    HIP_TRY(hipMemsetAsync(c.detcount.get(), 0, sizeof(uint32_t) * (size_t)c.C * c.max_chunks, s));
    HIP_TRY(hipMemsetAsync(c.next_allowed.get(), 0, sizeof(uint64_t) * c.C, s));
    HIP_TRY(hipMemsetAsync(c.pending.get(), 0xff, sizeof(uint64_t) * c.C, s));
    HIP_TRY(hipMemsetAsync(c.done_blocks.get(), 0, (1 + DONE_GROUPS) * sizeof(unsigned long long), s));
    if (c.capq_count) HIP_TRY(hipMemsetAsync(c.capq_count.get(), 0, sizeof(uint32_t), s));
    return 0;
}

// Geometry of the persistent front launch over P samples of each of C channels: Tc tiles per channel, cut into `nwaves` equal
// spans of the flattened (channel, tile) space -- one resident round of at most max_waves waves, a span never under MIN_SPAN tiles.
struct FrontGeom { uint32_t Tc, span, nwaves; };
inline FrontGeom front_geometry(uint32_t C, uint32_t P, uint32_t max_waves)
{
    const uint32_t Tc = (P + TILE - 1) / TILE;
    const uint64_t G = (uint64_t)C * Tc;
    uint32_t nwaves = (uint32_t)std::min<uint64_t>(max_waves, (G + MIN_SPAN - 1) / MIN_SPAN);
    if (nwaves == 0) nwaves = 1;
    return { Tc, (uint32_t)((G + nwaves - 1) / nwaves), nwaves };
}
// The resolve kernel of a push of P samples (and the capture kernel of the queue form) behind a front launch of geometry g.  search:
// the trigger search runs inside the kernel (search_in_resolve), and the push's housekeeping with it: zero2 from records_appending
// (det and detcount then go unread: that form keeps its hits in LDS).
inline void launch_resolve(CaptureState &c, const RecordListView &list, TimingState &tm, const FrontGeom &g, uint32_t P, hipStream_t s, bool search = false, uint32_t *zero2 = nullptr)
{
    ResolveArgs ra{};
    ra.det = c.det.get(); ra.detcount = c.detcount.get(); ra.max_chunks = c.max_chunks; ra.det_cap = c.det_cap;
    ra.tiles_per_channel = g.Tc; ra.span = g.span; ra.sps = c.sps; ra.n_proc = c.n_done + P;
    ra.next_allowed = c.next_allowed.get(); ra.pending = c.pending.get();
    if (search) { ra.search_P = P; ra.search_tol = c.tol; ra.zero1 = c.capq_count.get(); ra.zero2 = zero2; }
    // capture + decode side of the kernel
    ra.gring = c.gring.get(); ra.ring_mask = c.ring_words - 1; ra.ring_words = c.ring_words; ra.cap_words = resolve_cap_words(c.sps);
    ra.records = list.records; ra.nrecords = list.nrecords; ra.rec_cap = list.rec_cap; ra.status = list.status;
    ra.majority = c.majority; ra.track = c.track;
    ra.burst_syms = list.burst_syms;
    ra.done_blocks = c.done_blocks.get(); ra.hdr_host = list.hdr_host;
    ra.capq = c.capq.get(); ra.capq_count = c.capq_count.get(); ra.capq_cap = list.rec_cap;
    const size_t lds = c.capq ? 0 : resolve_dyn_lds(c.sps);
#ifdef RESOLVE_TIMELINE
    static TimelineBuf &tl = *new TimelineBuf();                 // kept for the life of the process
    ra.tl = tl.clear((size_t)24 * 4096, (size_t)24 * c.C, s);   // [C][24]; a handle with more than 4096 channels goes without
#endif
    // The wide instantiation (a channel cut into more wave segments than 256 lanes compact in one batch) exists for handles with few
    // channels, which always take the queue form: its 36.9 KB of static LDS next to the fused capture form's dynamic LDS is a
    // combination max_chunks never produces for 64 channels or more (Tc / span + 2 <= max_waves / C + 4 <= 131 there).  Held here, so
    // that a change to either threshold cannot turn into a launch failure: a handle without a queue stays on the narrow kernel, whose
    // batches walk any number of segments.
    const bool wide = ra.tiles_per_channel / ra.span + 2 > (uint64_t)RESOLVE_THREADS && c.capq;
    const ResolveLaunch k = c.sps == 2 ? resolve_kernels_of<true>(wide, search, ra.search_tol != 0) : resolve_kernels_of<false>(wide, search, ra.search_tol != 0);
    SpanGuard span(tm, s, c.wideband, T_RESOLVE);
    hipLaunchKernelGGL(k.resolve, dim3(c.C), dim3(k.threads), lds, s, ra);
    if (c.capq) {
        const dim3 gq(std::min<uint32_t>(list.rec_cap, 2048u));
        const size_t ldsq = (size_t)resolve_cap_stride(ra.cap_words) * 8;
        hipLaunchKernelGGL(k.capture, gq, dim3(64), ldsq, s, ra);
    }
    span.end();
#ifdef RESOLVE_TIMELINE
    if (ra.tl) tl.dump("AMPS_RECC_RESOLVE_TIMELINE", (size_t)24 * c.C, s);   // the last launch's stamps
#endif
}

// the part of the streaming / bit-domain kernel's arguments that both seams fill the same way, with the push's housekeeping: the
// kernel (thread 0) clears the capture queue count (null in the fused form) and the idle record list's words (records_appending)
inline FrontArgs front_args(const CaptureState &c, RecordLists &L, const FrontGeom &g, uint32_t r_prev, uint32_t avail, uint32_t P)
{
    FrontArgs fa{};
    fa.r_prev = r_prev; fa.avail = avail; fa.P = P; fa.tiles_per_channel = g.Tc; fa.n_channels = c.C; fa.span = g.span;
    fa.n_done = c.n_done; fa.gring = c.gring.get(); fa.ring_mask = c.ring_words - 1; fa.ring_words = c.ring_words;
    fa.det = c.det.get(); fa.detcount = c.detcount.get(); fa.max_chunks = c.max_chunks; fa.det_cap = c.det_cap;
    fa.tol = c.tol;
    fa.status = records_current(L).status;
    fa.zero1 = c.capq_count.get();
    fa.zero2 = records_appending(L);
    return fa;
}

// the fused chain on channel-major device IQ: front -> carry -> resolve -> capture/decode
// one workgroup per channel; wide groups when a channel spans more wave segments than 256 lanes cover in one batch.
// pw: the handle keeps received power (AMPS_RECC_FLAG_STREAM_POWER): its block means are taken behind the streaming kernel, from the
// block and the carry that launch read; ac: likewise its lag-one autocorrelation sums (AMPS_RECC_FLAG_STREAM_OFFSET); sz: the handle
// keeps seizure events (AMPS_RECC_FLAG_SEIZURE_EVENTS): their kernel runs behind the resolve, outside its timing span; ez: it keeps
// early messages (AMPS_RECC_FLAG_EARLY_MESSAGES): their two kernels run behind that one
inline int capture_run_iq(CaptureState &c, RecordLists &L, TimingState &tm, hipStream_t s, const float2 *iq, uint64_t ld, uint32_t nsamp,
                          const PowerRing *pw = nullptr, const AutocorrRing *ac = nullptr, const SeizureState *sz = nullptr,
                          const EarlyState *ez = nullptr)
{
    c.origin_locked = true;
    if (nsamp == 0) return 0;
    const uint32_t avail = c.r_prev + nsamp;
    const uint32_t P = (avail / 64) * 64, r_new = avail - P;
    const FrontGeom geom = front_geometry(c.C, P, c.max_waves);
    const uint32_t Tc = geom.Tc, span = geom.span, nwaves = geom.nwaves;
    if (P && (uint64_t)(Tc + span - 1) / span + 1 > c.max_chunks) return -E2BIG;
    if (P) {
        FrontArgs fa = front_args(c, L, geom, c.r_prev, avail, P);
        fa.block = iq; fa.carry = c.carry[c.carry_cur].get(); fa.ld = ld;
        fa.force_ones = ((c.slicer == AMPS_SLICER_PRODUCT || c.slicer == AMPS_SLICER_EXACT) && c.n_done == c.origin) ? c.sps : 0u;   // specs B, D: no partner yet
        fa.dbg_d = c.dbg_d.get(); fa.dbg_S = c.dbg_S.get(); fa.dbg_channel = 0;
        fa.carry_out = c.carry[c.carry_cur ^ 1].get(); fa.carry_n = HALO + r_new;     // the next push's carry is written by the streaming kernel itself
        SpanGuard g(tm, s, c.wideband, T_FRONT, P);
        if (debug_sync_enabled())
            std::fprintf(stderr, "amps_recc[debug]: front waves=%u span=%u Tc=%u C=%u P=%u avail=%u r_prev=%u ld=%llu n_done=%llu ring_words=%u max_chunks=%u det_cap=%u\n",
                         nwaves, span, Tc, c.C, P, avail, c.r_prev, (unsigned long long)ld, (unsigned long long)c.n_done, c.ring_words, c.max_chunks, c.det_cap);
        const front_kernel_t k = front_kernel_for(c.sps, c.slicer, fa.tol != 0);
        if (!k) return -EINVAL;
        hipLaunchKernelGGL(k, dim3((nwaves + 3) / 4), dim3(256), 0, s, fa);
        if (pw || ac) g.end();                                    // outside the streaming kernel's span: T_FRONT times what it always timed
        if (pw) stream_power_launch(*pw, fa, s);
        if (ac) stream_autocorr_launch(*ac, fa, s);
    }
    if (int rc = debug_sync(s, "front")) return rc;
    if (!P) {                                              // a push too short for a 64-sample word only moves the carry
        CarryArgs ca{};
        ca.block = iq; ca.carry_in = c.carry[c.carry_cur].get(); ca.carry_out = c.carry[c.carry_cur ^ 1].get();
        ca.ld = ld; ca.r_prev = c.r_prev; ca.avail = avail; ca.P = P; ca.r_new = r_new;
        SpanGuard g(tm, s, c.wideband, T_CARRY);
        hipLaunchKernelGGL(recc_carry_kernel, dim3((HALO + r_new + 255) / 256, c.C), dim3(256), 0, s, ca);
    }
    if (int rc = debug_sync(s, "carry")) return rc;
    if (P) {
        launch_resolve(c, records_current(L), tm, geom, P, s);
        if (int rc = debug_sync(s, "resolve + capture")) return rc;
        if (sz) seizure_launch(*sz, c.pending.get(), c.gring.get(), c.ring_words, c.sps, c.n_done + P, s);
        if (int rc = debug_sync(s, "seizure events")) return rc;
        if (ez) early_launch(*ez, c.pending.get(), c.gring.get(), c.ring_words, c.sps, c.track, c.majority, c.n_done + P, s);
        if (int rc = debug_sync(s, "early messages")) return rc;
    }
    HIP_TRY(hipGetLastError());
    c.n_done += P;
    c.r_prev = r_new;
    c.carry_cur ^= 1;
    return 0;
}

// bit-domain tail of the fused wideband seam: the slicer bits of [n_done, n_done + P) are already in the ring
inline int capture_run_bits(CaptureState &c, RecordLists &L, TimingState &tm, hipStream_t s, uint32_t P, const SeizureState *sz = nullptr,
                            const EarlyState *ez = nullptr)
{
    if (P == 0) return 0;
    const FrontGeom geom = front_geometry(c.C, P, c.max_waves_bits);
    const uint32_t Tc = geom.Tc, span = geom.span, nwaves = geom.nwaves;
    const bool in_resolve = search_in_resolve(c.wideband, (bool)c.capq, c.sps);
    // round 6, the search in the resolve kernel: ONE launch -- every channel's workgroup searches its own slicer bits (a quarter of the push per wave,
    // hits in LDS), then resolves, captures and decodes them as ever; the launch's housekeeping goes with it
    uint32_t *zero2 = nullptr;
    if (in_resolve) zero2 = records_appending(L);
    else {
        if ((uint64_t)(Tc + span - 1) / span + 1 > c.max_chunks) return -E2BIG;
        const FrontArgs fa = front_args(c, L, geom, 0, P, P);
        SpanGuard g(tm, s, c.wideband, T_FRONT, P);
        hipLaunchKernelGGL(bits_kernel_for(c.sps, fa.tol != 0), dim3((nwaves + 3) / 4), dim3(256), 0, s, fa);
        g.end();
#ifdef BITS_TIMELINE
        if (const char *path = std::getenv("AMPS_RECC_BITS_TIMELINE")) {
            std::vector<unsigned long long> tl(3 * 16384);
            if (hipStreamSynchronize(s) == hipSuccess && hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(bits_tl), tl.size() * 8) == hipSuccess)
                if (FILE *f = std::fopen(path, "wb")) { unsigned long long nw = nwaves; std::fwrite(&nw, 8, 1, f); std::fwrite(tl.data(), 8, tl.size(), f); std::fclose(f); }
        }
#endif
    }
    launch_resolve(c, records_current(L), tm, geom, P, s, in_resolve, zero2);
    if (sz) seizure_launch(*sz, c.pending.get(), c.gring.get(), c.ring_words, c.sps, c.n_done + P, s);
    if (ez) early_launch(*ez, c.pending.get(), c.gring.get(), c.ring_words, c.sps, c.track, c.majority, c.n_done + P, s);
    HIP_TRY(hipGetLastError());
    c.n_done += P;
    return 0;
}

} // namespace amps
