// recc_timing.hip.h -- kernel timing (AMPS_RECC_FLAG_TIME_KERNELS, amps_recc_set_timing / amps_recc_get_timing): pairs of events round
// the launches of a handle, collected into per-stage sums once they have completed.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "amps_recc.h"
#include "recc_devmem.hip.h"

namespace amps {

enum { T_FRONT = 0, T_RESOLVE, T_DECODE, T_CARRY, T_SYMBOLS, T_CHANNELIZER, T_XLATE, T_COUNT };

struct TimedSpan { Event a, b; int tag; uint64_t samples; };

struct TimingState {
    int mode = AMPS_RECC_TIMING_OFF;  // AMPS_RECC_TIMING_*
    uint32_t dominant_tick = 0;       // launches of the dominant kernel seen in DOMINANT_SAMPLED mode
    double ms[T_COUNT] = { 0 };
    uint32_t launches_front = 0, launches_chz = 0;
    uint64_t samples_front = 0;
    // the spans in flight with their events (one that is never collected goes with the state) and the spare events
    std::vector<TimedSpan> spans;
    std::vector<Event> event_pool;    // recycled by collect_spans
};

struct SpanGuard {   // records a pair of events around a launch when timing is on
    TimingState *t; hipStream_t s; int tag; uint64_t samples; Event a, b; bool on;
    static Event take(TimingState &t)   // a spare event, or a new one
    {
        Event e;
        if (t.event_pool.empty()) (void)e.create();
        else { e = std::move(t.event_pool.back()); t.event_pool.pop_back(); }
        return e;
    }
    SpanGuard(TimingState &t_, hipStream_t s_, bool wideband, int tag_, uint64_t samples_ = 0) : t(&t_), s(s_), tag(tag_), samples(samples_), on(t_.mode != AMPS_RECC_TIMING_OFF)
    {
        // "dominant" mode: only the streaming kernel of the seam (front kernel, or the channelizer on the wideband
        // seam) is bracketed -- two event records per push instead of ten, for timed regions that should not be perturbed
        if (on && t->mode >= AMPS_RECC_TIMING_DOMINANT) on = (tag == T_CHANNELIZER) || (tag == T_FRONT && !wideband);
        if (on && t->mode == AMPS_RECC_TIMING_DOMINANT_SAMPLED) on = (t->dominant_tick++ % AMPS_RECC_TIMING_SAMPLE_PERIOD) == 0;
        if (!on) return;
        a = take(*t); b = take(*t);
        if (!a || !b) { on = false; return; }
        (void)hipEventRecord(a.get(), s);
    }
    void end()     // close the span now (the destructor then does nothing)
    {
        if (!on) return;
        (void)hipEventRecord(b.get(), s);
        t->spans.push_back({ std::move(a), std::move(b), tag, samples });
        on = false;
    }
    static void end_cb(void *g) { static_cast<SpanGuard *>(g)->end(); }
    ~SpanGuard() { end(); }
};

inline void collect_spans(TimingState &t)   // collects the spans whose events have completed (all of them after a stream sync)
{
    size_t keep = 0;
    for (auto &s : t.spans) {
        if (hipEventQuery(s.b.get()) != hipSuccess) { t.spans[keep++] = std::move(s); continue; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a.get(), s.b.get()) == hipSuccess) {
            t.ms[s.tag] += ms;
            if (s.tag == T_FRONT) { t.launches_front++; t.samples_front += s.samples; }
            if (s.tag == T_CHANNELIZER) t.launches_chz++;
        }
        t.event_pool.push_back(std::move(s.a));
        t.event_pool.push_back(std::move(s.b));
    }
    t.spans.resize(keep);
}

inline void timing_set_mode(TimingState &t, int mode) { t.mode = mode; t.dominant_tick = 0; }

#if defined(CHZ_TIMELINE) || defined(RESOLVE_TIMELINE)
// Host side of the timeline builds (-DCHZ_TIMELINE: scripts/chz_timeline.py, -DRESOLVE_TIMELINE: scripts/resolve_timeline.py): the
// device buffer a kernel writes its clock stamps into.  The file is the stamps as they lie in the buffer, 8 bytes each, no header.
struct TimelineBuf {
    DevBuf<unsigned long long> dev;
    // the buffer -- `cap` stamps, allocated at the first call -- with its first n stamps cleared on the stream; null if it cannot be had
    unsigned long long *clear(size_t cap, size_t n, hipStream_t s)
    {
        if (n > cap || (!dev && dev.alloc(cap))) return nullptr;
        (void)hipMemsetAsync(dev.get(), 0, n * 8, s);
        return dev.get();
    }
    // if the environment variable `env` names a file: wait for the stream, copy the first n stamps back and write them there
    void dump(const char *env, size_t n, hipStream_t s) const
    {
        const char *path = std::getenv(env);
        if (!path) return;
        std::vector<unsigned long long> tl(n);
        if (hipStreamSynchronize(s) == hipSuccess && hipMemcpy(tl.data(), dev.get(), n * 8, hipMemcpyDeviceToHost) == hipSuccess)
            if (FILE *f = std::fopen(path, "wb")) { std::fwrite(tl.data(), 8, n, f); std::fclose(f); }
    }
};
#endif

} // namespace amps
