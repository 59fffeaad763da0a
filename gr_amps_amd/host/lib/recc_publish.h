// recc_publish.h -- what recc_wideband, recc_subband and recc_fused do behind every push: drain the records with their bursts, ask for
// their burst power where the block keeps power and for their carrier offset where it measures that, and publish on "bursts",
// "records", "power" and "offset"; and, on a block made with seizure_events, in front of all that the push's seizure events on
// "seizures", and on a block made with early_messages the push's early messages on "early".  Internal to lib/.
#pragma once
#include <amps/api.h>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include "amps_recc.h"
#include "amps_recc_seizure.h"
#include "amps_recc_early.h"

namespace gr {
namespace amps {

// payload of the "power" port, behind the record's channel number
struct recc_power_payload { float mean_power; uint32_t n_snaps; };
static_assert(sizeof(recc_power_payload) == 8, "payload of the power port");
// payload of the "offset" port, behind the record's channel number (amps_recc_burst_offset)
struct recc_offset_payload { float offset_hz; uint32_t n_blocks; };
static_assert(sizeof(recc_offset_payload) == 8, "payload of the offset port");

// The seizure events held behind the push just made (AMPS_RECC_FLAG_SEIZURE_EVENTS), oldest first, each as
// pmt::cons(channel, blob(amps_recc_seizure_t)) on "seizures": called right behind the push and before recc_drain_and_publish, so an
// event goes out in front of that call's records -- and its own record comes with a later push.  false = stop the flow graph.
inline bool recc_publish_seizures(gr::basic_block &blk, const char *name, amps_recc_t *h)
{
    amps_recc_seizure_t ev[64];
    size_t n = 0, left = 0;
    do {
        const int rc = amps_recc_drain_seizures(h, ev, sizeof(ev) / sizeof(ev[0]), &n, &left);
        if (rc == -ENOSPC) std::fprintf(stderr, "amps::%s: %s (seizure events dropped, continuing)\n", name, amps_recc_strerror(rc));
        else if (rc != 0) { std::fprintf(stderr, "amps::%s: seizure events: %s\n", name, amps_recc_strerror(rc)); return false; }
        for (size_t i = 0; i < n; i++)
            blk.message_port_pub(pmt::mp("seizures"), pmt::cons(pmt::from_long((long)ev[i].channel), pmt::mp(&ev[i], sizeof(ev[i]))));
    } while (left);
    return true;
}

// The early messages held behind the push just made (AMPS_RECC_FLAG_EARLY_MESSAGES), oldest first, each as
// pmt::cons(channel, blob(amps_recc_early_t)) on "early" -- the record of the message's announced words, n_words and found_at: called
// behind recc_publish_seizures and before recc_drain_and_publish, so a message goes out in front of that call's records, and the record
// that repeats it (same channel, same position) comes with a later push.  false = stop the flow graph.
inline bool recc_publish_early(gr::basic_block &blk, const char *name, amps_recc_t *h)
{
    amps_recc_early_t ev[16];
    size_t n = 0, left = 0;
    do {
        const int rc = amps_recc_drain_early(h, ev, sizeof(ev) / sizeof(ev[0]), &n, &left);
        if (rc == -ENOSPC) std::fprintf(stderr, "amps::%s: %s (early messages dropped, continuing)\n", name, amps_recc_strerror(rc));
        else if (rc != 0) { std::fprintf(stderr, "amps::%s: early messages: %s\n", name, amps_recc_strerror(rc)); return false; }
        for (size_t i = 0; i < n; i++)
            blk.message_port_pub(pmt::mp("early"), pmt::cons(pmt::from_long((long)ev[i].rec.channel), pmt::mp(&ev[i], sizeof(ev[i]))));
    } while (left);
    return true;
}

// What differs between the blocks: the name in the stderr lines, and whether "bursts" and "records" carry (channel, blob) pairs
// or the bare blob (recc_fused: one channel, and what gr::amps::recc publishes).  recs / bursts hold `cap` records; pow / nsnap hold as
// many, or are null on a block that keeps no power; off_hz / off_n likewise on a block that measures no carrier offset.  false = stop
// the flow graph (the caller knows what that takes).
inline bool recc_drain_and_publish(gr::basic_block &blk, const char *name, bool channel_pairs, amps_recc_t *h, amps_recc_burst_t *recs,
                                   unsigned char *bursts, size_t cap, float *pow, uint32_t *nsnap, float *off_hz = nullptr,
                                   uint32_t *off_n = nullptr)
{
    size_t nrec = 0;
    int rc = amps_recc_drain_bursts(h, recs, bursts, cap, &nrec);
    // -ENOSPC: more bursts than the list holds were found; the ones that fit are returned and the list recovers on the
    // next push -- a recoverable condition must not end the flow graph
    if (rc == -ENOSPC) std::fprintf(stderr, "amps::%s: %s (bursts dropped, continuing)\n", name, amps_recc_strerror(rc));
    else if (rc != 0) { std::fprintf(stderr, "amps::%s: %s\n", name, amps_recc_strerror(rc)); return false; }
    // the push that found a record has just been drained: its capture is inside the power ring's window
    if (pow && nrec) {
        rc = amps_recc_burst_power(h, recs, nrec, pow, nsnap);
        if (rc != 0) { std::fprintf(stderr, "amps::%s: burst power: %s\n", name, amps_recc_strerror(rc)); return false; }
    }
    if (off_hz && nrec) {                          // likewise the window of the autocorrelation sums
        rc = amps_recc_burst_offset(h, recs, nrec, off_hz, off_n);
        if (rc != 0) { std::fprintf(stderr, "amps::%s: burst offset: %s\n", name, amps_recc_strerror(rc)); return false; }
    }
    for (size_t i = 0; i < nrec; i++) {
        const pmt::pmt_t ch = pmt::from_long((long)recs[i].channel);
        const pmt::pmt_t burst = pmt::mp(bursts + i * AMPS_RECC_CAPTURE_SYMS, AMPS_RECC_CAPTURE_SYMS), rec = pmt::mp(&recs[i], sizeof(recs[i]));
        blk.message_port_pub(pmt::mp("bursts"), channel_pairs ? pmt::cons(ch, burst) : burst);
        blk.message_port_pub(pmt::mp("records"), channel_pairs ? pmt::cons(ch, rec) : rec);
        if (pow) {
            const recc_power_payload p = { pow[i], nsnap[i] };
            blk.message_port_pub(pmt::mp("power"), pmt::cons(ch, pmt::mp(&p, sizeof(p))));
        }
        if (off_hz) {
            const recc_offset_payload p = { off_hz[i], off_n[i] };
            blk.message_port_pub(pmt::mp("offset"), pmt::cons(ch, pmt::mp(&p, sizeof(p))));
        }
    }
    return true;
}

} // namespace amps
} // namespace gr
