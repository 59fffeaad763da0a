/* amps_recc_seizure.h -- SEIZURE EVENTS: an extension of the C ABI of amps_recc.h (same library, same handle, ABI version 4), in a header
 * of its own: the flag, the event and the one entry point below.  Include it beside, or instead of, amps_recc.h. */
#ifndef AMPS_RECC_SEIZURE_H
#define AMPS_RECC_SEIZURE_H

#include "amps_recc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* amps_recc_cfg_t.flags: the bit behind AMPS_RECC_FLAG_STREAM_OFFSET_UNIT */
#define AMPS_RECC_FLAG_SEIZURE_EVENTS 0x2000u /* IQ, translate and wideband seams: keep a list of SEIZURE EVENTS beside the record lists, one
                                               per seizure, available after the push in which its trigger was accepted
                                               (amps_recc_drain_seizures below, where the contract stands).  Off by default; with it off
                                               nothing is allocated or launched for it.  It changes no record, no kept blob, no ring and no
                                               timing span.  With max_samples_per_push == 0 (symbol seam only): -EINVAL */

/* ---- seizure events (handles created with AMPS_RECC_FLAG_SEIZURE_EVENTS; -ENOSYS without) ----
 * A record leaves the library once its whole capture is in: 3374 symbols, 169 ms, behind the trigger.  A base station has to set
 * the FOCC busy-idle bits while the mobile is still sending its seizure precursor; what it needs for that -- a seizure has begun, on
 * which channel, with which DCC -- is known as soon as the trigger is accepted.  A SEIZURE EVENT says so: ONE EVENT PER SEIZURE,
 * AVAILABLE AFTER THE PUSH IN WHICH ITS TRIGGER WAS ACCEPTED, on every data seam (IQ, translate, wideband).
 *
 * Rule.  Behind the resolve of every push runs one small kernel on the handle's stream (recc_seizure_kernel; it reads the slicer-bit
 *   ring and writes nothing the other kernels read).  For every channel c let p be the capture that channel has PENDING after the
 *   push -- an accepted trigger whose tail has not been received yet -- and n_proc the samples processed after it.  If there is one
 *   and p is not the capture last reported for c, one event is appended and p is remembered as reported.
 * Order.  The events of one push are appended in channel order, so the list is ordered by (found_at, channel); what an overflow keeps
 *   is therefore the same on every run.
 * Event.  channel and position are those of the record that will follow (position = p, numbered as amps_recc_burst_t.position);
 *   found_at = n_proc of that push in the same numbering.
 * Early DCC.  Read at the trigger's own timing (delay 0, the rule of AMPS_RECC_FLAG_FIXED_TIMING for the capture's first block):
 *   symbols s_i = the slicer bit at p + sps (i + 1), i = 0 ... 13; dcc[j] = !s_2j; dcc_bad = the number of pairs with s_2j == s_2j+1
 *   (manchester_decode_binbuf on those 14 symbols).  AMPS_SEIZURE_FLAG_DCC_COMPLETE is set iff p + 14 sps < n_proc; otherwise dcc and
 *   dcc_bad are zero and the flag is clear.  An event is NOT held back for its DCC (only from 5 samples per symbol on can it be
 *   incomplete): a caller that needs it reads it from the record.  A capture that tracks the bit clock may sample the record's DCC
 *   one sample away from the event's.
 * Relation to records.  Every event is followed, in a LATER push, by exactly one record with the same (channel, position), unless
 *   the stream ends or amps_recc_reset comes first.  A capture whose tail was already complete in the push that found its trigger
 *   (pushes longer than a burst) has no event: its record is there at once.
 * Delay bound.  found_at - position < P + 128, P the samples that push processed: a run start is looked at once the 64-sample word
 *   behind its own is in, which is at most 64 samples behind the end of the push before, and position is never in front of its
 *   run's start.
 * Capacity.  The list holds cfg.max_bursts events between drains; later ones are dropped, and the next drain answers -ENOSPC after
 *   delivering what is held (as amps_recc_drain does for records).
 * amps_recc_reset empties the list and forgets what was reported.  On distributed handles events stay rank-local:
 * amps_recc_drain_gather does not carry them.  A channel-group handle numbers `channel` as its records.
 *
 * amps_recc_drain_seizures waits (bounded, as every drain) for the pushes enqueued so far, copies the oldest min(cap, held) events,
 * ordered by (found_at, channel), into out, removes them, and reports in *nleft (may be NULL) how many stay.  It is independent of the
 * record lists and of an open split drain.  -EINVAL for a null handle or null nout, or out == NULL with cap > 0; -ENOSYS on a handle
 * without the flag; -ESTALE as the data seams; -ENOSPC as above. */
#define AMPS_SEIZURE_FLAG_DCC_COMPLETE 0x1u
typedef struct amps_recc_seizure {
    uint32_t channel;        /* as amps_recc_burst_t.channel of the record that follows                                  */
    uint32_t flags;          /* AMPS_SEIZURE_FLAG_*                                                                      */
    uint64_t position;       /* as amps_recc_burst_t.position of the record that follows                                 */
    uint8_t  dcc[7];         /* the coded DCC at the trigger's own timing (AMPS_SEIZURE_FLAG_DCC_COMPLETE), else zeros   */
    uint8_t  dcc_bad;        /* its bad Manchester pairs                                                                 */
    uint64_t found_at;       /* samples processed after the push that accepted the trigger, numbered as position         */
} amps_recc_seizure_t;
#define AMPS_RECC_SEIZURE_BYTES 32
int amps_recc_drain_seizures(amps_recc_t *h, amps_recc_seizure_t *out, size_t cap, size_t *nout, size_t *nleft);

#ifdef __cplusplus
}
#endif

#endif /* AMPS_RECC_SEIZURE_H */
