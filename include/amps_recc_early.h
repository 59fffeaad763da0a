/* amps_recc_early.h -- EARLY MESSAGES: an extension of the C ABI of amps_recc.h (same library, same handle, ABI version 4), in a header of
 * its own, beside amps_recc_seizure.h: the flag, the event and the one entry point below.  Include it beside, or instead of, amps_recc.h. */
#ifndef AMPS_RECC_EARLY_H
#define AMPS_RECC_EARLY_H

#include "amps_recc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* amps_recc_cfg_t.flags: the bit behind AMPS_RECC_FLAG_SEIZURE_EVENTS */
#define AMPS_RECC_FLAG_EARLY_MESSAGES 0x4000u /* IQ, translate and wideband seams: keep a list of EARLY MESSAGES beside the record lists, one
                                               per seizure whose word A announces fewer than seven words, available after the push in
                                               which the last repeat of its last announced word arrived (amps_recc_drain_early below,
                                               where the contract stands).  Off by default; with it off nothing is allocated or launched
                                               for it.  It changes no record, no kept blob, no ring and no timing span, and combines with
                                               every other flag.  With max_samples_per_push == 0 (symbol seam only): -EINVAL */

/* ---- early messages (handles created with AMPS_RECC_FLAG_EARLY_MESSAGES; -ENOSYS without) ----
 * A record leaves the library once its whole capture is in: 3374 symbols, 169 ms, behind the trigger, whatever the mobile sent.  The
 * length of a RECC message stands in its first word: word A carries NAWC, and the message is NAWC + 1 words of five repeats each.  A
 * page response is two words, a registration three: their last repeat is in 49 or 73 ms behind the trigger.  An EARLY MESSAGE is the
 * record of those words, decoded by the same capture walk and the same decode core as the record that follows: ONE EVENT PER SEIZURE,
 * AVAILABLE AFTER THE PUSH IN WHICH THE LAST REPEAT OF ITS LAST ANNOUNCED WORD ARRIVED, on every data seam (IQ, translate, wideband).
 *
 * Why it is exact.  The capture's timing walk is causal: the sampling delay of block b of the walk (block 0 the trigger, block 1 the
 *   coded DCC with repeat 0 of word A, blocks 2 ... 35 the other repeats) depends on blocks <= b only.  A prefix of the walk over the
 *   slicer bits received so far therefore gives exactly the prefix of the capture the record will be decoded from.
 * Rule.  Behind the resolve of every push run two small kernels on the handle's stream (recc_early_wave_kernel, recc_early_scan_kernel;
 *   they read the slicer-bit ring and write nothing the other kernels read).  After the resolve of a push, let c be a channel whose
 *   capture p is still PENDING (an accepted trigger whose tail has not been received yet) and n_proc the samples processed.  Let
 *   T(n) = p + sps (15 + 480 n) + K, with K = AMPS_TRACK_BLOCKS where the capture tracks the bit clock and 0 under
 *   AMPS_RECC_FLAG_FIXED_TIMING.  (T(7) is the span a record waits for: a seven-word message never has an event, its record is there
 *   in the same push.)
 *   1. Once T(1) < n_proc, word A is in.  The walk runs over blocks 0 ... 5, then the handle's decode mode (reference or
 *      AMPS_RECC_FLAG_MAJORITY) decodes word A.  valid[0] == 0, or a_NAWC + 1 >= 7: this capture never has an event.  Otherwise
 *      n_words = a_NAWC + 1.
 *   2. In the first push after which T(n_words) < n_proc with p still pending, one event is appended and p is remembered as reported.
 *      found_at = n_proc of that push.
 *   3. rec is the decode core's record (in the handle's decode mode) of the capture's bit string at the walk's delays over blocks
 *      0 ... 5 n_words, with every bit of the words >= n_words zero and their manch_bad zero.  Behind the core, valid[w] = 0 and
 *      first_valid_rep[w] = 5 for w >= n_words.  channel and position are the record's.
 *   4. The events of one push are appended in channel order, so the list is ordered by (found_at, channel); what an overflow keeps is
 *      therefore the same on every run.
 * Relation to the record.  Every event is followed, in a LATER push, by exactly one record R with its (channel, position), unless the
 *   stream ends or amps_recc_reset comes first.  Identical to R's are: dcc and dcc_bad; every a_* field; and for w < n_words
 *   manch_bad[w], valid[w], first_valid_rep[w], word_raw[w] and word_dec[w].  Where R's parse consumed no word >= n_words (every
 *   well-formed message), all parsed fields are R's and amps_recc_reply_words(&rec) is byte for byte amps_recc_reply_words(R).  A
 *   caller that answers from the early message drops the later record by (channel, position).
 * With AMPS_RECC_FLAG_SEIZURE_EVENTS on the same handle a capture's early message never precedes its seizure event.
 * Capacity.  The list holds cfg.max_bursts events between drains; later ones are dropped, and the next drain answers -ENOSPC after
 *   delivering what is held (as amps_recc_drain does for records).
 * amps_recc_reset empties the list and forgets what was reported.  On distributed handles events stay rank-local:
 * amps_recc_drain_gather does not carry them.  A channel-group handle numbers `channel` (the event's rec.channel) as its records.
 *
 * amps_recc_drain_early waits (bounded, as every drain) for the pushes enqueued so far, copies the oldest min(cap, held) events,
 * ordered by (found_at, channel), into out, removes them, and reports in *nleft (may be NULL) how many stay.  It is independent of the
 * record lists and of an open split drain.  -EINVAL for a null handle or null nout, or out == NULL with cap > 0; -ENOSYS on a handle
 * without the flag; -ESTALE as the data seams; -ENOSPC as above. */
typedef struct amps_recc_early {
    amps_recc_burst_t rec;   /* the record of the first n_words words (rule 3)                                       */
    uint64_t found_at;       /* samples processed after the push that completed the message, numbered as rec.position */
    uint32_t n_words;        /* words the message announced: a_NAWC + 1, 1 ... 6                                      */
    uint32_t _pad;
} amps_recc_early_t;
#define AMPS_RECC_EARLY_BYTES 744
int amps_recc_drain_early(amps_recc_t *h, amps_recc_early_t *out, size_t cap, size_t *nout, size_t *nleft);

#ifdef __cplusplus
}
#endif

#endif /* AMPS_RECC_EARLY_H */
