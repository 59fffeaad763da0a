/* amps_recc.h -- C ABI of the MI355X-native AMPS reverse-control-channel (RECC) receive path.
 *
 * This is the drop-in boundary.  Every entry point replaces one
 * interface of the reference (unsynchronized/gr-amps); citations are file:line under the
 * reference tree:
 *
 *   amps_recc_push_symbols      <-  gr::amps::recc_impl::work            lib/recc_impl.cc:93-145
 *                                   (io signature: 1 x unsigned char in, lib/recc_impl.cc:71-73;
 *                                    "bursts" blob of 3374 bytes out,    lib/recc_impl.cc:82,126)
 *   amps_recc_decode_bursts     <-  recc_decode_impl::bursts_message     lib/recc_decode_impl.cc:81-169
 *                                   recc_decode_impl::recc_bch_decode    lib/recc_decode_impl.cc:53-79
 *                                   manchester_decode_binbuf             lib/utils.cc:27-59
 *                                   recc_word_a/_b/_c_serial/_called     lib/amps_packet.h:103-274
 *                                   extract_min_3 / calc_min             lib/amps_packet.h:277-302,354-366
 *   amps_recc_push_iq / _drain  <-  the flow-graph sub-chain  quadrature_demod_cf -> clock_recovery_mm_ff
 *                                   -> binary_slicer_fb -> amps_recc -> amps_recc_decode
 *                                   (grc/recctest.grc:458,846-874,807,310,349 and connections :3238-3274)
 *   amps_recc_push_wideband     <-  N x (freq_xlating_fir_filter_ccc -> the chain above), one per 30 kHz
 *                                   channel (grc/recctest.grc:889-937, taps :115-155); polyphase channelizer
 *                                   front end: M = 1024 branches at fs = 30.72 Msps, 8 taps per branch,
 *                                   D = 768 (40 ksps per channel, samples_per_symbol = 2; the default) or
 *                                   D = 512 (60 ksps, samples_per_symbol = 3): the two geometries
 *                                   amps_recc_create accepts (anything else: -EINVAL)
 *   amps_recc_reply_words       <-  handle_response / handle_registration / handle_origination
 *                                   lib/recc_decode_impl.cc:181-272 + word builders lib/amps_packet.cc:26-95
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative errno-style
 * code (never throws, never aborts); one handle is single-threaded (same rule as a GNU Radio block,
 * SURVEY.md 8b "Threading"); all compute runs in hand-written HIP kernels on the handle's device --
 * there is NO CPU fallback: without a usable HIP device amps_recc_create() fails with -ENODEV.
 */
#ifndef AMPS_RECC_H
#define AMPS_RECC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMPS_RECC_ABI_VERSION 4   /* 2: amps_recc_cfg_t gained wideband_groups / wideband_group; 3: default slicer = spec D, captures track the bit
                                     clock unless AMPS_RECC_FLAG_FIXED_TIMING, amps_recc_rccl_* / _push_wideband_bcast / _drain_gather / _debug_exact_slice added;
                                     4: amps_recc_push_wideband_dist (scatter + all-gather), amps_recc_rccl_info / _abort / _set_timeout; rccl_init checks the
                                     group split and allocates; every collective entry is bounded and carries a status word;
                                     (still 4, one entry point added and nothing changed: amps_recc_push_wideband_short, 16-bit I/Q through the wideband seam;
                                     still 4, three entry points and a flag added and nothing changed: amps_recc_channel_power / _burst_power /
                                     _power_ring_snaps behind AMPS_RECC_FLAG_CHANNEL_POWER;
                                     still 4, three entry points added and nothing changed: amps_recc_set_xlate_shared / _push_raw_shared /
                                     _debug_xlate_shared, many channels of one shared narrowband stream;
                                     still 4, four entry points added and nothing changed: amps_recc_push_raw_shared_as / _push_raw_as /
                                     _debug_xlate_shared_as / _debug_xlate_as, the translate seams on an SDR's integer samples (AMPS_RECC_SAMPLES_*);
                                     still 4, one entry point added and nothing changed: amps_recc_xlate_shared_plan, with the shared translate seam's
                                     decimations 5, 6, 10, 12, 16 and 20;
                                     still 4, two entry points added and nothing changed: amps_recc_set_xlate_resampled / amps_recc_xlate_resample_plan,
                                     the shared translate seam behind a rational L / M resampler;
                                     still 4, a flag added and nothing changed: AMPS_RECC_FLAG_STREAM_POWER, received power on the IQ and
                                     translate seams through amps_recc_channel_power / _burst_power / _power_ring_snaps;
                                     still 4, a flag and three entry points added and nothing changed: AMPS_RECC_FLAG_STREAM_OFFSET, carrier offset
                                     on the IQ and translate seams through amps_recc_channel_autocorr / _burst_autocorr / _burst_offset;
                                     still 4, a flag and one entry point added and nothing changed: AMPS_RECC_FLAG_STREAM_OFFSET_UNIT, the
                                     unit-amplitude statistic behind the same three entry points, and amps_recc_retune_xlate;
                                     still 4, one entry point added and nothing changed: amps_recc_wideband_plan, with cfg.wideband_channels = 512,
                                     256 and 128, the wideband seam at 15.36, 7.68 and 3.84 Msps;
                                     still 4, two entry points added and nothing changed: amps_recc_push_wideband_as / _debug_channelize_as, the
                                     wideband seam on 8-bit I/Q (sc8, cu8), read in place on every bank;
                                     still 4, one entry point added and nothing changed: amps_recc_wideband_grid_plan, with cfg.wideband_channels =
                                     2500, 2000, 1000 and 500 at wideband_decim = M / 4, the wideband seam at 25, 20, 10 and 5 Msps;
                                     still 4, two entry points added and nothing changed: amps_recc_set_wideband_shift / amps_recc_wideband_shift,
                                     a tuner's frequency error corrected inside the banks below 1024 branches;
                                     still 4, three entry points added and nothing changed: amps_recc_set_wideband_resample /
                                     amps_recc_wideband_resample_plan / amps_recc_debug_wideband_resample, an L / M resampler in front of the
                                     banks for the rates that are no bank's: 8, 12.5, 16, 6, 4 and 3.2 Msps;
                                     still 4, nothing changed in this header: a flag and one entry point in a header of their own,
                                     amps_recc_seizure.h -- one event per seizure after the push in which its trigger was accepted;
                                     still 4, nothing changed in this header: a flag and one entry point in a header of their own,
                                     amps_recc_early.h -- a message's announced words as soon as the last of them is in) */

/* protocol constants of the reference */
#define AMPS_RECC_TRIGGER_SYMS 74   /* lib/recc_impl.cc:76-77: 37 bits x 2 Manchester symbols   */
#define AMPS_RECC_CAPTURE_SYMS 3374 /* lib/recc_impl.cc:70: (7 + 7*240) bits x 2                */
#define AMPS_RECC_WORDS        7    /* lib/recc_decode_impl.cc:92                                */
#define AMPS_RECC_REPEATS      5    /* lib/recc_decode_impl.cc:101                               */
#define AMPS_RECC_WORD_BITS    48   /* BCH(48,36) = BCH(63,51) shortened by 15                   */
#define AMPS_RECC_MSG_BITS     36
#define AMPS_RECC_SYMBUF       65536 /* lib/recc_impl.cc:68 d_symbufsz                           */
#define AMPS_RECC_WINDOW       4096  /* lib/recc_impl.cc:69 d_windowsz                           */
#define AMPS_RECC_MAX_WORK_ITEMS 61439 /* lib/recc_impl.cc:103: noutput_items < bufsz - windowsz */

/* where a data pointer lives */
#define AMPS_MEM_HOST   0
#define AMPS_MEM_DEVICE 1

/* amps_recc_cfg_t.flags */
#define AMPS_RECC_FLAG_TIME_KERNELS 0x1u /* record HIP events around every kernel (amps_recc_get_timing) */
#define AMPS_RECC_FLAG_UNFUSED_WIDEBAND 0x4u /* channelizer seam: keep the channel-major intermediate in HBM (two kernels)
                                               instead of fusing the RECC front end behind the FFT; same results */
#define AMPS_RECC_FLAG_SLICER_PRODUCT 0x8u /* IQ / wideband seams: slicer spec B of amps_recc_numerics.h (sign of
                                               Im(x[n] conj(x[n-sps])), the telescoped form of discriminator + boxcar) */
#define AMPS_RECC_FLAG_SLICER_SINE  0x10u /* IQ / wideband seams: slicer spec C (boxcar over Im(x[n] conj(x[n-1])): spec A without the
                                               arctangent) */
#define AMPS_RECC_FLAG_SLICER_EXACT 0x80u /* IQ / wideband seams: slicer spec D (the sign of spec A's boxcar sum computed exactly from sign
                                               bits and the winding number: spec A's decisions at spec C's cost).  At most one of the four
                                               SLICER flags may be set */
#define AMPS_RECC_FLAG_SLICER_ATAN  0x40u /* IQ / wideband seams: slicer spec A (arctangent discriminator + boxcar), explicitly.
                                               With no SLICER flag a handle uses amps_recc_default_slicer() */
#define AMPS_RECC_FLAG_KEEP_BURSTS  0x20u /* IQ / wideband seams: also keep the 3374 captured symbol bytes of every burst (what
                                               gr::amps::recc publishes on "bursts", lib/recc_impl.cc:126) for amps_recc_drain_bursts */
#define AMPS_RECC_FLAG_FIXED_TIMING 0x100u /* IQ / wideband seams: sample all 3374 symbols of a capture at the one phase the trigger run
                                               gives (rounds 1-3).  Default: the capture tracks the mobile's bit clock, one sample per
                                               repeat at most, from where the mid-bit transitions fall -- the fast path's
                                               stand-in for clock_recovery_mm_ff's loop (grc/recctest.grc:846-874) */
#define AMPS_RECC_FLAG_CHANNEL_POWER 0x200u /* wideband seam, fused form: keep per-channel received power (amps_recc_channel_power,
                                               amps_recc_burst_power below).  Off by default; with it off nothing is allocated or launched for it.
                                               With AMPS_RECC_FLAG_UNFUSED_WIDEBAND, on a handle without wideband_channels, or with
                                               wideband_channels < 1024 (its snapshot kernel is the 1024 bank's): -EINVAL */
#define AMPS_RECC_FLAG_STREAM_POWER 0x400u /* IQ and translate seams: keep per-channel received power (the same three entry points; the
                                               definition for these seams stands below theirs).  Off by default; with it off nothing is
                                               allocated or launched for it and no record changes.  Also taken by a wideband handle with
                                               wideband_channels < 1024, whose block goes through the IQ seam.  On a handle with
                                               wideband_channels = 1024 (fused or not), with max_samples_per_push == 0 (symbol seam only), or
                                               together with AMPS_RECC_FLAG_CHANNEL_POWER: -EINVAL */
#define AMPS_RECC_FLAG_STREAM_OFFSET 0x800u /* IQ and translate seams: keep the per-channel lag-one autocorrelation sums from which a burst's
                                               carrier offset is read (amps_recc_channel_autocorr, amps_recc_burst_autocorr,
                                               amps_recc_burst_offset below).  Off by default; with it off nothing is allocated or launched
                                               for it and no record changes.  Combines freely with AMPS_RECC_FLAG_STREAM_POWER.  Also taken
                                               with wideband_channels < 1024 (fs = 30 kHz M / D there) and with the banks of 10 kHz bins (fs = 40 kHz).  On a handle with wideband_channels
                                               = 1024 (fused or not), with max_samples_per_push == 0 (symbol seam only), or together with
                                               AMPS_RECC_FLAG_CHANNEL_POWER: -EINVAL */
#define AMPS_RECC_FLAG_STREAM_OFFSET_UNIT 0x1000u /* the same ring, entry points, numbering, window and error rules as
                                               AMPS_RECC_FLAG_STREAM_OFFSET, holding the UNIT-AMPLITUDE statistic U instead of A (defined
                                               with the entry points below): the one to use behind a translate seam's channel filter, the
                                               default 10 kHz one included.  Off by default; with it off nothing is allocated or launched
                                               for it and no record changes.  A handle keeps one offset ring with one statistic: both
                                               offset flags together are -EINVAL, as is every combination AMPS_RECC_FLAG_STREAM_OFFSET
                                               refuses.  Combines freely with AMPS_RECC_FLAG_STREAM_POWER */
/* (bit 0x2000u is AMPS_RECC_FLAG_SEIZURE_EVENTS of the extension header amps_recc_seizure.h: seizure events, amps_recc_drain_seizures) */
/* (bit 0x4000u is AMPS_RECC_FLAG_EARLY_MESSAGES of the extension header amps_recc_early.h: early messages, amps_recc_drain_early) */
#define AMPS_RECC_FLAG_MAJORITY    0x2u /* decode mode "majority" instead of "reference" (SURVEY.md 8f.2), see below */

/* message classes, the branches of lib/recc_decode_impl.cc:108-168 */
enum amps_recc_msg_class {
    AMPS_MSG_INVALID_WORD_A = 0, /* validwords[0]==false  -> dropped   (:108-111) */
    AMPS_MSG_E_ZERO         = 1, /* worda.E==false        -> dropped   (:113-116) */
    AMPS_MSG_PAGE_RESPONSE  = 2, /* handle_response                    (:121-122) */
    AMPS_MSG_REGISTRATION   = 3, /* handle_registration                (:123-138) */
    AMPS_MSG_ORIGINATION    = 4, /* handle_origination                 (:139-165) */
    AMPS_MSG_BAD_NAWC       = 5, /* origination with nawc outside 1..4 (:155-158) */
    AMPS_MSG_UNKNOWN        = 6  /* "got unknown RECC message"         (:166-168) */
};

/* Decode modes.
 * reference (default): exactly lib/recc_decode_impl.cc:96-117 -- the five repeats are BCH-decoded in order and
 *   the first that decodes wins; only validwords[0] gates; fields are parsed from the RAW repeat 0.
 * majority (AMPS_RECC_FLAG_MAJORITY): what TIA/EIA-553 specifies and the reference leaves as "XXX" -- each of
 *   the 48 bit positions of a word is a 3-of-5 vote over the repeats; the voted word is BCH-decoded once and is
 *   valid only if it decodes AND no correction falls into the 15 shortening positions; fields are parsed from the
 *   corrected bits; every word the dispatch reads must be valid; the 7-bit coded DCC must be within one bit of a
 *   code word.  In this mode word_raw = voted bits, first_valid_rep = number of repeats equal to the voted word.
 *   On error-free bursts both modes produce the same words, fields and class.
 *   In full: the vote is over the Manchester-decoded bits (dcc, dcc_bad and manch_bad are as in reference mode).  The
 *   IT++ three-root acceptance (S1 = 0, S3 a cube) counts as decoding, and its three positions are corrections like any
 *   other: one of them in the shortening positions makes the word invalid.  word_dec = the 36 message bits of the voted
 *   word, corrected where the word is valid (a correction in the parity leaves them alone) and as voted where it is
 *   not; the fields of such a word are parsed from the voted bits.  The dispatch is the reference's on these fields and
 *   valid[0]; the words it reads are A and B, word C where the registration or origination branch takes the serial
 *   number, and the called-address words the origination branch consumes.  If any of those is invalid and the class
 *   would be PAGE_RESPONSE or later, the class is AMPS_MSG_INVALID_WORD_A (has_esn, esn, dialed and n_called_words
 *   stay as the branch left them); INVALID_WORD_A and E_ZERO stand as they are.  AMPS_BURST_FLAG_DCC_INVALID is set
 *   when dcc[] differs in two or more of its 7 bits from each of 0000000, 0011111, 1100011, 1111100. */

/* amps_recc_burst_t.flags */
#define AMPS_BURST_FLAG_NONBINARY 0x1u /* a symbol byte outside {0,1} was seen (reference: assert(0), UB in Release) */
#define AMPS_BURST_FLAG_WORDC_NAWC_MISMATCH 0x2u /* "protocol violation" warning of :134-136 / :150-152 */
#define AMPS_BURST_FLAG_BAD_DIGIT 0x4u /* digit code 13..15 truncated a called-address word (amps_packet.h:219-223) */
#define AMPS_BURST_FLAG_DCC_INVALID 0x8u /* majority mode: coded DCC further than one bit from every code word */

/* One decoded seizure burst.  Bits are one byte per bit (0/1), MSB first, exactly as the reference
 * holds them (lib/recc_decode_impl.cc:92-95).  Layout is fixed: natural alignment, 728 bytes. */
typedef struct amps_recc_burst {
    uint32_t channel;        /* RECC instance index                                                     */
    uint32_t flags;          /* AMPS_BURST_FLAG_*                                                       */
    uint64_t position;       /* symbol seam: 0.  IQ seams: absolute sample index of the last trigger
                                symbol's decision instant (capture symbol i is sliced at position+sps*(i+1)) */
    uint8_t  dcc[7];         /* manchester_decode_binbuf(bdata, dcc, 7)            (:90)               */
    uint8_t  dcc_bad;        /* its return value (bad Manchester pairs)                                 */
    uint16_t manch_bad[AMPS_RECC_WORDS];                 /* errs[i]                 (:97)               */
    uint8_t  valid[AMPS_RECC_WORDS];                     /* validwords[w]           (:102)              */
    uint8_t  first_valid_rep[AMPS_RECC_WORDS];           /* r at the break, 5 if none valid            */
    uint8_t  word_raw[AMPS_RECC_WORDS][AMPS_RECC_WORD_BITS]; /* words[w][0..47]: repeat 0, uncorrected --
                                                            what the reference parses (:112,117,130,146,161) */
    uint8_t  word_dec[AMPS_RECC_WORDS][AMPS_RECC_MSG_BITS];  /* corrected message bits of the first valid
                                                            repeat; uncorrected bits of repeat 4 if none   */
    /* ---- parsed fields (lib/amps_packet.h:103-198), always from word_raw like the reference ---- */
    uint8_t  a_F, a_NAWC, a_T, a_S, a_E, a_ER, a_SCM, _pad0;
    uint32_t a_MIN1;
    uint8_t  b_F, b_NAWC, b_MSG_TYPE, b_ORDQ, b_ORDER, b_LT, b_EP, b_SCM4, b_MPCI, b_SDCC1, b_SDCC2, _pad1;
    uint16_t b_MIN2;
    uint16_t _pad2;
    uint32_t esn;            /* recc_word_c_serial::SERIAL when read, else 0                            */
    uint8_t  has_esn;        /* registration: worda.S (:128); origination: worda.S (:145)               */
    uint8_t  msg_class;      /* enum amps_recc_msg_class                                                */
    uint8_t  n_called_words; /* origination: number of called-address words consumed                    */
    uint8_t  _pad3;
    char     min[12];        /* calc_min(): 10 digits, NUL padded                                        */
    char     dialed[36];     /* concatenated recc_word_called::digits(), NUL padded (<= 32 chars)        */
    uint32_t _pad4;
} amps_recc_burst_t;
#define AMPS_RECC_BURST_BYTES 728

/* beyond ~8 wrong symbols the dotting pattern shifted by one bit period starts to pass as a trigger */
#define AMPS_RECC_MAX_SYNC_TOLERANCE 8

typedef struct amps_recc_cfg {
    uint32_t struct_size;          /* sizeof(amps_recc_cfg_t), for ABI evolution                          */
    uint32_t n_channels;           /* independent RECC instances handled per push (1 .. 2^20-1); a channel's
                                    * stream may run for 2^44 samples between resets (2.8 years at 200 ksps) */
    uint32_t samples_per_symbol;   /* IQ seam: samples per Manchester symbol (10 at 200 ksps); 2..16      */
    uint32_t max_samples_per_push; /* IQ seam: capacity per channel per push (0 = IQ seam unused).
                                    * Wideband seam: the unit is FRAMES (channel-rate samples: wideband samples / wideband_decim), and
                                    * what is bounded is what a push PRODUCES, the frames carried over from earlier pushes included:
                                    * see amps_recc_push_wideband.  Either way it sizes the slicer-bit ring (amps_recc_debug_slicer_bits) */
    uint32_t max_bursts;           /* capacity of the device-side result list per push/drain (>=1)        */
    int32_t  device;               /* HIP device ordinal, -1 = current device                             */
    uint32_t flags;                /* AMPS_RECC_FLAG_*                                                    */
    uint32_t wideband_channels;    /* channelizer seam: M branches of 30 kHz, for a stream at M * 30 ksps: 1024 (30.72 Msps), or 512, 256, 128
                                    * (15.36, 7.68, 3.84 Msps: the narrow banks, see amps_recc_wideband_plan); 0 = seam unused; other values:
                                    * -EINVAL.  At M < 1024 the seam is the two-kernel form (AMPS_RECC_FLAG_UNFUSED_WIDEBAND is accepted and
                                    * changes nothing), wideband_groups > 1 and AMPS_RECC_FLAG_CHANNEL_POWER are -EINVAL, amps_recc_rccl_init
                                    * answers -ENOSYS, and AMPS_RECC_FLAG_STREAM_POWER / _STREAM_OFFSET / _STREAM_OFFSET_UNIT are accepted:
                                    * blocks of 256 channel-rate samples, as on the IQ seam.  Bin M / 2 is centred on +- fs / 2, where the
                                    * radio's own anti-alias filter rolls off: a channel there is received as the radio delivers it.
                                    * Or M branches of 10 kHz, for a stream at M * 10 ksps: 2500, 2000, 1000, 500 (25, 20, 10, 5 Msps: the
                                    * rates of radios on a 100 or 200 MHz clock, see amps_recc_wideband_grid_plan), ONLY together with
                                    * wideband_decim = M / 4 stated explicitly.  Everything said of M < 1024 holds for these banks too.  A
                                    * 30 kHz channel sits on every third bin: channel c of the handle is bin (wideband_first_channel + 3 c)
                                    * mod M, and 3 n_channels <= M (833, 666, 333, 166 channels at most), -EINVAL beyond.  A tuner set to any
                                    * multiple of 10 kHz puts every channel centre on a bin */
    uint32_t wideband_decim;       /* channelizer seam: D input samples per output frame: M / 2 or 3 M / 4, anything else -EINVAL.
                                    * M = 1024: 0 = amps_recc_default_wideband_decim().  M < 1024: 0 = 3 M / 4, the same ratio.
                                    * M = 2500, 2000, 1000, 500: M / 4 (40 ksps per channel, samples_per_symbol = 2, 0 is filled in as 2);
                                    * 0 and every other value are -EINVAL there.
                                    * samples_per_symbol = 0 is filled in as 3 M / (2 D).  At M = 1024:
                                    * 768 (4/3 x oversampled: 40 ksps per channel, samples_per_symbol = 2; the default since round 6)
                                    * or 512 (2x oversampled: 60 ksps, samples_per_symbol = 3; 1.5 x the frames per input byte,
                                    * 0.2 - 0.7 dB more sensitive)                                                     */
    uint32_t wideband_taps_per_branch; /* prototype length = taps_per_branch * M: 8 (0 selects 8); at the banks of 10 kHz bins 3 (0 selects 3) */
    uint32_t wideband_first_channel;   /* first FFT bin that is an active RECC channel, < M (it counts 10 kHz bins at M = 2500 ... 500) */
    uint32_t sync_tolerance;       /* IQ / wideband seams: accept a trigger with up to this many of its 74
                                    * symbols wrong.  0 = exact match, the reference's memmem
                                    * (lib/recc_impl.cc:118) -- keep 0 for parity runs.  <= AMPS_RECC_MAX_SYNC_TOLERANCE */
    uint32_t wideband_groups;      /* channelizer seam: 0 / 1 = this handle decodes the whole band selection; G = 2, 4 or 8 = the band's
                                    * channels are split into G interleaved groups and this handle decodes ONE of them (one handle per
                                    * GPU of a node, every one fed the same wideband stream: BASELINE configs[4]).  Group r = the active
                                    * channels whose FFT bin k has (k mod 64) in [r * 64/G, (r+1) * 64/G): blocks of 64/G adjacent channels,
                                    * every 64 -- the split that lets a rank skip the last FFT pass and the slicer for everybody else's
                                    * bins.  n_channels / wideband_first_channel still describe the WHOLE band selection; records carry
                                    * whole-band channel numbers; fused form only, and the handle serves the wideband seam only:
                                    * amps_recc_push_iq / _push_raw / _push_symbols answer -ENOSYS on it                                */
    uint32_t wideband_group;       /* channelizer seam: which group, 0 .. wideband_groups - 1                                          */
    void    *stream;               /* hipStream_t to launch on, NULL = library-owned stream               */
} amps_recc_cfg_t;

typedef struct amps_recc_timing {
    uint32_t struct_size;
    uint32_t launches_front;   /* number of timed launches of the front kernel since last reset           */
    double   ms_front;         /* summed HIP-event time of the dominant streaming kernel (demod+sync)     */
    double   ms_resolve;       /* per-channel detection ordering / capture scheduling kernel              */
    double   ms_decode;        /* burst extract + Manchester + BCH + parse kernel                         */
    double   ms_carry;         /* inter-push halo copy kernel                                             */
    double   ms_symbols;       /* symbol-seam work() kernel                                               */
    uint64_t samples_front;    /* per-channel IQ samples consumed by the timed front launches             */
    double   ms_channelizer;   /* polyphase channelizer kernel (wideband seam)                            */
    uint32_t launches_channelizer;
    uint32_t _pad;
    double   ms_xlate;         /* translate seam: mixing + channel FIR + decimation kernel                */
} amps_recc_timing_t;

typedef struct amps_recc amps_recc_t; /* opaque; owns device buffers + per-channel stream state */

/* version / introspection */
int         amps_recc_abi_version(void);
/* the numeric slicer spec (AMPS_SLICER_* of amps_recc_numerics.h) of a handle created with no SLICER flag */
int         amps_recc_default_slicer(void);
/* The decimation a wideband handle created with cfg.wideband_decim = 0 uses (cfg.samples_per_symbol = 0 is then filled in to match:
 * 1536 / decim).  768 since round 6: 4/3 x oversampled, 2 samples per symbol -- 1.4 x the throughput of the 2x oversampled bank for
 * 0.2 dB at 1 % burst loss without a carrier offset and 0.7 dB at +-2 kHz (profiles/r06/decim768_sensitivity.txt).  512 (3 samples per
 * symbol) stays one field away: the more sensitive form, and what rounds 1-5 shipped. */
uint32_t    amps_recc_default_wideband_decim(void);
const char *amps_recc_strerror(int code);
size_t      amps_recc_burst_size(void);   /* sizeof(amps_recc_burst_t), for binding self-checks */

/* lifetime */
int  amps_recc_create(amps_recc_t **out, const amps_recc_cfg_t *cfg);
void amps_recc_destroy(amps_recc_t *h);
int  amps_recc_reset(amps_recc_t *h);     /* back to the just-constructed state of every channel */
/* Resume / offset a stream: the first sample pushed after create or reset gets this absolute index (a multiple of 64,
 * < 2^44), so `position` of the records continues a numbering kept elsewhere (checkpoint / restart of a receiver).
 * What precedes the origin is treated like what precedes a stream that starts at 0.  -EBUSY after the first push. */
int  amps_recc_set_origin(amps_recc_t *h, uint64_t first_sample);

/* (i) exact drop-in seam.  One call == one recc_impl::work() call on EVERY channel with
 * noutput_items = n; syms is [n_channels][ld] bytes (values 0/1).  Bursts published by this call
 * are copied to bursts_out ([cap][3374] host bytes) with their channel in burst_channel[], sorted
 * by channel (a channel publishes at most one burst per work() call).  n<1 returns 0 with *nout=0
 * (lib/recc_impl.cc:99-102); n>AMPS_RECC_MAX_WORK_ITEMS returns -EINVAL (the reference asserts). */
int amps_recc_push_symbols(amps_recc_t *h, const uint8_t *syms, size_t ld, int n, int mem,
                           uint8_t *bursts_out, uint32_t *burst_channel, size_t cap, size_t *nout);

/* recc_decode core on a batch of 3374-byte bursts ([nbursts][3374], host or device per `mem`); out and burst_channel are
 * always HOST memory. */
int amps_recc_decode_bursts(amps_recc_t *h, const uint8_t *bursts, size_t nbursts, int mem,
                            const uint32_t *burst_channel /* may be NULL */, amps_recc_burst_t *out);

/* (ii) fused seam: interleaved fc32 IQ, channel-major: sample i of channel c at iq[2*(c*ld + i)].
 * Enqueues the fused demod->sync->capture->decode kernels on the handle's stream and returns
 * without synchronising; results accumulate on the device until amps_recc_drain().
 * Ownership: a HOST buffer has been copied to the device when the call returns (synchronous copy into a
 * fenced staging buffer) and may be reused at once.  A DEVICE buffer is read in place by the enqueued
 * kernels: it must stay valid and unmodified until a drain (or drain_end) that covers this push has
 * returned, or the caller has synchronised the handle's stream.  The same holds for push_wideband /
 * push_raw. */
int amps_recc_push_iq(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem);

/* channelizer seam: one wideband interleaved fc32 stream (fs = M * 30 kHz) -> polyphase
 * channelizer -> the same fused path on every active channel.  nsamp wideband samples.
 * Capacity: cfg.max_samples_per_push counts FRAMES here (one per wideband_decim samples).  A push produces the whole frames of
 * the samples it is given plus those that earlier pushes left over -- in the fused form (the default) rounded down to a multiple
 * of 64, so up to 63 frames and a fraction of one wait for the next push -- and is refused with -E2BIG, nothing consumed, when the
 * frames it would produce exceed max_samples_per_push: up to 63 more than the block itself holds.  A block of at most
 * max_samples_per_push - 63 frames is therefore always accepted, whatever was pushed before (the tests and bench.py create their
 * handles for block + 72 frames); a block of exactly max_samples_per_push frames only while nothing is left over, as when every
 * block so far was a multiple of 64 frames. */
int amps_recc_push_wideband(amps_recc_t *h, const float *iq, size_t nsamp, int mem);

/* like amps_recc_push_wideband, the block as interleaved 16-bit I/Q ("sc16": what converters, the wire formats of USRP-class devices
 * and wideband capture files deliver): sample n = ((float)iq[2n], (float)iq[2n+1]).
 * By definition this is amps_recc_push_wideband on the block converted with a plain int16 -> float conversion, no scaling (every
 * int16 is exact in fp32 and a power-of-two scale changes no decision of any slicer spec): same stream, same carry, same records,
 * same error codes (-EINVAL, -ENOSYS on a handle without the wideband seam, -E2BIG, -ESTALE), same ownership rules for host and
 * device blocks, nsamp == 0 returns 0.  The two calls may be mixed freely on one handle, push by push.  A device block need only be
 * 4-byte aligned (a slice that starts at an odd sample is legal).  The fused filter bank reads the 16-bit block in place, 4 bytes
 * per sample from the host and from HBM; no fc32 copy of it exists (the checking form AMPS_RECC_FLAG_UNFUSED_WIDEBAND expands it first).
 * Not offered in 16 bits: amps_recc_push_wideband_dist / _bcast (the blocks RCCL carries stay fc32) and the IQ seam, whose callers have
 * already filtered in float.  The translate seams take 16-bit and 8-bit samples through their _as entry points (AMPS_RECC_SAMPLES_*),
 * and so does this seam: amps_recc_push_wideband_as below. */
int amps_recc_push_wideband_short(amps_recc_t *h, const int16_t *iq, size_t nsamp, int mem);

/* translate seam: the channel filter the reference's test flow graph wires in front of the
 * chain -- freq_xlating_fir_filter_ccc(decim, firdes.low_pass(gain, rate, cutoff, width), center, rate),
 * grc/recctest.grc:889-937 with taps :115-155 -- so that its ".raw" fc32 captures (400 ksps, channel at
 * +-160 kHz, :591) can be pushed directly.  rate_hz / decim must equal samples_per_symbol * 20 kHz.
 * gain / cutoff_hz / width_hz = 0 select the flow graph's 3.0 / 10 kHz / 4.5 kHz (299 taps at 400 ksps).
 * decim = 0 removes the stage.  Resets nothing else; call before the first push.
 * -EINVAL for a center_hz beyond the rate or not a number (NaN), as amps_recc_set_xlate_shared answers for each of its centres;
 * -EINVAL for a filter the design cannot make: a width_hz that gives fewer than 3 taps (int(74 rate_hz / (22 width_hz)) made odd: a
 * width of about 1.68 rate_hz or more gives one tap and a window of 0 / 0) or a cutoff_hz above rate_hz / 2, which firdes.low_pass
 * refuses too;
 * -E2BIG for a filter of more than 1024 taps (padded to a multiple of 8).  A configuration that is refused leaves the handle's
 * translate stage as it was. */
typedef struct amps_recc_xlate_cfg {
    uint32_t struct_size;
    uint32_t decim;            /* 1, 2 or 4 */
    double   rate_hz;          /* input sample rate */
    double   center_hz;        /* channel centre relative to the input's centre, |center| <= rate */
    double   gain, cutoff_hz, width_hz;
} amps_recc_xlate_cfg_t;
int amps_recc_set_xlate(amps_recc_t *h, const amps_recc_xlate_cfg_t *x);
/* like amps_recc_push_iq but iq is [n_channels][ld] at rate_hz; every channel uses the same centre.
 * nsamp <= decim * max_samples_per_push; any nsamp (leftover samples wait for the next push). */
int amps_recc_push_raw(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem);
/* test tap: run only the translate stage (continuing its stream); out is host [n_channels][out_ld] fc32 */
int amps_recc_debug_xlate(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem,
                          float *out, size_t out_ld, size_t *nout);

/* translate seam, shared form: MANY channels of ONE narrowband stream -- one modest SDR tuned to a system's control channels delivers
 * one fc32 stream of a few hundred ksps that holds many 30 kHz channels (a system's 21 reverse control channels span 630 kHz; the
 * 400 ksps captures of grc/recctest.grc:591 hold up to 13) -- each translated to DC, low-passed and decimated by the filter above,
 * then decoded by the fused IQ seam, all channels in one launch per stage.
 * DEFINITION.  Record `channel` c is centre center_hz[c].  The filtered stream of channel c is what amps_recc_set_xlate with that
 * centre (same rate, decim, gain, cutoff, width) plus amps_recc_push_raw of the same samples produce on a ONE-channel handle, bit
 * for bit (amps_recc_debug_xlate_shared row c == amps_recc_debug_xlate there); the records are therefore those of that handle,
 * except for `channel`.  Duplicate centres are legal and give duplicate records.
 * For the decimations amps_recc_set_xlate does not have, the same identity holds against a ONE-channel handle of this entry point
 * (row c == row 0 of amps_recc_debug_xlate_shared there), and the stream itself is the formula y_c[k] = sum_i h[i] z_c[decim k - i],
 * z_c[n] = x[n] e^{-j 2 pi center_hz[c] n / rate_hz}, as one fp32 fma chain in ascending tap order.
 * decim: 1, 2, 4 or 8 (8 only here: 1.6 Msps at 10 samples per symbol, 1195 taps with the default filter), or 5, 6, 10, 12, 16 or 20
 * (only here: the rates SDRs deliver -- 1.0 Msps / 5, 1.2 / 6, 2.0 / 10, 2.4 / 12, 3.2 / 16 at 10 samples per symbol, 2.4 Msps / 20 at 6;
 * amps_recc_xlate_shared_plan lists what a rate admits); 0 removes the stage.
 * rate_hz / decim must equal samples_per_symbol * 20 kHz; gain / cutoff_hz / width_hz = 0 select the flow graph's 3.0 / 10 kHz /
 * 4.5 kHz as amps_recc_set_xlate does.  The two translate stages exclude each other: configuring one removes the other;
 * amps_recc_push_raw on a shared-configured handle and amps_recc_push_raw_shared on a handle configured with amps_recc_set_xlate
 * answer -ENOSYS, as both do on an unconfigured handle.  Resets nothing else; call before the first push.
 * Errors: -EINVAL (null handle or cfg, wrong struct_size, n_centers != n_channels, null center_hz, a decim other than 0, 1, 2, 4, 5,
 * 6, 8, 10, 12, 16, 20, rate mismatch, a centre beyond the rate, a width_hz that gives fewer than 3 taps or a cutoff_hz above
 * rate_hz / 2, as amps_recc_set_xlate); -E2BIG (the filter, padded to a multiple of 8, has more than 1280
 * taps at decim 1, 2, 4, 8 or more than 2400 at decim 5, 6, 10, 12, 16, 20: the default filter fits up to 3.2 Msps, 2391 taps);
 * -ENOSYS (a handle without the IQ seam, or a channel-group handle).
 * A 4 Msps stream (HackRF) at decim 20 needs width_hz >= 5.61 kHz under the 2400 limit: int(74 * 4e6 / (22 * width_hz)) made odd is
 * 2399 at 5610 Hz, 2403 at 5600 Hz and 2989 at the default 4.5 kHz. */
typedef struct amps_recc_xlate_shared_cfg {
    uint32_t struct_size;
    uint32_t decim;              /* 1, 2, 4, 5, 6, 8, 10, 12, 16 or 20; 0 removes the stage */
    uint32_t n_centers;          /* must equal cfg.n_channels */
    uint32_t _pad;
    double   rate_hz;            /* rate_hz / decim == samples_per_symbol * 20 kHz */
    double   gain, cutoff_hz, width_hz;  /* 0 = the flow graph's 3.0 / 10 kHz / 4.5 kHz, as amps_recc_set_xlate */
    const double *center_hz;     /* [n_centers], |center| <= rate_hz; duplicates are legal */
} amps_recc_xlate_shared_cfg_t;
int amps_recc_set_xlate_shared(amps_recc_t *h, const amps_recc_xlate_shared_cfg_t *x);
/* "Which decimation do I ask for?"  The (decim, samples_per_symbol) pairs amps_recc_set_xlate_shared accepts for a stream at rate_hz
 * with transition width width_hz (0 = the flow graph's 4.5 kHz), ascending by decim; ntaps = the filter's length.  Returns how many
 * there are (may exceed cap, of which the first cap are written; out may be NULL with cap 0); 0 for a rate no decimation serves
 * (2.048 Msps, 2.5 Msps: these take the rational resampler, amps_recc_set_xlate_resampled) or a width that gives fewer than 3 taps, which the configuration refuses;
 * -EINVAL for a rate that is not a positive number.  Host arithmetic only:
 * no handle and no device needed, and it asks the same function the configuration asks, so the two cannot disagree. */
typedef struct amps_recc_xlate_plan { uint32_t decim, samples_per_symbol, ntaps, _pad; } amps_recc_xlate_plan_t;
int amps_recc_xlate_shared_plan(double rate_hz, double width_hz, amps_recc_xlate_plan_t *out, size_t cap);

/* Which filter bank for a wideband stream at rate_hz?  No device needed.  Writes up to `cap` entries of what amps_recc_create accepts as
 * (wideband_channels, wideband_decim, samples_per_symbol) for that rate, the default decimation first, `taps` the prototype's length, and
 * returns how many the rate admits (call with cap = 0 to size): two for a rate within 0.5 Hz of M * 30 kHz, M = 1024, 512, 256 or 128 --
 * 3.84e6: (128, 96, 2, 1024), (128, 64, 3, 1024) -- and 0 for any other rate (10e6, 20e6, 1.92e6: resample in front, or use the
 * translate seam below 3.2 Msps).  -EINVAL: rate_hz not positive and finite, out == NULL with cap > 0. */
typedef struct amps_recc_wideband_plan { uint32_t channels, decim, samples_per_symbol, taps; } amps_recc_wideband_plan_t;
int amps_recc_wideband_plan(double rate_hz, amps_recc_wideband_plan_t *out, size_t cap);
/* The same question for every bank the seam has, the ones whose bins are not 30 kHz wide included.  Same count, cap and error rules.
 * An entry adds the width of a bin, the bins from one channel to the next (channel c = bin (wideband_first_channel + channel_stride c)
 * mod channels) and the most n_channels a handle takes.  For 30.72, 15.36, 7.68 and 3.84 Msps: the entries of amps_recc_wideband_plan
 * with bin_hz = 30000, channel_stride = 1, max_channels = channels.  For a rate within 0.5 Hz of M * 10 kHz, M = 2500, 2000, 1000 or 500,
 * one entry (M, M / 4, 2, 3 M, 10000, 3, M / 3) -- 10e6: (1000, 250, 2, 3000, 10000, 3, 333) -- with wideband_decim to be stated as given.
 * Nothing for 12.5, 6.25, 2.5 or 1.92 Msps, where rate / 40 kHz is no integer. */
typedef struct amps_recc_wideband_grid_plan { uint32_t channels, decim, samples_per_symbol, taps, bin_hz, channel_stride, max_channels, _pad; } amps_recc_wideband_grid_plan_t;
int amps_recc_wideband_grid_plan(double rate_hz, amps_recc_wideband_grid_plan_t *out, size_t cap);
/* For the rates both answer with nothing, ask amps_recc_xlate_resample_plan below. */
/* iq is ONE row of nsamp samples at rate_hz.  Any nsamp <= decim * max_samples_per_push (-E2BIG beyond); leftover samples (fewer than
 * decim) wait for the next push.  Host and device blocks follow the ownership rules of amps_recc_push_raw; amps_recc_reset restarts
 * the stream; ms_xlate of amps_recc_get_timing counts the kernel.  -ESTALE as the data seams. */
int amps_recc_push_raw_shared(amps_recc_t *h, const float *iq, size_t nsamp, int mem);
/* test tap: run only the shared translate stage (continuing its stream); out is host [n_channels][out_ld] fc32 */
int amps_recc_debug_xlate_shared(amps_recc_t *h, const float *iq, size_t nsamp, int mem,
                                 float *out, size_t out_ld, size_t *nout);

/* translate seam, shared form behind a rational resampler: the rates no integer decimation brings to samples_per_symbol * 20 kHz --
 * 2.048 Msps (the RTL-SDR tools' default) * 5/64 = 160 ksps, 2.5 Msps (USRP N2xx, Airspy) * 2/25 = 200 ksps, 3.0 Msps * 2/25 = 240,
 * 1.024 Msps * 5/32, 768 ksps (Airspy HF+) * 5/24 or 5/16, 1.25 Msps * 4/25; amps_recc_xlate_resample_plan lists what a rate admits.
 * DEFINITION.  The stream at rate_hz is resampled by interp / decim = L / M to samples_per_symbol * 20 kHz by the textbook polyphase
 * resampler behind the per-channel mix of amps_recc_set_xlate_shared.  The prototype g = firdes.low_pass(gain * L, L * rate_hz,
 * cutoff_hz, width_hz), the flow graph's filter designed at the up-sampled rate with its gain times L for the zero stuffing, has
 * N_g = int(74 L rate_hz / (22 width_hz)) made odd taps.  Phase p has the taps h_p[i] = g[L i + p], zero beyond N_g:
 * Np = ceil(N_g / L) taps per phase, zero padded to a multiple of 8 (ntp).  For output k write k M = L q_k + p_k, 0 <= p_k < L; then
 *     y_c[k] = sum_{i = 0}^{ntp - 1} h_{p_k}[i] z_c[q_k - i],   z_c[n] = x[n] e^{-j 2 pi center_hz[c] n / rate_hz},
 * the mix of sample n taken from its absolute index as in the integer forms, the sum one fp32 fma chain in ascending i, samples
 * before the stream's start zero.  After N input samples in all the stream has delivered ceil(L N / M) outputs -- the k with
 * q_k <= N - 1; a push delivers the difference to what was delivered before, and later outputs wait for their last input.  The
 * result does not depend on push boundaries, the sample format or the other channels.
 * interp: 2 ... 5; decim: interp < decim <= 64 with no factor in common with interp; 0 removes the stage.  rate_hz * interp / decim
 * must equal samples_per_symbol * 20 kHz; gain / cutoff_hz / width_hz = 0 select the flow graph's 3.0 / 10 kHz / 4.5 kHz.
 * Once configured, amps_recc_push_raw_shared, _push_raw_shared_as, _debug_xlate_shared and _debug_xlate_shared_as run this stage: any
 * nsamp that delivers at most max_samples_per_push outputs (-E2BIG beyond).  The three translate forms exclude each other:
 * configuring one removes the others.  Resets nothing else; call before the first push.
 * Errors, as amps_recc_set_xlate_shared: -EINVAL (null handle or cfg, wrong struct_size, n_centers != n_channels, null center_hz,
 * interp outside 2 ... 5, decim <= interp or > 64, a common factor, rate mismatch, a centre beyond the rate, a width_hz that gives
 * fewer than 3 taps or a cutoff_hz above interp * rate_hz / 2); -E2BIG (more than 2400 padded taps per phase, or the interp tap
 * sets and the mixed window of 64 decim + ntp samples beyond 80 KB of LDS: the default filter fits every ratio above, 2.048 Msps *
 * 5/64 has 1531 taps per phase); -ENOSYS (a handle without the IQ seam, or a channel-group handle).  A configuration that is
 * refused leaves the handle's translate stage as it was. */
typedef struct amps_recc_xlate_resample_cfg {
    uint32_t struct_size;
    uint32_t interp;             /* L: 2 ... 5 */
    uint32_t decim;              /* M: interp < M <= 64, gcd(L, M) = 1; 0 removes the stage */
    uint32_t n_centers;          /* must equal cfg.n_channels */
    uint32_t _pad;
    double   rate_hz;            /* rate_hz * interp / decim == samples_per_symbol * 20 kHz */
    double   gain, cutoff_hz, width_hz;  /* 0 = the flow graph's 3.0 / 10 kHz / 4.5 kHz, as amps_recc_set_xlate */
    const double *center_hz;     /* [n_centers], |center| <= rate_hz; duplicates are legal */
} amps_recc_xlate_resample_cfg_t;
int amps_recc_set_xlate_resampled(amps_recc_t *h, const amps_recc_xlate_resample_cfg_t *x);
/* "Which ratio do I ask for?"  The (interp, decim, samples_per_symbol) triples amps_recc_set_xlate_resampled accepts for a stream at
 * rate_hz with transition width width_hz (0 = 4.5 kHz), ascending by (interp, decim); ntaps_per_phase = ceil(N_g / interp).  Return
 * value, cap and errors as amps_recc_xlate_shared_plan; 0 for a rate no admitted ratio serves (2.4 Msps: integer decimation is its
 * answer).  Host arithmetic only, and it asks the same function the configuration asks. */
typedef struct amps_recc_resample_plan { uint32_t interp, decim, samples_per_symbol, ntaps_per_phase; } amps_recc_resample_plan_t;
int amps_recc_xlate_resample_plan(double rate_hz, double width_hz, amps_recc_resample_plan_t *out, size_t cap);

/* translate seams on an SDR's integer samples, read IN PLACE.  No SDR delivers fc32: USRP-class devices, Lime and Pluto deliver
 * interleaved int16 ("sc16"), HackRF int8 ("sc8"), RTL-SDR offset-binary uint8 ("cu8"), and their capture files hold the same. */
#define AMPS_RECC_SAMPLES_FC32 0   /* float I, float Q: what the plain entry points take            */
#define AMPS_RECC_SAMPLES_SC16 1   /* int16 I, int16 Q:  sample = ((float)i, (float)q)               */
#define AMPS_RECC_SAMPLES_SC8  2   /* int8  I, int8  Q:  sample = ((float)i, (float)q)               */
#define AMPS_RECC_SAMPLES_CU8  3   /* uint8 I, uint8 Q, offset binary: ((float)i - 127.5f, (float)q - 127.5f) */
/* DEFINITION.  Each _as call is the fc32 call of the same name (amps_recc_push_raw_shared, _push_raw, _debug_xlate_shared,
 * _debug_xlate) on the block converted by the plain conversion above, no scaling.  Every conversion is exact in binary32, so the
 * result is the same stream, the same carry, the same output bits from the stage, the same records and the same error codes.
 * format == AMPS_RECC_SAMPLES_FC32 IS the fc32 call; an unknown format is -EINVAL.  Formats may be mixed freely on one handle, push
 * by push, with each other and with the fc32 entry points (the stage's carry is fc32).  ld and nsamp count SAMPLES, whatever their
 * size.  A device block need only be aligned to one sample: 4 bytes for sc16, 2 bytes for sc8 and cu8 (a slice that starts at an odd
 * sample is legal).  Every other error, nsamp == 0, and the ownership rules for host and device blocks are those of the fc32 calls.
 * The block is read in its own format by the stage's kernels -- 4 or 2 bytes per sample over the host link and from HBM; no fc32
 * copy of it exists on the host or on the device.
 * No scaling and no DC removal are offered: the stage is linear, so the filter's `gain` is the place for a scale, and a tuner's DC
 * lands on centre 0, where no control channel sits.
 * Not offered in integer formats: amps_recc_push_iq (its callers have already filtered in float) and the distributed pushes
 * amps_recc_push_wideband_dist / _bcast (the blocks RCCL carries stay fc32). */
int amps_recc_push_raw_shared_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem);
int amps_recc_push_raw_as(amps_recc_t *h, const void *iq, size_t ld, size_t nsamp, int format, int mem);
int amps_recc_debug_xlate_shared_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nout);
int amps_recc_debug_xlate_as(amps_recc_t *h, const void *iq, size_t ld, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nout);

/* wideband seam on an SDR's integer samples, read IN PLACE on every bank: a HackRF streams 3.84 to 15.36 Msps as sc8 and nothing else.
 * DEFINITION.  Each _as call is the fc32 call of the same name (amps_recc_push_wideband, amps_recc_debug_channelize) on the block
 * converted by the plain AMPS_RECC_SAMPLES_* conversion above, no scaling (cu8: minus 127.5).  Every conversion is exact in binary32,
 * so the result is the same stream, the same fc32 carry, the same output bits from the filter bank, the same records, the same power
 * and autocorrelation rings and the same error codes: -EINVAL, -ENOSYS on a handle without the wideband seam, -E2BIG with nothing
 * consumed, -ESTALE; nsamp == 0 returns 0 from the push.  format == AMPS_RECC_SAMPLES_FC32 IS amps_recc_push_wideband,
 * AMPS_RECC_SAMPLES_SC16 IS amps_recc_push_wideband_short; an unknown format is -EINVAL.  Formats may alternate push by push on one
 * handle, with each other and with the two existing entry points.  nsamp counts SAMPLES, whatever their size.  A device block need
 * only be aligned to one sample: 2 bytes for sc8 and cu8 (a slice that starts at an odd sample is legal), and the kernels touch no
 * aligned dword that holds no byte of it.  A host block is staged as it is, at 2 bytes per sample; ownership is as for the fc32 call.
 * The banks of 512, 256 and 128 branches read the 8-bit block in place, 2 bytes per sample over the host link and from HBM; no fc32
 * copy of it exists, and so do the banks of 2500, 2000, 1000 and 500 branches (25 to 5 Msps: an N2xx's sc16 or sc8 over the wire, an
 * Airspy's or SDRplay's sc16, a HackRF's sc8 at 20 and 10 Msps), for every format.  The 1024 bank (30.72 Msps: no radio delivers 8 bits there, converted capture files do) expands an 8-bit block
 * to fc32 on the device first and then runs as on any fc32 block, in every form it has.
 * Received power (amps_recc_channel_power / _burst_power) reads in the input's own units squared.  No scaling is offered: the bank
 * is linear and no slicer's decision depends on scale. */
int amps_recc_push_wideband_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem);
int amps_recc_debug_channelize_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem,
                                  float *out, size_t out_ld, size_t *nframes);

/* The tuner's frequency error, corrected inside the filter bank: a bank has fixed bins, and a radio whose crystal is a few ppm off (1 ppm
 * is 835 Hz at 835 MHz) delivers every channel that far from its bin's centre.  With a shift set, the bank runs on
 *     z[n] = x[n] e^(-j 2 pi frac(n step))
 * in place of x[n].  n is the wideband sample's absolute index, counted from the handle's creation or last amps_recc_reset
 * (amps_recc_set_origin numbers channel-rate samples and does not move it).  step is shift_hz / fs as a 0.64 fixed-point fraction of a
 * turn, fs = wideband_channels x 30 kHz, or x 10 kHz at the banks of 10 kHz bins.  The product is the translate seams' mixer: the phasor
 * from the top 24 bits of the wrapped 64-bit product n step through sincospif, one fp32 complex multiply, evaluated per sample from
 * the absolute index and never as a running rotation.  A sample gets the same bits whichever workgroup stages it, whichever push it
 * arrived in and whatever format it had.
 * Sign: shift_hz is the frequency in the delivered stream of what shall land on bin 0's centre.  A radio that delivers everything e
 * hertz too high gets shift_hz = +e.
 * The shift takes effect with the next push or debug tap.  Nothing is reset: taps, carry (which keeps UNMIXED input: every launch
 * mixes all it stages with the step in force), positions and everything behind the bank are kept; no device write, no host wait, so
 * the call may be made between drain_begin and drain_end.  shift_hz == 0, the state after create, runs the unmixed kernels: the
 * behaviour without this call, bit for bit.  amps_recc_reset keeps the shift and restarts n at 0.
 * Contract, as for amps_recc_retune_xlate: from the first push after the call the bank's output is bit for bit that of a twin handle
 * that had the new shift from the start and was fed the same pushes.  Records of bursts whose dotting begins at least 2048
 * channel-rate samples after that push's first frame are byte-identical to the twin's; the one discriminator product and the ring
 * blocks that span the change are not.
 * -EINVAL: h == NULL, a NaN, |shift_hz| > fs / 2.  -ENOSYS: a handle without the wideband seam, or with wideband_channels = 1024 (the
 * fused bank has no mixing form; radios that reach 30.72 Msps have a TCXO).  A refused call leaves the handle as it was.
 * amps_recc_wideband_shift reads the shift in force back as quantised to the step, within fs 2^-64 of what was set (-EINVAL for a
 * NULL argument, -ENOSYS as above). */
int amps_recc_set_wideband_shift(amps_recc_t *h, double shift_hz);
int amps_recc_wideband_shift(const amps_recc_t *h, double *shift_hz);

/* wideband seam behind a rational resampler: the rates SDRs deliver that are no bank's rate -- a HackRF's 8 Msps * 5/4 = 10 Msps, its
 * 12.5 Msps * 2/1 = 25 and 16 Msps * 5/4 = 20, an Airspy Mini's or SDRplay's 6 Msps * 5/3 = 10, 4 Msps * 5/4 = 5, 3.2 Msps * 6/5 = 3.84;
 * amps_recc_wideband_resample_plan lists what a rate admits.  Resampling UP to the next bank rate keeps the whole delivered band, and
 * frequencies in hertz do not move: a tuner on a multiple of the bank's bin width still has every channel centre on a bin, and
 * amps_recc_set_wideband_shift corrects what is left.
 * DEFINITION.  The stream at rate_hz is resampled by interp / decim = L / M to the bank's rate, wideband_channels times its bin width,
 * by the textbook polyphase resampler.  With f_low = min(rate_hz, the bank's rate), width_hz = 0 selects f_low / 16 and cutoff_hz = 0
 * selects f_low / 2 - width_hz / 2: the stop band then begins at f_low / 2 and the pass band is flat to f_low / 2 - width_hz.  The
 * prototype g = firdes.low_pass(L, L * rate_hz, cutoff_hz, width_hz) (Blackman), the design of amps_recc_set_xlate_resampled at the
 * up-sampled rate with gain L for the zero stuffing, has N_g = int(74 L rate_hz / (22 width_hz)) made odd taps.  Phase p has the taps
 * h_p[i] = g[L i + p], zero beyond N_g: Np = ceil(N_g / L) taps per phase, zero padded to a multiple of 8 (ntp) -- 54 (56) with the
 * defaults when resampling up, 107 (112) at 1/2.  For output k write k M = L q_k + p_k, 0 <= p_k < L; then
 *     y[k] = sum_{i = 0}^{ntp - 1} h_{p_k}[i] x[q_k - i],
 * each component one fp32 fma chain in ascending i, x the block converted by the plain AMPS_RECC_SAMPLES_* conversion, samples before
 * the stream's start zero, k and q absolute indices since create or amps_recc_reset in 64-bit arithmetic.  After N input samples in
 * all the stream has delivered ceil(L N / M) outputs; a push delivers the difference to what was delivered before.  The result does
 * not depend on push boundaries or on the sample format.
 * The bank behind it sees y exactly as it would see a device fc32 block: the carry, the frame masks, max_samples_per_push in frames,
 * positions, the power and offset rings and the records are what they are without a resampler, and the n of
 * amps_recc_set_wideband_shift counts the resampler's outputs.
 * interp, decim: 1 ... 8 with no factor in common, interp != decim, 1/2 <= interp / decim <= 4; decim = 0 removes the stage.
 * rate_hz * interp / decim must lie within 1e-6 (relative) of the bank's rate.
 * While a resampler is configured, amps_recc_push_wideband, _short, _as, amps_recc_debug_channelize and _as take blocks at rate_hz, in
 * any format, through the resampler; a push whose frames would exceed max_samples_per_push answers -E2BIG with nothing consumed; the
 * distributed pushes amps_recc_push_wideband_dist / _bcast answer -ENOSYS.  amps_recc_reset keeps the configuration and restarts k
 * and q at 0 with zero history.
 * Errors: -EINVAL (null handle or cfg, wrong struct_size); -ENOSYS (a handle without the wideband seam); -EBUSY (the seam has taken
 * a block since create or reset: set or remove the stage before the first push, or after amps_recc_reset); -EINVAL (interp or decim
 * outside 1 ... 8, a common factor, interp == decim, a ratio outside 1/2 ... 4, a rate mismatch, numbers that are not finite or are
 * negative, a width_hz that gives fewer than 3 taps, a cutoff_hz above interp * rate_hz / 2); -E2BIG (more than 512 padded taps per
 * phase, or the tap sets and a tile's window beyond 64 KB of LDS).  A call that is refused leaves the handle as it was. */
typedef struct amps_recc_wideband_resample_cfg {
    uint32_t struct_size, interp, decim, _pad;   /* L, M; decim = 0 removes the stage */
    double   rate_hz;                            /* the delivered rate; rate_hz * L / M == the bank's rate */
    double   cutoff_hz, width_hz;                /* 0 = the defaults above */
} amps_recc_wideband_resample_cfg_t;
int amps_recc_set_wideband_resample(amps_recc_t *h, const amps_recc_wideband_resample_cfg_t *r);
/* "Which ratio into which bank?"  The (interp, decim, channels, bank_decim) combinations a stream at rate_hz admits with the default
 * filter, ascending by (interp, decim) and, within one bank, by its decimations in the order of amps_recc_wideband_grid_plan:
 * 8e6: (5, 2, 2000, 500), (5, 4, 1000, 250), (5, 8, 500, 125); 12.5e6: (2, 1, 2500, 625), (4, 5, 1000, 250), (8, 5, 2000, 500);
 * 3.2e6: (6, 5, 128, 96), (6, 5, 128, 64); nothing for 56 Msps.  A bank's own rate lists only true resamplings.  An entry adds what
 * amps_recc_create wants beside channels and bank_decim (samples_per_symbol), ntaps_per_phase = ceil(N_g / interp), the bank's bin
 * width and channel stride, and usable_hz = 2 (f_low / 2 - width_hz), the band the filter keeps flat.  Give the handle the channels
 * inside that band only (wideband_first_channel, n_channels): when resampling up, the bank's bins beyond the delivered band hold the
 * stop band's images of the band, signal and noise alike some 74 dB down, and an FM receiver decodes an image as it does the mobile.
 * Return value, cap and errors
 * as amps_recc_wideband_grid_plan.  Host arithmetic only, and it asks the same function the configuration asks. */
typedef struct amps_recc_wideband_resample_plan {
    uint32_t interp, decim, channels, bank_decim, samples_per_symbol, ntaps_per_phase, bin_hz, channel_stride, usable_hz, _pad;
} amps_recc_wideband_resample_plan_t;
int amps_recc_wideband_resample_plan(double rate_hz, amps_recc_wideband_resample_plan_t *out, size_t cap);
/* test tap: run only the resampler on a block in `format` (AMPS_RECC_SAMPLES_*), continuing its stream; out is host fc32 [cap] and
 * *nout the outputs this block delivered (-E2BIG beyond cap, with nothing consumed).  -ENOSYS without a configured resampler. */
int amps_recc_debug_wideband_resample(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem, float *out, size_t cap, size_t *nout);

/* Retune: replace the centres of the translate form configured last (amps_recc_set_xlate, _set_xlate_shared or _set_xlate_resampled)
 * in mid-stream.  Taps, carry, absolute positions, the decimation or L / M and everything behind the stage are kept; nothing is
 * reset.  n must equal the configured number of centres -- n_channels for the shared and the resampled form, 1 for the per-row form --
 * else -EINVAL; each centre is checked as the configuration checked it (|center_hz| <= rate_hz, a NaN refused: -EINVAL); -ENOSYS where
 * no translate form is configured.  A refused call leaves the handle as it was.
 * The new centres take effect with the NEXT push (or debug tap).  The update is ordered on the handle's stream behind the kernels
 * already queued, the host does not wait for the device, and center_hz is not read after the call returns.  It may be issued between
 * amps_recc_drain_begin and amps_recc_drain_end.
 * CONTRACT.  A sample's phasor comes from its absolute index times its channel's step and the carry holds unmixed input, so from the
 * first push after the call the stage's output -- what amps_recc_debug_xlate_shared[_as] / amps_recc_debug_xlate[_as] return -- is bit
 * for bit that of a twin handle configured with the new centres from the start and fed the same pushes.
 * Downstream ONE discriminator product spans the change: the first new output against the carried last old one.  The block of A / U
 * and of block power that contains that sample, and any capture that spans it, are therefore not those of the twin.  Records of bursts
 * whose dotting begins at least 2048 channel-rate samples after the retune point are byte-identical to the twin's. */
int amps_recc_retune_xlate(amps_recc_t *h, const double *center_hz, size_t n);

/* Reference-timing seam (checking mode): the flow graph's OWN sub-chain in front of amps_recc, computed on the device as GNU
 * Radio 3.7 defines it -- analog.quadrature_demod_cf(1) -> digital.clock_recovery_mm_ff(omega 10, gain_omega .25*.175^2*3,
 * mu 0, gain_mu .05, omega_relative_limit .005) -> digital.binary_slicer_fb (grc/recctest.grc:458, 846-874, 807) -- for
 * every channel of a channel-major fc32 block at 200 ksps (samples_per_symbol must be 10).  The Mueller & Mueller loop is
 * a sequential recursion: one lane per channel.  symbols_out is host memory [n_channels][sym_ld] (values 0/1: exactly the
 * byte stream gr::amps::recc::work is fed), nsym_out[c] the number produced for channel c by this call (<= nsamp/9 + 16);
 * stream state continues across calls.  Feed the symbols to amps_recc_push_symbols for the reference chain end to end. */
int amps_recc_refchain_symbols(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem,
                               uint8_t *symbols_out, size_t sym_ld, uint32_t *nsym_out);
/* test tap: the two tables the seam uses (fast_atan2f: 258 floats, MMSE interpolator: 129 x 8 floats) */
int amps_recc_refchain_tables(amps_recc_t *h, float *atan258, float *mmse1032);

/* Stream ordering for DEVICE buffers.  A handle created with cfg.stream = NULL launches on its own non-blocking stream,
 * which is not ordered against any other stream: a device buffer must have been completely written before it is pushed.
 * Either synchronise the producing stream first, or record an event behind the producer and hand it over here: work
 * enqueued by LATER calls on this handle waits for it (hipStreamWaitEvent; nothing blocks on the host).  `hip_event` is
 * a hipEvent_t. */
int amps_recc_wait_event(amps_recc_t *h, void *hip_event);
/* the converse: records `hip_event` (a hipEvent_t of the caller) behind everything enqueued on the handle so far, so that
 * another stream can wait for the handle's kernels before it overwrites a buffer they read */
int amps_recc_record_event(amps_recc_t *h, void *hip_event);

/* Synchronise the handle's stream and copy out the decoded bursts accumulated since the last
 * drain, sorted by (channel, position).  -ENOSPC if the device list overflowed max_bursts
 * (the first max_bursts records are still returned). */
int amps_recc_drain(amps_recc_t *h, amps_recc_burst_t *out, size_t cap, size_t *nout);
/* Split drain for streaming callers that must not idle the GPU while the host collects results:
 *     push(n); drain_begin();  push(n+1);  drain_end(&records of everything pushed before drain_begin) ...
 * drain_begin closes the current record list without waiting (later pushes append to a second list);
 * drain_end waits only for the work enqueued before drain_begin.  At most one split drain is open
 * (-EBUSY otherwise); amps_recc_drain == drain_begin + drain_end. */
int amps_recc_drain_begin(amps_recc_t *h);
int amps_recc_drain_end(amps_recc_t *h, amps_recc_burst_t *out, size_t cap, size_t *nout);
/* amps_recc_drain that also hands out the captured symbols of every record, bursts_out[i] = the 3374 bytes (0/1) the reference's
 * recc block would have published for record i ([cap][3374] host bytes; handle created with AMPS_RECC_FLAG_KEEP_BURSTS, -ENOSYS
 * otherwise).  decode_bursts(bursts_out[i]) gives out[i] again (position and channel aside). */
int amps_recc_drain_bursts(amps_recc_t *h, amps_recc_burst_t *out, uint8_t *bursts_out, size_t cap, size_t *nout);

/* test/diagnostic taps (not on the hot path): FM-demod floats and sliced symbol bits of one
 * channel for the last push_iq() call.  demod/soft/hard are host arrays of length n (may be NULL). */
int amps_recc_debug_demod(amps_recc_t *h, const float *iq, size_t nsamp, int mem,
                          float *demod, float *soft, uint8_t *hard);

/* test tap of the slicer bit ring: the bits of absolute samples [first, first + n) of every ring row, one byte (0 / 1) each,
 * into host memory out[n_channels][out_ld], once the pushes enqueued so far have finished; *rows = the rows written (n_channels,
 * or a channel-group handle's own channel count: row i = the i-th channel of its group in band order), *produced = one past the
 * last sample the slicer has produced (set_origin counts).  Every seam that slices into the ring has one: IQ, translate and
 * wideband (fused and AMPS_RECC_FLAG_UNFUSED_WIDEBAND).  The ring holds exactly the window
 *     [max(origin, produced - R), produced),   R = the smallest power of two >= max_samples_per_push + sps * 3586 + 1024
 * samples (3586 = AMPS_RECC_CAPTURE_SYMS + 2 * AMPS_RECC_TRIGGER_SYMS + 64).
 * -ERANGE if any of the samples is not produced yet or no longer held by the ring; -ENOSYS on a handle without the ring (symbol
 * seam only); -EINVAL for out == NULL or out_ld < n with n > 0 (rows / produced may be NULL).  n = 0 only reports rows and produced.
 * Changes nothing: the next push behaves as if the call had not been made. */
int amps_recc_debug_slicer_bits(amps_recc_t *h, uint64_t first, size_t n, uint8_t *out, size_t out_ld,
                                uint32_t *rows, uint64_t *produced);

/* ---- received power of the wideband seam (handles created with AMPS_RECC_FLAG_CHANNEL_POWER; -ENOSYS on a handle with neither power flag) ----
 * A POWER SNAPSHOT is taken at every channel-rate sample index s with s % AMPS_RECC_POWER_STRIDE == 0, s in the numbering of
 * amps_recc_debug_slicer_bits and of amps_recc_burst_t.position (absolute, amps_recc_set_origin counted: frame m of the stream is
 * s = origin + m).  Snapshot j = s / 256 of row r is P[r][j] = |Y_k[m]|^2, Y_k[m] the filter-bank output of the row's FFT bin for that
 * frame (prototype and decimation are the handle's; samples before the stream start are zeros): linear power, fp32, unscaled.  The
 * prototype has unit DC gain, so an unmodulated carrier of amplitude a at a channel centre reads a^2; blocks pushed with
 * amps_recc_push_wideband_short read in int16 units squared.  Snapshots depend on the stream only, never on how it was cut into pushes
 * or on the sample type of a block; the fused form holds back up to 63 frames, and snapshot j exists once its frame has been consumed:
 * 256 j < produced (the `produced` of amps_recc_debug_slicer_bits).  The handle keeps the last R / 256 snapshots of every row, R the
 * span of the slicer-bit ring (see amps_recc_debug_slicer_bits): every record found by a push still has its whole capture inside the
 * window when that push is drained.  amps_recc_reset empties the window.  Cost: one short kernel behind the filter bank per push that
 * re-computes one frame in 256. */
#define AMPS_RECC_POWER_STRIDE 256
/* out[row][i] = P[row][first_snap + i], i < n, into host memory out[rows][out_ld], once the pushes enqueued so far have finished;
 * *rows as amps_recc_debug_slicer_bits reports it, *produced_snaps = one past the newest snapshot (either may be NULL).  The held
 * window is [max(ceil(origin / 256), produced_snaps - R / 256), produced_snaps): -ERANGE for anything outside it.  n = 0 only reports.
 * -EINVAL for a null handle, or out == NULL / out_ld < n with n > 0; -ESTALE as the data seams.  Changes nothing. */
int amps_recc_channel_power(amps_recc_t *h, uint64_t first_snap, size_t n, float *out, size_t out_ld,
                            uint32_t *rows, uint64_t *produced_snaps);
/* Burst power: for each of the n records (host array; only `channel` and `position` are read) the arithmetic mean of P[row(channel)][j]
 * over all j with position <= 256 j <= position + AMPS_RECC_CAPTURE_SYMS * samples_per_symbol -- the capture -- into mean_power[i], and
 * the number of those snapshots, floor(hi / 256) - ceil(lo / 256) + 1 (26 or 27 at D = 768, 39 or 40 at D = 512), into n_snaps[i].  If any
 * of them is no longer held or not yet produced: n_snaps[i] = 0 and mean_power[i] = 0.0f, which is not an error.  `channel` is the
 * whole-band channel number the records carry; one this handle does not decode: -EINVAL (as for a null handle or null arrays with n > 0). */
int amps_recc_burst_power(amps_recc_t *h, const amps_recc_burst_t *recs, size_t n, float *mean_power, uint32_t *n_snaps);
/* snapshots the handle keeps per row, R / 256; 0 on a handle without the flag (or a null handle) */
uint32_t amps_recc_power_ring_snaps(const amps_recc_t *h);

/* ---- received power of the IQ and translate seams (handles created with AMPS_RECC_FLAG_STREAM_POWER) ----
 * The three entry points above answer on such a handle too, with the same arguments and errors, for a BLOCK MEAN instead of a snapshot:
 * on these seams the channel-rate stream is in device memory for the length of a push, so all of it is read, not one sample in 256.
 * Numbering.  y_c[s] is the channel-rate sample of row c at absolute index s, the numbering of amps_recc_burst_t.position and of
 *   amps_recc_debug_slicer_bits (amps_recc_set_origin counted): the sample the streaming kernel slices -- the caller's IQ on
 *   amps_recc_push_iq, the translate stage's output on amps_recc_push_raw[_as] and amps_recc_push_raw_shared[_as] (integer, wide and
 *   rational forms).  Row = channel: rows = n_channels.
 * Block j of row c is  P[c][j] = (1 / 256) * sum over s = 256 j ... 256 j + 255 of |y_c[s]|^2 : linear, fp32, unscaled,
 *   AMPS_RECC_POWER_STRIDE the block length.  An unmodulated carrier of amplitude a reads a^2 on amps_recc_push_iq and (gain * a)^2 at a
 *   centre of a translate seam once the filter has filled.
 * Summation order, ONE and fixed: the terms are t(s) = fma(im, im, re * re) in fp32.  Lane l = 0 ... 63 adds
 *   ((t(256 j + l) + t(256 j + l + 64)) + t(256 j + l + 128)) + t(256 j + l + 192); the 64 lane sums are added by the butterfly
 *   a_l = a_l + a_(l xor o) for o = 32, 16, 8, 4, 2, 1; the result times 2^-8, which is exact.  Every term is non-negative, so
 *   |P - exact| <= 257 * 2^-24 * exact.
 * Existence.  Block j exists once 256 (j + 1) <= produced, `produced` as amps_recc_debug_slicer_bits reports it (the seam holds back
 *   fewer than 64 samples); *produced_snaps = floor(produced / 256).
 * Held window.  [max(ceil(origin / 256), produced_snaps - R / 256), produced_snaps), R the span of the slicer-bit ring; anything outside
 *   it is -ERANGE.  A block that would begin before the origin is never reported.  Every record found by a push still has its whole
 *   capture inside the window when that push is drained.
 * Independence.  Values depend on the stream only: not on how it was cut into pushes, on ld, on host or device residence, or on the
 *   integer format a translate push arrived in (bit-identical in each case).  amps_recc_reset empties the window; the debug taps
 *   amps_recc_debug_xlate* leave it alone, as they leave the slicer alone.
 * Burst power.  The arithmetic mean of P[channel][j] over the blocks that lie wholly inside the capture,
 *   j0 = ceil(position / 256) ... j1 = floor((position + AMPS_RECC_CAPTURE_SYMS * samples_per_symbol) / 256) - 1, n_snaps = j1 - j0 + 1
 *   (130 or 131 at 10 samples per symbol, 38 or 39 at 3).  If any of those blocks is not held: {0.0f, 0}, which is not an error.
 *   channel >= n_channels: -EINVAL.
 * Cost: one short kernel behind the streaming kernel per push, one more read of the push's samples. */

/* ---- carrier offset of the IQ and translate seams (handles created with AMPS_RECC_FLAG_STREAM_OFFSET or AMPS_RECC_FLAG_STREAM_OFFSET_UNIT; -ENOSYS without) ----
 * How far a mobile's carrier stands from the centre of its channel, from the lag-one autocorrelation (pulse-pair) sum of the stream:
 * Manchester FM is balanced over every bit, so over a burst at offset f the products y[s] conj(y[s - 1]) sum to
 * e^(j 2 pi f / fs) (N+ e^(jd) + N- e^(-jd)) with N+ = N-, whose argument is 2 pi f / fs.  The sum is amplitude-weighted: noise-only
 * blocks add little.  Behind a channel filter that cuts into the offset signal the estimate reads low, because the filter takes
 * amplitude from the side of the spectrum the offset moved outwards and the sum leans to the other: 4 - 5 % low behind a translate
 * seam's filter with cutoff_hz = 16e3, and behind the default 10 kHz cut-off so far that it comes out with the WRONG SIGN -- measure
 * behind 16 kHz, or on amps_recc_push_iq (DESIGN.md 4.7g has the measured table) -- or create the handle with
 * AMPS_RECC_FLAG_STREAM_OFFSET_UNIT, whose statistic U (defined at the end of this comment) is right behind the default filter too.
 * Numbering, rows and blocks are those of AMPS_RECC_FLAG_STREAM_POWER above: y_c[s] the channel-rate sample the streaming kernel slices,
 *   s absolute (amps_recc_set_origin counted), row = channel, a block AMPS_RECC_POWER_STRIDE = 256 samples.
 * Block j of row c is  A[c][j] = 2^-8 * sum over s = 256 j ... 256 j + 255 of y_c[s] * conj(y_c[s - 1]) : complex, an fp32 pair
 *   (re, im), unscaled.  y_c[origin - 1] = 0: the sample in front of the stream is zero, so the first product of a block that begins at
 *   the origin is zero.  An unmodulated carrier a e^(j 2 pi f s / fs) reads a^2 e^(j 2 pi f / fs).
 * Summation order, ONE and fixed.  With a = y[s] and b = y[s - 1] the terms are, in fp32,
 *   re(s) = fma(a.re, b.re, a.im * b.im)   and   im(s) = fma(a.im, b.re, -(a.re * b.im)).
 *   Re and im are summed separately and alike: lane l = 0 ... 63 adds ((t(256 j + l) + t(256 j + l + 64)) + t(256 j + l + 128)) +
 *   t(256 j + l + 192); the 64 lane sums are added by the butterfly a_l = a_l + a_(l xor o) for o = 32, 16, 8, 4, 2, 1; the result times
 *   2^-8, which is exact.  Error: a term carries at most 2 u |a| |b| (the product's rounding and the fma's; |a.re b.re| + |a.im b.im| <=
 *   |a| |b|), u = 2^-24, and the 255 additions at most 255 u times the sum of the |terms| whatever the order, so each component lies
 *   within 257 * 2^-24 * 2^-8 * sum |y[s]| |y[s - 1]| of the exact value.  The terms cancel, so the bound is relative to that sum, not to |A|.
 * Existence, held window, independence: exactly as for the block means above -- block j exists once 256 (j + 1) <= produced,
 *   *produced_blocks = floor(produced / 256); the window is [max(ceil(origin / 256), produced_blocks - R / 256), produced_blocks),
 *   R the span of the slicer-bit ring (amps_recc_debug_slicer_bits), and anything outside it is -ERANGE; every record found by a
 *   push still has its whole capture inside the window when that push is drained; values depend on the stream only (not on the cut
 *   into pushes, ld, residence or integer format: bit-identical in each case); amps_recc_reset empties the window, the debug taps leave it
 *   alone.  With both flags on nothing of either changes: the power values are those of a handle with AMPS_RECC_FLAG_STREAM_POWER alone.
 * Cost: one short kernel behind the streaming kernel per push, one more read of the push's samples.
 *
 * THE UNIT-AMPLITUDE STATISTIC (handles created with AMPS_RECC_FLAG_STREAM_OFFSET_UNIT instead).  Every product is brought to unit
 * amplitude before it is summed, so a sample counts by its phase step alone and a filter that takes amplitude from one side of the
 * spectrum no longer pulls the sum to the other: behind the DEFAULT 10 kHz filter the burst estimate has the right sign and stays within
 * 26 Hz of what was sent out to +-2.5 kHz (CPU measurement, DESIGN.md 4.7g: +1500 Hz reads +1495 where A reads -475), and on the IQ
 * seam it is the better of the two at every level tried.  Use it wherever a channel filter stands in front; A remains for callers who
 * want the amplitude weighting (noise-only blocks count little in A and fully in U).
 * Block j of row c is  U[c][j] = 2^-8 * sum over s = 256 j ... 256 j + 255 of u(s),  u(s) = p(s) / |p(s)|,  p(s) = (re(s), im(s)) exactly
 *   the two fp32 fma expressions above.  u(s) = (0, 0) where both components of p(s) are zero -- the product with y_c[origin - 1] = 0 is
 *   one such term -- and where a component of p(s) is not finite (fc32 input only).  The divisor stays 2^8 whatever the number of
 *   zero terms.  An unmodulated carrier reads e^(j 2 pi f / fs) whatever its amplitude.
 * Normalisation, ONE sequence, fp32, independent of re^2 + im^2 fitting the format: with e the binary exponent of the larger of |re|,
 *   |im| (that magnitude = f 2^e, 0.5 <= f < 1, subnormals included), re' = re 2^-e and im' = im 2^-e (exact scalings);
 *   m = fma(im', im', re' * re'), which lies in [0.25, 2); r = the device's reciprocal square root of m (v_rsq_f32, within 1 ulp, NOT
 *   correctly rounded); u = (re' * r, im' * r).
 * Summation: lane grouping, ascending order, the xor butterfly 32 ... 1 and the exact times 2^-8 are those of A, on u(s) in place of the
 *   product.  Values are bit-identical however the stream is cut into pushes, whatever ld, residence or integer format.
 * Error, against u computed exactly from the fp32 samples, for products that are normal fp32 numbers (a product that underflows has
 *   lost bits before it is normalised): p carries at most 2 u |p| (u = 2^-24) even where one component cancels, the
 *   normalisation about 4 u more (m's two roundings halved by the root, 1 ulp of the root, one multiply), so a term is within about 6 u of
 *   the exact unit vector; the 255 additions add at most 255 u times the sum of |terms| <= 256.  Each component of U lies within
 *   261 * 2^-24 = 1.6e-5 of exact, ABSOLUTE (|U| <= 1).  Because the root is not correctly rounded this is a bound against the CPU model,
 *   not bit equality with it.
 * amps_recc_channel_autocorr, _burst_autocorr and _burst_offset return U, its sum over a capture's blocks and that sum's argument in
 *   Hz, with every rule stated for A.  |sum of U| / n_blocks lies in [0, 1] and is a COHERENCE figure: near 1 for a clean carrier or
 *   a strong burst, falling towards 0 as noise takes over; it is read from amps_recc_burst_autocorr and needs no entry point.
 * Cost: as A plus the normalisation's arithmetic; the kernel reads the same bytes. */
/* out[(row * out_ld + i) * 2 + {0, 1}] = {re, im} of A[row][first_block + i], i < n, into host memory out[rows][out_ld][2], once the
 * pushes enqueued so far have finished; *rows = n_channels, *produced_blocks = one past the newest block (either may be NULL).  n = 0
 * only reports.  -ERANGE outside the held window; -EINVAL for a null handle, or out == NULL / out_ld < n with n > 0; -ESTALE as the
 * data seams.  Changes nothing. */
int amps_recc_channel_autocorr(amps_recc_t *h, uint64_t first_block, size_t n, float *out, size_t out_ld,
                               uint32_t *rows, uint64_t *produced_blocks);
/* Burst sum: for each of the n records (host array; only `channel` and `position` are read) the fp32 sum of A[channel][j] over the
 * blocks that lie wholly inside the capture -- j0 = ceil(position / 256) ... j1 = floor((position + AMPS_RECC_CAPTURE_SYMS *
 * samples_per_symbol) / 256) - 1, the blocks of burst power -- into sum[2 i] (re) and sum[2 i + 1] (im), and their number j1 - j0 + 1
 * into n_blocks[i].  Order, each component alone: lane l adds 0 + A[j0 + l] + A[j0 + l + 64] + ... ascending, then the butterfly
 * o = 32 ... 1 as above; no division.  If any of those blocks is not held: {0.0f, 0.0f} and 0, which is not an error.
 * channel >= n_channels: -EINVAL, before any wait (as for a null handle or null arrays with n > 0). */
int amps_recc_burst_autocorr(amps_recc_t *h, const amps_recc_burst_t *recs, size_t n, float *sum, uint32_t *n_blocks);
/* Burst offset in Hz: of the same sums, offset_hz[i] = (float)(atan2((double)im, (double)re) * fs / (2 pi)), fs = 20000 *
 * samples_per_symbol, computed on the host in double and rounded to float once; n_blocks[i] as above.  0.0f when n_blocks[i] == 0 or
 * both sums are zero.  Positive: the mobile is above the channel centre.  Unambiguous within +- fs / 2.  Errors as
 * amps_recc_burst_autocorr. */
int amps_recc_burst_offset(amps_recc_t *h, const amps_recc_burst_t *recs, size_t n, float *offset_hz, uint32_t *n_blocks);

/* ---- one band over the GPUs of a node (BASELINE configs[4]: "RCCL broadcast of wideband IQ over xGMI") ----
 * One process and one handle per GPU, every handle created with cfg.wideband_groups = N, wideband_group = its rank (the reference's
 * channels are independent -- per-instance state only, lib/recc_impl.h:31-43 -- so any split of them is exact).  Rank 0 (or any one
 * rank) calls amps_recc_rccl_unique_id and the application carries the 128 bytes to the other ranks (a file, MPI,
 * torch.distributed's store: the control plane is the application's); every rank then calls amps_recc_rccl_init and from then on
 * amps_recc_push_wideband_dist (or _bcast) in step.  RCCL is loaded at run time (librccl.so, or the library the environment
 * variable AMPS_RECC_RCCL_LIB names); -ENOSYS where it is absent.  nranks = 1 is valid.
 *
 * No rank is ever left waiting inside a collective (round 5):
 *  - everything that can fail on one rank is checked or allocated BEFORE a collective and travels through it as a status word (a
 *    16-byte all-gather in front of every push and every gather): either all ranks run the data collective or none does, and all of
 *    them return an error -- the rank's own, or -EREMOTEIO on the ranks that were fine.  The communicator stays usable;
 *  - every wait of the host is bounded (amps_recc_rccl_set_timeout, default 30 s, or AMPS_RECC_RCCL_TIMEOUT_MS at init): when the
 *    other ranks do not answer the communicator is aborted and the call returns -ETIMEDOUT; from then on the collective entry
 *    points answer -ENOTCONN.  Since round 6 the bound holds for EVERY wait that can sit behind a collective -- amps_recc_drain /
 *    _drain_end / _drain_bursts, amps_recc_reset, amps_recc_rccl_info and amps_recc_destroy as well;
 *  - an aborted collective lets the kernels queued behind it run on a receive buffer that never received: what the handle found
 *    since its last drain is void and its stream state has advanced over garbage.  The data seams and the drains therefore answer
 *    -ESTALE after a communicator died (timeout, error or amps_recc_rccl_abort) until amps_recc_reset has been called; then the handle
 *    decodes again, on its own (amps_recc_push_wideband) or with a new communicator;
 *  - a rank that has to leave (its flow graph stops, its device failed) calls amps_recc_rccl_abort: its peers then run into their
 *    bound instead of waiting for ever.
 *
 * amps_recc_rccl_init is itself a collective: it returns when all nranks have joined AND compared notes.  -EINVAL on a handle built
 * with wideband_groups = G >= 2 unless nranks == G and rank == wideband_group (it would decode part of the band and nobody the
 * rest), or when the ranks' handles were built for different group counts; -EREMOTEIO where another rank failed; in all those
 * cases every rank returns an error and no rank keeps a communicator.  The receive buffers (2 x the largest push) and the gather
 * buffers are allocated here, for the capacities the ranks have in common: the smallest max_samples_per_push, the largest
 * max_bursts.  Only a rank that cannot join at all (no id, rank outside 0 .. nranks - 1: -EINVAL at once) leaves the others
 * waiting in RCCL's own bootstrap. */
#define AMPS_RECC_RCCL_ID_BYTES 128
int amps_recc_rccl_unique_id(uint8_t id[AMPS_RECC_RCCL_ID_BYTES]);
int amps_recc_rccl_init(amps_recc_t *h, const uint8_t id[AMPS_RECC_RCCL_ID_BYTES], int nranks, int rank);
int amps_recc_rccl_set_timeout(amps_recc_t *h, uint32_t milliseconds);
int amps_recc_rccl_abort(amps_recc_t *h);
/* How the step's block travels root -> everybody:
 *   BROADCAST          one flat ncclBroadcast: every xGMI link out of the root carries the whole block B;
 *   SCATTER_ALLGATHER  the root sends rank k its N-th of the block (ncclSend / ncclRecv in one group), then one ncclAllGather, in place:
 *                      B/N per link and phase (~4x less time at N = 8).
 * Both deliver the same bytes: the records do not depend on the mode. */
#define AMPS_RECC_DIST_BROADCAST         0
#define AMPS_RECC_DIST_SCATTER_ALLGATHER 1
/* Every rank in step, with the same root and mode.  The root passes its block (`mem` says where it lives) and its size; the other
 * ranks' iq / nsamp are ignored (NULL, 0): the ROOT's nsamp is what every rank pushes -- it travels in the header, so callers whose
 * block sizes cannot be agreed beforehand (GNU Radio schedulers in different processes) need no side channel -- and comes back in
 * *npushed (may be NULL).  The block is distributed on a stream of the library's own into one of two receive buffers and pushed
 * through the wideband seam of every rank (amps_recc_push_wideband on the received block), the collective of push i beside the
 * kernels of push i - 1.  Ownership of the root's block: a HOST block has been staged when the call returns and is free; a DEVICE
 * block is read in place, behind everything enqueued on the handle's stream so far (so amps_recc_wait_event orders it behind its
 * producer), and may be overwritten by work that is ordered behind a LATER call on this handle (amps_recc_record_event) or after a
 * drain that covers this push.  Records are drained per rank as ever (or by amps_recc_drain_gather) and carry whole-band channel numbers.
 * END OF STREAM: the root passing (iq = NULL, nsamp = 0) says it has no more samples -- every rank returns -ENODATA from that call, no
 * data collective runs, nothing is pushed, the communicator stays up (a later call with samples continues the stream).  Ranks whose
 * own sources end at other times than the root's keep calling until they see it.
 * Errors: the root's -EINVAL (a block without samples or samples without a block, unknown mode) / -E2BIG (beyond the smallest rank's
 * capacity) with -EREMOTEIO on the other ranks; -EINVAL everywhere when the ranks pass different modes; -ETIMEDOUT / -ENOTCONN / -EIO:
 * see above. */
int amps_recc_push_wideband_dist(amps_recc_t *h, const float *iq, size_t nsamp, int mem, int root, int mode, size_t *npushed);
/* = amps_recc_push_wideband_dist(h, iq, nsamp, mem, root, AMPS_RECC_DIST_BROADCAST, NULL) */
int amps_recc_push_wideband_bcast(amps_recc_t *h, const float *iq, size_t nsamp, int mem, int root);
/* The collective drain that goes with it (the burst records back to one place): every rank calls it in step; each
 * drains its own list as amps_recc_drain does (no split drain may be open) and the records of all ranks arrive at `root`, merged
 * and sorted by (channel, position) -- what one whole-band handle would have returned.  The other ranks get *nout = 0 and may pass
 * out = NULL, cap = 0.  -ENOSPC on every rank if any rank's list overflowed max_bursts (and on the root if cap is too small; what
 * fits is returned), -EIO (or the rank's own error) on every rank if any rank's drain failed -- that rank still takes part and says
 * so in the status word.  The header exchange ({status, count}), then one ncclAllGather of the lists padded to the longest; the wait
 * for the handle's own kernels (which wait for the data collectives) is bounded like every other: -ETIMEDOUT. */
int amps_recc_drain_gather(amps_recc_t *h, amps_recc_burst_t *out, size_t cap, size_t *nout, int root);
/* What the communicator of this handle is, as RCCL itself reports it, and on which device -- enough for a record of an N-GPU run to
 * prove N distinct devices and N ranks by itself (a handle without a communicator: nranks = 0, the device fields are filled).  collective_* : the data collectives of push_wideband_dist timed with HIP events
 * on the library's stream (handles with kernel timing on: AMPS_RECC_FLAG_TIME_KERNELS / amps_recc_set_timing), bytes = block sizes. */
typedef struct amps_recc_rccl_info {
    uint32_t struct_size;
    int32_t  alive;                 /* 1: communicator usable; 0: aborted (timeout / amps_recc_rccl_abort)            */
    int32_t  nranks, rank;          /* as passed to amps_recc_rccl_init                                                */
    int32_t  comm_nranks, comm_rank;/* ncclCommCount / ncclCommUserRank of the communicator (-1: not available)       */
    int32_t  device;                /* HIP device ordinal of the handle                                                */
    int32_t  pci_domain, pci_bus, pci_device;
    uint8_t  device_uuid[16];       /* hipDeviceProp_t::uuid                                                           */
    uint64_t max_samples_per_push;  /* common capacity of the ranks' handles (samples per block)                      */
    uint32_t max_bursts_per_gather; /* longest record list of any rank                                                 */
    uint32_t timeout_ms;
    uint64_t collectives_timed;     /* data collectives whose events have been read                                    */
    double   collective_ms;         /* their summed duration                                                           */
    uint64_t collective_bytes;      /* their summed block bytes                                                        */
    int32_t  last_mode;             /* AMPS_RECC_DIST_* of the last push, -1 before the first                          */
    int32_t  _pad;
    char     library[96];           /* the name librccl was loaded by                                                  */
} amps_recc_rccl_info_t;
int amps_recc_rccl_info(amps_recc_t *h, amps_recc_rccl_info_t *info);

/* test tap of slicer spec D's bit logic, evaluated ON THE HOST by the very functions the kernels inline (no device needed):
 *   form 0: the streaming kernel's 32-sample window, oldest sample at bit 0: in = {SX, ST, SC}; out[0] = the slicer bits, exact from bit
 *           `sps` on (sps = any supported samples-per-symbol);
 *   form 1: the filter bank's word, newest frame at bit 0, sps = 3 or 2 frames per symbol (behind the D = 512 / D = 768 bank): in = {SX,
 *           ST, SC, SX of the previous 32 frames, wp and wm of the previous call}; out = {slicer bits, wp, wm}.
 * 0, or -EINVAL. */
int amps_recc_debug_exact_slice(int form, int sps, const uint32_t *in, uint32_t *out);

/* test tap of the channelizer seam: channelise nsamp wideband samples (continuing the handle's wideband
 * stream) WITHOUT running the RECC kernels; out is host memory [n_channels][out_ld] fc32, *nframes the
 * number of output samples per channel produced. */
int amps_recc_debug_channelize(amps_recc_t *h, const float *iq, size_t nsamp, int mem,
                               float *out, size_t out_ld, size_t *nframes);

int amps_recc_get_timing(amps_recc_t *h, amps_recc_timing_t *t, int reset);
/* HIP-event timing of the launches: OFF, ALL kernels (what AMPS_RECC_FLAG_TIME_KERNELS selects at creation), or only the
 * DOMINANT streaming kernel of the seam in use (front kernel; channelizer on the wideband seam) -- two event records
 * per push instead of ten, for timed regions that should not be perturbed -- or the dominant kernel of every
 * AMPS_RECC_TIMING_SAMPLE_PERIOD-th push only (DOMINANT_SAMPLED: the two event records cost a wideband step 6.5 us = 1.9 %,
 * profiles/r06/event_cost.txt).  Synchronises the stream. */
#define AMPS_RECC_TIMING_OFF      0
#define AMPS_RECC_TIMING_ALL      1
#define AMPS_RECC_TIMING_DOMINANT 2
#define AMPS_RECC_TIMING_DOMINANT_SAMPLED 3
#define AMPS_RECC_TIMING_SAMPLE_PERIOD 8
int amps_recc_set_timing(amps_recc_t *h, int mode);

/* reply generation of recc_decode: fills the focc_words / fvc_words payloads the
 * reference would publish for this burst.  Pure host integer code. */
typedef struct amps_recc_reply {
    uint8_t  has_focc;  int32_t focc_stream; int32_t focc_nwords; uint8_t focc_word1[28]; uint8_t focc_word2[28];
    uint8_t  has_fvc;   int32_t fvc_count;   uint8_t fvc_word1[28]; uint64_t fvc_repeat;
    uint8_t  has_mutes; uint8_t fvc_mute;    uint8_t audio_mute;
    uint8_t  has_command; char command[48];
} amps_recc_reply_t;
int amps_recc_reply_words(const amps_recc_burst_t *burst, amps_recc_reply_t *reply);

/* BCH(63,51,t=2) shortened to (k+12,k) on the device, one code word per lane: k = 36 -> RECC (48,36),
 * k = 28 -> FOCC/FVC (40,28) as encoded by focc_impl::focc_bch / fvc_impl::fvc_bch (lib/focc_impl.cc:156-176,
 * lib/fvc_impl.cc:98-107).  Bits are one byte each, MSB first; arrays are [nwords][k] / [nwords][k+12], host or
 * device per `mem`; results are host arrays.  valid[i] = 1 iff the word decodes with no correction inside the
 * 63-(k+12) shortening positions. */
int amps_bch_encode_words(amps_recc_t *h, const uint8_t *msg, size_t nwords, int k, int mem, uint8_t *codewords);
int amps_bch_decode_words(amps_recc_t *h, const uint8_t *codewords, size_t nwords, int k, int mem,
                          uint8_t *msg, uint8_t *valid, uint8_t *nerrors);

#ifdef __cplusplus
}
#endif
#endif /* AMPS_RECC_H */
