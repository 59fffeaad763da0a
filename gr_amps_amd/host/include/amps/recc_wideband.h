// gr::amps::recc_wideband -- NEW block type (not in the reference): the whole AMPS band in one block.
// Input: ONE gr_complex stream at 1024 x 30 kHz = 30.72 Msps (fc32); the block runs the 1024-branch polyphase channelizer with the
// RECC front end fused behind its FFT on the MI355X (amps_recc_push_wideband) and stands where the reference would need, PER
// CHANNEL, the chain freq_xlating_fir_filter_ccc -> analog_quadrature_demod_cf -> digital_clock_recovery_mm_ff ->
// digital_binary_slicer_fb -> amps_recc (grc/recctest.grc:889-937, 458, 846-874, 807, 310), 832 times over.
// Message ports:  "bursts"  pmt::cons(from_long(channel), blob(3374)) -- cdr = what amps_recc publishes (lib/recc_impl.cc:126);
//                 "records" pmt::cons(from_long(channel), blob(amps_recc_burst_t)) -- the burst already decoded;
//                 "power"   (blocks made with channel_power = true only) pmt::cons(from_long(channel), blob(8)) for every record, behind its
//                           "records" message: the 8 bytes are { float mean_power; uint32_t n_snaps; } in host byte order, as
//                           amps_recc_burst_power returns them -- the mean |filter-bank output|^2 of the record's channel over its capture
//                           (linear, unscaled: 1.0 for a mobile at full scale of an fc32 stream, the input's own units squared behind an integer format) and
//                           the number of power snapshots averaged (26 / 27 at decim 768, 39 / 40 at 512; 0 with power 0.0 if the handle no
//                           longer held them).  The block drains after every push, so every record is covered.
//                 "seizures" (blocks made with seizure_events = true only) pmt::cons(from_long(channel), blob(32)): one amps_recc_seizure_t
//                           (include/amps_recc_seizure.h) per seizure, published from the work() call whose push accepted its trigger, in
//                           front of that call's records -- some 170 ms before the seizure's own record: what an FOCC block needs to
//                           set its busy-idle bits in time.  Behind set_rccl a rank publishes its own group's events.
//                 "early" (blocks made with early_messages = true only) pmt::cons(from_long(channel), blob(744)): one amps_recc_early_t
//                           (include/amps_recc_early.h: the record of the message's announced words, found_at, n_words) per seizure whose
//                           word A announced fewer than seven words, published from the work() call whose push brought the last of
//                           them, in front of that call's records: what a base station answers from, 120 or 96 ms before the record
//                           that repeats it.  Behind set_rccl a rank publishes its own group's messages.
// With channels = 512, 256 or 128 the input is a stream at channels x 30 kHz = 15.36, 7.68 or 3.84 Msps -- what one SDR delivers -- through
// the bank of that many branches, in the two-kernel form (cfg.wideband_channels of include/amps_recc.h); "power" then carries the stream
// power of the IQ seam (AMPS_RECC_FLAG_STREAM_POWER: the mean of |y|^2 over the blocks of 256 channel-rate samples inside the capture).
// Bin channels / 2 is centred on +- fs / 2, where the radio's own anti-alias filter rolls off: a channel there is as good as the radio.
// With channels = 2500, 2000, 1000 or 500 and decim = channels / 4 the input is a stream at channels x 10 kHz = 25, 20, 10 or 5 Msps --
// a radio on a 100 or 200 MHz clock, a 10 Msps dongle -- through the bank of that many branches of 10 kHz, likewise in the two-kernel
// form: a 30 kHz channel on every third bin, channel c = bin (first_bin + 3 c) mod channels, n_channels <= channels / 3, 40 ksps per
// channel.  first_bin then counts 10 kHz bins: a tuner on any multiple of 10 kHz puts every channel centre on a bin.
// channel 0 = FFT bin `first_bin` (centre first_bin x 30 kHz above the stream's centre, modulo the sample rate).
#pragma once
#include <amps/api.h>
#include <string>

namespace gr {
namespace amps {

class AMPS_API recc_wideband : virtual public gr::sync_block {
public:
    typedef AMPS_SPTR<recc_wideband> sptr;
    // slicer: -1 = the library default (spec D since round 4), 0 = numeric spec A (arctangent discriminator + boxcar), 1 = spec B,
    //         2 = spec C, 3 = spec D (include/amps_recc_numerics.h)
    // groups / group: one band over the GPUs of a node (BASELINE configs[4]).  groups = 2, 4 or 8: this block (one flow graph and one
    //         process per GPU, every one fed the same stream) decodes interleaved channel group `group` only -- cfg.wideband_groups of
    //         include/amps_recc.h; channel numbers on the ports stay whole-band numbers.
    // decim: input samples per filter-bank frame, 512 (60 ksps per channel) or 768 (40 ksps); 0 = amps_recc_default_wideband_decim()
    // short_input: the input item is two shorts -- interleaved 16-bit I/Q, what a UHD source set to sc16 or an "interleaved short" file
    //         source delivers -- instead of one gr_complex; the block pushes it as it is (amps_recc_push_wideband_short: 4 bytes per
    //         sample to the device, no float copy on the host).  Scale does not matter to any slicer spec.  set_rccl is refused on such
    //         a block: the distributed seam carries fc32.
    // channel_power: keep per-channel received power (AMPS_RECC_FLAG_CHANNEL_POWER) and publish every record's burst power on "power"
    // channels: branches of the filter bank = 30 kHz channels across the stream: 1024, or 512, 256, 128 (n_channels <= channels, first_bin <
    //         channels; decim = channels / 2 or 3 channels / 4, 0 = the latter; groups and set_rccl belong to 1024); or 2500, 2000, 1000,
    //         500 branches of 10 kHz: make(n_channels <= channels / 3, first_bin, ..., decim = channels / 4, ..., channels, input_format),
    //         e.g. decim = 500, channels = 2000 for 20 Msps -- the decimation has to be stated there, 0 is refused
    // input_format: AMPS_RECC_SAMPLES_* of include/amps_recc.h.  0 = one gr_complex per item (or two shorts behind short_input = true,
    //         which keeps meaning format 1); 1 (sc16) = two shorts; 2 (sc8) = two signed bytes, what a HackRF streams at 3.84 to
    //         15.36 Msps; 3 (cu8) = two offset-binary bytes.  Items of 8, 4, 2 and 2 bytes, pushed as they are
    //         (amps_recc_push_wideband_as: no float copy on the host).  A non-zero input_format other than 1 together with
    //         short_input = true throws, as does an unknown format; set_rccl is refused on every integer format.
    // shift_hz: the tuner's frequency error, corrected inside the filter bank (amps_recc_set_wideband_shift: every bank but the 1024
    //         one): the frequency in the delivered stream of what shall land on bin 0's centre, +e for a radio that delivers
    //         everything e hertz too high.  0 = none.  A non-zero shift on a 1024 bank, or beyond +- fs / 2, throws.
    // rate_hz, interp, decim_in: a stream at a rate that is no bank's (amps_recc_set_wideband_resample): the items arrive at rate_hz and are
    //         resampled by interp / decim_in to the bank's rate on the device -- a HackRF's 8 Msps x 5/4 into channels = 1000, 12.5 Msps x 2/1
    //         into 2500; amps_recc_wideband_resample_plan lists what a rate admits.  rate_hz = 0: none.  A ratio or rate the library refuses
    //         throws.  Not with set_rccl, which throws on such a block: the library has no distributed push behind a resampler (-ENOSYS).
    // seizure_events: keep seizure events (AMPS_RECC_FLAG_SEIZURE_EVENTS) and publish them on "seizures"
    // early_messages: keep early messages (AMPS_RECC_FLAG_EARLY_MESSAGES) and publish them on "early"
    static sptr make(int n_channels = 832, int first_bin = 96, int slicer = -1, int groups = 0, int group = 0, int decim = 0, bool short_input = false,
                     bool channel_power = false, int channels = 1024, int input_format = 0, double shift_hz = 0.0,
                     double rate_hz = 0.0, int interp = 1, int decim_in = 1, bool seizure_events = false, bool early_messages = false);
    // Replace the shift in mid-stream: in force from the next work() call on, nothing reset, and from then on the bank delivers what a
    // block made with this shift would.  Throws where the library refuses (NaN, beyond +- fs / 2, a 1024 bank).
    virtual void set_shift(double shift_hz) = 0;
    // Let ONE rank own the stream: after this call (a collective over all `nranks` blocks; `id` = the 128 bytes one of them got from
    // rccl_unique_id(), carried between the processes by the application) work() distributes rank `root`'s input over xGMI with RCCL
    // inside amps_recc_push_wideband_dist (mode 0 = flat broadcast, 1 = scatter + all-gather: AMPS_RECC_DIST_*).  The other ranks'
    // input only paces their flow graphs and is ignored -- INCLUDING ITS ITEM COUNTS: GNU Radio's schedulers in different processes do
    // not hand out the same noutput_items sequence, so the block never puts its own count into a collective.  The root cuts its input
    // into blocks of at most 2^22 samples, one collective per block, each carrying its size in the library's header; the ranks stay in
    // step by STREAM POSITION: a non-root rank joins collectives -- of whatever size the root announces -- until the root's stream has
    // covered the items its own pacing input has offered (feed it a null source behind a throttle at the root's sample rate).
    // A rank whose push or drain fails aborts its communicator before it returns WORK_DONE
    // (amps_recc_rccl_abort): its peers' bounded waits then end with -ETIMEDOUT instead of never.
    virtual void set_rccl(const std::string &id, int nranks, int rank, int root = 0, int mode = 0) = 0;
    static std::string rccl_unique_id();
};

} // namespace amps
} // namespace gr
