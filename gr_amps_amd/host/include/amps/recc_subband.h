// gr::amps::recc_subband -- NEW block type (not in the reference): many 30 kHz channels of ONE narrowband stream in one block.
// Input: ONE gr_complex stream at rate_hz (a few hundred ksps to 3.2 Msps: one modest SDR tuned to a system's control channels), or
// with input_format the SDR's own integer items;
// the block runs, for every centre of centers_hz, the flow graph's channel filter freq_xlating_fir_filter_ccc(decim,
// firdes.low_pass(3, rate, cutoff, width), centre, rate) (grc/recctest.grc:889-937, taps :115-155) and the fused chain behind it
// on the MI355X -- amps_recc_set_xlate_shared / amps_recc_push_raw_shared: all channels in one launch per stage -- and stands
// where the reference would need that filter plus analog_quadrature_demod_cf -> digital_clock_recovery_mm_ff ->
// digital_binary_slicer_fb -> amps_recc (:458, 846-874, 807, 310) once per channel.
// Message ports:  "bursts"  pmt::cons(from_long(channel), blob(3374)) -- cdr = what amps_recc publishes (lib/recc_impl.cc:126);
//                 "records" pmt::cons(from_long(channel), blob(amps_recc_burst_t)) -- the burst already decoded;
//                 "power"   (blocks made with channel_power = true only) pmt::cons(from_long(channel), blob(8)) for every record, behind
//                           its "records" message: the 8 bytes are { float mean_power; uint32_t n_snaps; } in host byte order, as
//                           amps_recc_burst_power returns them -- the mean |channel filter output|^2 over the record's capture, linear and
//                           unscaled (RSSI up to a constant), and the number of 256-sample power blocks averaged (130 / 131 at 10 samples
//                           per symbol; 0 with power 0.0 if the handle no longer holds them);
//                 "offset"  (blocks made with channel_offset = true only) pmt::cons(from_long(channel), blob(8)) for every record, behind
//                           its "records" (and "power") message: { float offset_hz; uint32_t n_blocks; } as amps_recc_burst_offset returns
//                           them -- how far the mobile's carrier stands from centers_hz[channel], positive above it, and the number of
//                           256-sample blocks it was read from (0 with 0.0 Hz if the handle no longer holds them).  Behind the default
//                           10 kHz cut-off the figure is not usable -- the filter cuts the side of the signal the offset moved outwards,
//                           and the estimate leans the other way; with cutoff_hz = 16e3 it reads about 5 % low.  With
//                           offset_unit = true the figure is the unit-amplitude statistic's (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT), which
//                           is usable behind the default filter: within 26 Hz out to +-2.5 kHz (same section);
//                 "seizures" (blocks made with seizure_events = true only) pmt::cons(from_long(channel), blob(32)): one amps_recc_seizure_t
//                           (include/amps_recc_seizure.h) per seizure, published from the work() call whose push accepted its trigger, in
//                           front of that call's records -- some 170 ms before the seizure's own record;
//                 "early" (blocks made with early_messages = true only) pmt::cons(from_long(channel), blob(744)): one amps_recc_early_t
//                           (include/amps_recc_early.h: the record of the message's announced words, found_at, n_words) per seizure whose
//                           word A announced fewer than seven words, published from the work() call whose push brought the last of
//                           them, in front of that call's records; the record that repeats it has its (channel, position);
// as gr::amps::recc_wideband publishes them.  channel c = the channel at centers_hz[c] relative to the stream's centre.
#pragma once
#include <amps/api.h>
#include <vector>

namespace gr {
namespace amps {

class AMPS_API recc_subband : virtual public gr::sync_block {
public:
    typedef AMPS_SPTR<recc_subband> sptr;
    // rate_hz / decim must be samples_per_symbol x 20 kHz; decim: 1, 2, 4, 5, 6, 8, 10, 12, 16 or 20 (2.4 Msps / 12, 2.0 / 10, 3.2 / 16 ...);
    // a refused combination is answered with what the rate admits (amps_recc_xlate_shared_plan)
    // slicer: -1 = the library default, 0 .. 3 = numeric spec A .. D (include/amps_recc_numerics.h)
    // cutoff_hz / width_hz: 0 = the flow graph's 10 kHz / 4.5 kHz
    // interp: 1 = decimation alone (the above); 2 ... 5 = the rational resampler, the stream resampled by interp / decim for the rates no
    //         decimation serves -- 2.048 Msps x 5/64 at 8 samples per symbol, 2.5 Msps x 2/25 at 10 (amps_recc_set_xlate_resampled;
    //         decim up to 64, coprime to interp).  A refused combination is answered with both plans.
    // input_format: AMPS_RECC_SAMPLES_* of include/amps_recc.h.  0 = one gr_complex per item; 1 (sc16) = two shorts, what a UHD source set
    //         to sc16 or an "interleaved short" file source delivers; 2 (sc8) = two signed bytes (HackRF); 3 (cu8) = two offset-binary
    //         unsigned bytes (RTL-SDR).  The block pushes the items as they are (amps_recc_push_raw_shared_as: 4 or 2 bytes per sample
    //         to the device, no float copy on the host); the records are those of the plainly converted stream.
    // channel_power: keep per-channel received power (AMPS_RECC_FLAG_STREAM_POWER) and publish every record's burst power on "power"
    // channel_offset: measure the carrier offset (AMPS_RECC_FLAG_STREAM_OFFSET) and publish every record's on "offset"
    // offset_unit: with channel_offset, the unit-amplitude statistic (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT) instead; the port stays "offset"
    // seizure_events: keep seizure events (AMPS_RECC_FLAG_SEIZURE_EVENTS) and publish them on "seizures"
    // early_messages: keep early messages (AMPS_RECC_FLAG_EARLY_MESSAGES) and publish them on "early"
    static sptr make(double rate_hz, const std::vector<double> &centers_hz, int decim = 4, int samples_per_symbol = 10, int slicer = -1,
                     double cutoff_hz = 0.0, double width_hz = 0.0, int input_format = 0, int interp = 1, bool channel_power = false,
                     bool channel_offset = false, bool offset_unit = false, bool seizure_events = false, bool early_messages = false);
    // new centres in mid-stream (amps_recc_retune_xlate): as many as the block was made with; from the next work() call on the stage
    // delivers what a block made with these centres would, and nothing is reset.  Call it from the thread that runs work() (a message
    // handler) or between runs; throws std::runtime_error where the library refuses (another number of centres, one beyond the rate)
    virtual void retune(const std::vector<double> &centers_hz) = 0;
};

} // namespace amps
} // namespace gr
