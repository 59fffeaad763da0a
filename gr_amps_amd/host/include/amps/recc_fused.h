// gr::amps::recc_fused -- NEW block type (not in the reference): replaces the whole sub-chain
//   quadrature_demod_cf -> clock_recovery_mm_ff -> binary_slicer_fb -> amps_recc   (grc/ampsbs.grc:775,1752,1713,497)
// with the fused MI355X kernel.  Input: one gr_complex stream at samples_per_symbol * 20 kHz
// (200 ksps for the flow graphs as wired); output: the same "bursts" message port as gr::amps::recc,
// so amps_recc_decode connects to it unchanged.  It additionally publishes the already decoded
// record on port "records" (blob of amps_recc_burst_t).
// With xlate_rate_hz > 0 it also absorbs the flow graph's channel filter (freq_xlating_fir_filter_ccc with the
// firdes.low_pass taps, grc/recctest.grc:889-937, :115-155): the input is then the raw capture rate (400 ksps in
// recctest.grc) with the channel at xlate_center_hz, and xlate_rate_hz / xlate_decim = samples_per_symbol * 20 kHz.
// xlate_cutoff_hz / xlate_width_hz = 0 keep the flow graph's 10 kHz / 4.5 kHz.  A mobile whose carrier is off by 2 kHz loses half its
// bursts at 12 dB C/N behind THAT filter (it cuts into a signal it no longer centres) and none behind a 14 kHz one of the same length
// (profiles/r06/cfo_filter_width.txt): a receiver that expects carrier offsets sets xlate_cutoff_hz = 14e3.
// channel_power = true keeps received power (AMPS_RECC_FLAG_STREAM_POWER) and adds the port "power": behind each "records" message
// pmt::cons(from_long(0), blob{ float mean_power; uint32_t n_snaps }), the mean |sample|^2 of what the kernel sliced (the input, or the
// channel filter's output) over the record's capture and the number of 256-sample blocks averaged, as gr::amps::recc_wideband and
// gr::amps::recc_subband publish it.
// channel_offset = true measures the carrier offset (AMPS_RECC_FLAG_STREAM_OFFSET) and adds the port "offset": behind each "records"
// message pmt::cons(from_long(0), blob{ float offset_hz; uint32_t n_blocks }), amps_recc_burst_offset of the record: how far the mobile's
// carrier stands from the channel centre, and the 256-sample blocks it was read from.  Behind the default 10 kHz channel filter the
// figure is not usable (the filter cuts the side of the signal the offset moved outwards and the estimate leans the other way); set
// xlate_cutoff_hz = 16e3 to steer by it -- or offset_unit = true: with channel_offset = true it selects the
// unit-amplitude statistic (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT), which reads the offset behind the default filter too (+1500 Hz reads
// +1495 Hz where the other reads -475 Hz).  The port stays "offset".
// seizure_events = true keeps seizure events (AMPS_RECC_FLAG_SEIZURE_EVENTS) and adds the port "seizures": pmt::cons(from_long(0),
// blob(32)), one amps_recc_seizure_t (include/amps_recc_seizure.h) per seizure, published from the work() call whose push accepted its trigger,
// in front of that call's records -- some 170 ms before the seizure's own record.
// early_messages = true keeps early messages (AMPS_RECC_FLAG_EARLY_MESSAGES) and adds the port "early": pmt::cons(from_long(0), blob(744)),
// one amps_recc_early_t (include/amps_recc_early.h: the record of the message's announced words, found_at, n_words) per seizure whose
// word A announced fewer than seven words, published from the work() call whose push brought the last of them, in front of that call's
// records -- 120 ms (two words) or 96 ms (three) before the record that repeats it.
// retune(xlate_center_hz) moves the translate stage's centre in mid-stream (amps_recc_retune_xlate): from the next work() call on the
// stage delivers what a block made with that centre would; nothing is reset.  Call it from the thread that runs work() (a message
// handler) or between runs; it throws std::runtime_error where the library refuses (no translate stage, a centre beyond the rate).
#pragma once
#include <amps/api.h>

namespace gr {
namespace amps {

class AMPS_API recc_fused : virtual public gr::sync_block {
public:
    typedef AMPS_SPTR<recc_fused> sptr;
    static sptr make(int samples_per_symbol = 10, double xlate_rate_hz = 0.0, double xlate_center_hz = 0.0, int xlate_decim = 2,
                     double xlate_cutoff_hz = 0.0, double xlate_width_hz = 0.0, bool channel_power = false, bool channel_offset = false,
                     bool offset_unit = false, bool seizure_events = false, bool early_messages = false);
    virtual void retune(double xlate_center_hz) = 0;
};

} // namespace amps
} // namespace gr
