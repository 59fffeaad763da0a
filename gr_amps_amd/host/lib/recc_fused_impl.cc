// recc_fused_impl.cc -- gr::amps::recc_fused: complex baseband in; on "bursts" the same 3374-byte symbol blob gr::amps::recc
// publishes (lib/recc_impl.cc:126), on "records" the already decoded record.
// Replaces quadrature_demod_cf -> clock_recovery_mm_ff -> binary_slicer_fb -> amps_recc with the fused
// MI355X kernel (amps_recc_push_iq / amps_recc_drain).
#include <amps/recc_fused.h>
#include <cerrno>
#include <cstdio>
#include <stdexcept>
#include <vector>
#include "amps_recc.h"
#include "recc_publish.h"

namespace gr {
namespace amps {

class recc_fused_impl : public recc_fused {
    amps_recc_t *d_handle;
    bool d_raw;
    bool d_power;                                  // AMPS_RECC_FLAG_STREAM_POWER: every record's burst power goes out on "power"
    bool d_offset;                                 // AMPS_RECC_FLAG_STREAM_OFFSET or _OFFSET_UNIT: every record's carrier offset goes out on "offset"
    bool d_seizures;                               // AMPS_RECC_FLAG_SEIZURE_EVENTS: every push's seizure events go out on "seizures"
    bool d_early;                                  // AMPS_RECC_FLAG_EARLY_MESSAGES: every push's early messages go out on "early"
    std::vector<unsigned char> d_bursts;
    static const int kMaxPush = 1 << 20;
    static const int kMaxRecs = 64;

public:
    recc_fused_impl(int sps, double xlate_rate, double xlate_center, int xlate_decim, double xlate_cutoff, double xlate_width, bool channel_power, bool channel_offset,
                    bool offset_unit, bool seizure_events, bool early_messages)
        : gr::sync_block("recc_fused", gr::io_signature::make(1, 1, 2 * sizeof(float)), gr::io_signature::make(0, 0, 0)), d_handle(nullptr),
          d_raw(xlate_rate > 0.0), d_power(channel_power), d_offset(channel_offset), d_seizures(seizure_events), d_early(early_messages), d_bursts((size_t)kMaxRecs * AMPS_RECC_CAPTURE_SYMS)
    {
        amps_recc_cfg_t cfg = {};
        cfg.struct_size = sizeof(cfg);
        cfg.n_channels = 1;
        cfg.samples_per_symbol = (uint32_t)sps;
        cfg.max_samples_per_push = kMaxPush;
        cfg.max_bursts = kMaxRecs;
        cfg.device = -1;
        cfg.flags = AMPS_RECC_FLAG_KEEP_BURSTS | (channel_power ? AMPS_RECC_FLAG_STREAM_POWER : 0u) | (channel_offset ? (offset_unit ? AMPS_RECC_FLAG_STREAM_OFFSET_UNIT : AMPS_RECC_FLAG_STREAM_OFFSET) : 0u)   // the captured symbols travel with the record
                  | (seizure_events ? AMPS_RECC_FLAG_SEIZURE_EVENTS : 0u) | (early_messages ? AMPS_RECC_FLAG_EARLY_MESSAGES : 0u);
        int rc = amps_recc_create(&d_handle, &cfg);
        if (rc != 0) throw std::runtime_error(std::string("amps::recc_fused: ") + amps_recc_strerror(rc));
        if (d_raw) {
            amps_recc_xlate_cfg_t x = {};
            x.struct_size = sizeof(x);
            x.decim = (uint32_t)xlate_decim;
            x.rate_hz = xlate_rate;
            x.center_hz = xlate_center;
            x.cutoff_hz = xlate_cutoff;                    // 0 = the flow graph's 10 kHz / 4.5 kHz
            x.width_hz = xlate_width;
            rc = amps_recc_set_xlate(d_handle, &x);
            if (rc != 0) {
                amps_recc_destroy(d_handle);
                throw std::runtime_error(std::string("amps::recc_fused (xlate): ") + amps_recc_strerror(rc));
            }
        }
        message_port_register_out(pmt::mp("bursts"));          // what amps_recc publishes: connects to amps_recc_decode unchanged
        message_port_register_out(pmt::mp("records"));         // the same burst already decoded (recc_decode accepts it too)
        if (d_power) message_port_register_out(pmt::mp("power"));
        if (d_offset) message_port_register_out(pmt::mp("offset"));
        if (d_seizures) message_port_register_out(pmt::mp("seizures"));
        if (d_early) message_port_register_out(pmt::mp("early"));
    }
    ~recc_fused_impl() { amps_recc_destroy(d_handle); }

    void retune(double xlate_center_hz) override
    {
        const int rc = amps_recc_retune_xlate(d_handle, &xlate_center_hz, 1);
        if (rc != 0) throw std::runtime_error(std::string("amps::recc_fused (retune): ") + amps_recc_strerror(rc));
    }

    int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &)
    {
        const float *in = (const float *)input_items[0];
        int done = 0;
        while (done < noutput_items) {
            int n = noutput_items - done;
            if (n > kMaxPush) n = kMaxPush;
            int rc = d_raw ? amps_recc_push_raw(d_handle, in + 2 * (size_t)done, (size_t)n, (size_t)n, AMPS_MEM_HOST)
                           : amps_recc_push_iq(d_handle, in + 2 * (size_t)done, (size_t)n, (size_t)n, AMPS_MEM_HOST);
            if (rc != 0) { std::fprintf(stderr, "amps::recc_fused: %s\n", amps_recc_strerror(rc)); return WORK_DONE; }
            if (d_seizures && !recc_publish_seizures(*this, "recc_fused", d_handle)) return WORK_DONE;
            if (d_early && !recc_publish_early(*this, "recc_fused", d_handle)) return WORK_DONE;
            amps_recc_burst_t recs[kMaxRecs];
            float pow[kMaxRecs];
            uint32_t nsnap[kMaxRecs];
            float off[kMaxRecs];
            uint32_t offn[kMaxRecs];
            if (!recc_drain_and_publish(*this, "recc_fused", false, d_handle, recs, d_bursts.data(), kMaxRecs, d_power ? pow : nullptr, d_power ? nsnap : nullptr,
                                        d_offset ? off : nullptr, d_offset ? offn : nullptr))
                return WORK_DONE;
            done += n;
        }
        consume_each(noutput_items);
        return 0;
    }
};

recc_fused::sptr recc_fused::make(int samples_per_symbol, double xlate_rate_hz, double xlate_center_hz, int xlate_decim, double xlate_cutoff_hz, double xlate_width_hz,
                                  bool channel_power, bool channel_offset, bool offset_unit, bool seizure_events, bool early_messages)
{
    return gnuradio::get_initial_sptr(new recc_fused_impl(samples_per_symbol, xlate_rate_hz, xlate_center_hz, xlate_decim, xlate_cutoff_hz, xlate_width_hz,
                                                          channel_power, channel_offset, offset_unit, seizure_events, early_messages));
}

} // namespace amps
} // namespace gr
