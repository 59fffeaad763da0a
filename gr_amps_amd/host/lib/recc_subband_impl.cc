// recc_subband_impl.cc -- gr::amps::recc_subband: one narrowband complex stream in, (channel, burst) and (channel, record) pairs out.
#include <amps/recc_subband.h>
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "amps_recc.h"
#include "recc_publish.h"

namespace gr {
namespace amps {

class recc_subband_impl : public recc_subband {
    amps_recc_t *d_handle;
    int d_decim, d_interp;                         // the stream is resampled by d_interp / d_decim; interp 1 = decimated
    int d_format;                                  // AMPS_RECC_SAMPLES_*: what one input item holds
    std::vector<amps_recc_burst_t> d_recs;
    std::vector<unsigned char> d_bursts;
    bool d_power = false;                          // AMPS_RECC_FLAG_STREAM_POWER: every record's burst power goes out on "power"
    std::vector<float> d_pow;
    std::vector<uint32_t> d_nsnap;
    bool d_offset = false;                         // AMPS_RECC_FLAG_STREAM_OFFSET or _OFFSET_UNIT: every record's carrier offset goes out on "offset"
    std::vector<float> d_off;
    std::vector<uint32_t> d_offn;
    bool d_seizures = false;                       // AMPS_RECC_FLAG_SEIZURE_EVENTS: every push's seizure events go out on "seizures"
    bool d_early = false;                          // AMPS_RECC_FLAG_EARLY_MESSAGES: every push's early messages go out on "early"
    static const int kMaxOut = 1 << 18;            // channel-rate samples per push: 1.3 s at 200 ksps
    static const int kMaxRecs = 1024;
    // bytes of one input item: two floats, two shorts or two bytes; 0 = no such format
    static size_t item_size(int format)
    {
        return format == AMPS_RECC_SAMPLES_FC32 ? 2 * sizeof(float) : format == AMPS_RECC_SAMPLES_SC16 ? 2 * sizeof(short)
             : format == AMPS_RECC_SAMPLES_SC8 || format == AMPS_RECC_SAMPLES_CU8 ? 2 : 0;
    }

    // what to ask for instead of a refused (rate, decim, samples per symbol): the plan of that rate
    // -- both plans: the integer decimations and the interp / decim ratios of the rational resampler
    static std::string refused(double rate_hz, double width_hz, int decim, int interp, int sps)
    {
        amps_recc_xlate_plan_t plan[16];
        const int n = amps_recc_xlate_shared_plan(rate_hz, width_hz, plan, 16);
        amps_recc_resample_plan_t rplan[16];
        const int nr = amps_recc_xlate_resample_plan(rate_hz, width_hz, rplan, 16);
        char buf[96];
        std::snprintf(buf, sizeof buf, "; asked: %g sps x %d / %d at %d samples per symbol; ", rate_hz, interp, decim, sps);
        std::string s = buf;
        if (n <= 0 && nr <= 0)
            return s + "neither a decimation (1, 2, 4, 5, 6, 8, 10, 12, 16, 20; amps_recc_xlate_shared_plan) nor a ratio interp / decim (interp 2 ... 5, "
                       "decim up to 64; amps_recc_xlate_resample_plan) serves this rate and transition width";
        if (n > 0) s += "this rate admits (decim, samples per symbol, taps):";
        for (int i = 0; i < std::min(n, 16); i++) {
            std::snprintf(buf, sizeof buf, " (%u, %u, %u)", plan[i].decim, plan[i].samples_per_symbol, plan[i].ntaps);
            s += buf;
        }
        if (nr > 0) s += std::string(n > 0 ? "; and" : "this rate admits") + " (interp, decim, samples per symbol, taps per phase):";
        for (int i = 0; i < std::min(nr, 16); i++) {
            std::snprintf(buf, sizeof buf, " (%u, %u, %u, %u)", rplan[i].interp, rplan[i].decim, rplan[i].samples_per_symbol, rplan[i].ntaps_per_phase);
            s += buf;
        }
        return s;
    }

public:
    recc_subband_impl(double rate_hz, const std::vector<double> &centers_hz, int decim, int sps, int slicer, double cutoff_hz, double width_hz, int input_format,
                      int interp, bool channel_power, bool channel_offset, bool offset_unit, bool seizure_events, bool early_messages)
        : gr::sync_block("recc_subband", gr::io_signature::make(1, 1, (int)std::max<size_t>(item_size(input_format), 1)), gr::io_signature::make(0, 0, 0)),
          d_handle(nullptr), d_decim(decim), d_interp(interp), d_format(input_format), d_recs(kMaxRecs), d_bursts((size_t)kMaxRecs * AMPS_RECC_CAPTURE_SYMS),
          d_power(channel_power), d_pow(channel_power ? kMaxRecs : 0), d_nsnap(channel_power ? kMaxRecs : 0),
          d_offset(channel_offset), d_off(channel_offset ? kMaxRecs : 0), d_offn(channel_offset ? kMaxRecs : 0),
          d_seizures(seizure_events), d_early(early_messages)
    {
        if (!item_size(input_format)) throw std::runtime_error("amps::recc_subband: input_format must be 0 (fc32), 1 (sc16), 2 (sc8) or 3 (cu8)");
        if (centers_hz.empty()) throw std::runtime_error("amps::recc_subband: no centres");
        if (decim < 1) throw std::runtime_error("amps::recc_subband: decim must be 1, 2, 4, 5, 6, 8, 10, 12, 16 or 20, or up to 64 behind an interp of 2 ... 5");
        if (interp < 1) throw std::runtime_error("amps::recc_subband: interp must be 1 (decimation alone) or 2 ... 5");
        amps_recc_cfg_t cfg = {};
        cfg.struct_size = sizeof(cfg);
        cfg.n_channels = (uint32_t)centers_hz.size();
        cfg.samples_per_symbol = (uint32_t)sps;
        cfg.max_samples_per_push = kMaxOut;
        cfg.max_bursts = kMaxRecs;
        cfg.device = -1;
        cfg.flags = AMPS_RECC_FLAG_KEEP_BURSTS | (channel_power ? AMPS_RECC_FLAG_STREAM_POWER : 0u) | (channel_offset ? (offset_unit ? AMPS_RECC_FLAG_STREAM_OFFSET_UNIT : AMPS_RECC_FLAG_STREAM_OFFSET) : 0u)
                  | (seizure_events ? AMPS_RECC_FLAG_SEIZURE_EVENTS : 0u) | (early_messages ? AMPS_RECC_FLAG_EARLY_MESSAGES : 0u)
                  | (slicer == 0 ? AMPS_RECC_FLAG_SLICER_ATAN : slicer == 1 ? AMPS_RECC_FLAG_SLICER_PRODUCT
                                                  : slicer == 2 ? AMPS_RECC_FLAG_SLICER_SINE : slicer == 3 ? AMPS_RECC_FLAG_SLICER_EXACT : 0u);
        int rc = amps_recc_create(&d_handle, &cfg);
        if (rc != 0) throw std::runtime_error(std::string("amps::recc_subband: ") + amps_recc_strerror(rc));
        if (interp == 1) {
            amps_recc_xlate_shared_cfg_t x = {};
            x.struct_size = sizeof(x);
            x.decim = (uint32_t)decim;
            x.n_centers = (uint32_t)centers_hz.size();
            x.rate_hz = rate_hz;
            x.cutoff_hz = cutoff_hz;                   // 0 = the flow graph's 10 kHz / 4.5 kHz
            x.width_hz = width_hz;
            x.center_hz = centers_hz.data();
            rc = amps_recc_set_xlate_shared(d_handle, &x);
        } else {                                       // the rational resampler: 2.048 Msps x 5/64, 2.5 Msps x 2/25, ...
            amps_recc_xlate_resample_cfg_t x = {};
            x.struct_size = sizeof(x);
            x.interp = (uint32_t)interp;
            x.decim = (uint32_t)decim;
            x.n_centers = (uint32_t)centers_hz.size();
            x.rate_hz = rate_hz;
            x.cutoff_hz = cutoff_hz;
            x.width_hz = width_hz;
            x.center_hz = centers_hz.data();
            rc = amps_recc_set_xlate_resampled(d_handle, &x);
        }
        if (rc != 0) {
            amps_recc_destroy(d_handle);
            throw std::runtime_error(std::string("amps::recc_subband (xlate): ") + amps_recc_strerror(rc) + refused(rate_hz, width_hz, decim, interp, sps));
        }
        message_port_register_out(pmt::mp("bursts"));
        message_port_register_out(pmt::mp("records"));
        if (d_power) message_port_register_out(pmt::mp("power"));
        if (d_offset) message_port_register_out(pmt::mp("offset"));
        if (d_seizures) message_port_register_out(pmt::mp("seizures"));
        if (d_early) message_port_register_out(pmt::mp("early"));
    }
    ~recc_subband_impl() { amps_recc_destroy(d_handle); }

    void retune(const std::vector<double> &centers_hz) override
    {
        const int rc = amps_recc_retune_xlate(d_handle, centers_hz.data(), centers_hz.size());
        if (rc != 0) throw std::runtime_error(std::string("amps::recc_subband (retune): ") + amps_recc_strerror(rc));
    }

    int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &)
    {
        const unsigned char *in = (const unsigned char *)input_items[0];
        const size_t item = item_size(d_format);
        // a leftover sample of the last push may complete one more output; interp outputs per decim inputs
        const int max_push = (int)((long long)(kMaxOut - 1) * d_decim / d_interp);
        int done = 0;
        while (done < noutput_items) {
            int n = noutput_items - done;
            if (n > max_push) n = max_push;
            int rc = amps_recc_push_raw_shared_as(d_handle, in + item * (size_t)done, (size_t)n, d_format, AMPS_MEM_HOST);
            if (rc != 0) { std::fprintf(stderr, "amps::recc_subband: %s\n", amps_recc_strerror(rc)); return WORK_DONE; }
            if (d_seizures && !recc_publish_seizures(*this, "recc_subband", d_handle)) return WORK_DONE;
            if (d_early && !recc_publish_early(*this, "recc_subband", d_handle)) return WORK_DONE;
            if (!recc_drain_and_publish(*this, "recc_subband", true, d_handle, d_recs.data(), d_bursts.data(), kMaxRecs, d_power ? d_pow.data() : nullptr,
                                        d_power ? d_nsnap.data() : nullptr, d_offset ? d_off.data() : nullptr, d_offset ? d_offn.data() : nullptr))
                return WORK_DONE;
            done += n;
        }
        consume_each(noutput_items);
        return 0;
    }
};

recc_subband::sptr recc_subband::make(double rate_hz, const std::vector<double> &centers_hz, int decim, int samples_per_symbol, int slicer,
                                      double cutoff_hz, double width_hz, int input_format, int interp, bool channel_power, bool channel_offset,
                                      bool offset_unit, bool seizure_events, bool early_messages)
{
    return gnuradio::get_initial_sptr(new recc_subband_impl(rate_hz, centers_hz, decim, samples_per_symbol, slicer, cutoff_hz, width_hz, input_format, interp,
                                                            channel_power, channel_offset, offset_unit, seizure_events, early_messages));
}

} // namespace amps
} // namespace gr
