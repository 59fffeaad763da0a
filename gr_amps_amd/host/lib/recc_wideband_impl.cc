// recc_wideband_impl.cc -- gr::amps::recc_wideband: one 30.72 Msps complex stream (or 15.36, 7.68, 3.84 Msps: channels < 1024; or 25, 20, 10, 5 Msps: channels = 2500 ... 500 of 10 kHz) in, (channel, burst) and (channel, record) pairs out.
#include <amps/recc_wideband.h>
#include <cerrno>
#include <cstdio>
#include <stdexcept>
#include <vector>
#include "amps_recc.h"
#include "recc_publish.h"
#include <string>

namespace gr {
namespace amps {

class recc_wideband_impl : public recc_wideband {
    amps_recc_t *d_handle;
    std::vector<amps_recc_burst_t> d_recs;
    std::vector<unsigned char> d_bursts;
    static const int kMaxPush = 1 << 22;          // wideband samples per push (8192 frames)
    static const int kMaxRecs = 4096;
    bool d_bcast = false;                          // set_rccl: the stream comes from rank d_root by RCCL
    int d_root = 0, d_rank = 0, d_mode = AMPS_RECC_DIST_BROADCAST;
    unsigned long long d_stream_samples = 0, d_paced_items = 0;   // non-root ranks: samples the root has distributed / items this rank's pacing input has offered
    bool d_ended = false;                          // the root's end of stream has been sent (root) / seen (the others)
    int d_format = AMPS_RECC_SAMPLES_FC32;         // AMPS_RECC_SAMPLES_* of the items: one gr_complex, two shorts ("sc16") or two bytes ("sc8", "cu8")
    bool d_resample = false;                       // the items arrive at a rate of their own and reach the bank through the L / M resampler: no set_rccl
    bool d_power = false;                          // AMPS_RECC_FLAG_CHANNEL_POWER: every record's burst power goes out on "power"
    std::vector<float> d_pow;
    std::vector<uint32_t> d_nsnap;
    bool d_seizures = false;                       // AMPS_RECC_FLAG_SEIZURE_EVENTS: every push's seizure events go out on "seizures"
    bool d_early = false;                          // AMPS_RECC_FLAG_EARLY_MESSAGES: every push's early messages go out on "early"

public:
    // bytes of one item of a format; 0: no such format
    static size_t item_size(int format)
    {
        return format == AMPS_RECC_SAMPLES_FC32 ? 2 * sizeof(float) : format == AMPS_RECC_SAMPLES_SC16 ? 2 * sizeof(short)
             : format == AMPS_RECC_SAMPLES_SC8 || format == AMPS_RECC_SAMPLES_CU8 ? 2 : 0;
    }
    // short_input = true keeps meaning format 1; it contradicts every other non-zero format
    static int checked_format(bool short_input, int input_format)
    {
        if (!item_size(input_format)) throw std::runtime_error("amps::recc_wideband: input_format must be 0 (fc32), 1 (sc16), 2 (sc8) or 3 (cu8)");
        if (short_input && input_format != AMPS_RECC_SAMPLES_FC32 && input_format != AMPS_RECC_SAMPLES_SC16)
            throw std::runtime_error("amps::recc_wideband: short_input means input_format 1 (sc16)");
        return short_input ? AMPS_RECC_SAMPLES_SC16 : input_format;
    }

    recc_wideband_impl(int C, int first_bin, int slicer, int groups, int group, int decim, bool short_input, bool channel_power, int channels, int input_format, double shift_hz,
                       double rate_hz, int interp, int decim_in, bool seizure_events, bool early_messages)
        : gr::sync_block("recc_wideband", gr::io_signature::make(1, 1, (int)item_size(checked_format(short_input, input_format))), gr::io_signature::make(0, 0, 0)),
          d_handle(nullptr), d_recs(kMaxRecs), d_bursts((size_t)kMaxRecs * AMPS_RECC_CAPTURE_SYMS), d_format(checked_format(short_input, input_format)), d_power(channel_power),
          d_pow(channel_power ? kMaxRecs : 0), d_nsnap(channel_power ? kMaxRecs : 0), d_seizures(seizure_events), d_early(early_messages)
    {
        amps_recc_cfg_t cfg = {};
        cfg.struct_size = sizeof(cfg);
        cfg.n_channels = (uint32_t)C;
        cfg.samples_per_symbol = 0;                // what goes with the decimation: 3 (60 ksps per channel, D = 512) or 2 (40 ksps, D = 768)
        const bool narrow = channels > 0 && channels != 1024;      // every bank but the 1024 one is the two-kernel form: received power is the IQ seam's
        const int dmin = narrow ? (decim > 0 ? decim : 3 * channels / 4) : 512;   // fewest input samples a frame takes
        const bool resample = rate_hz != 0.0;                      // the input arrives at rate_hz and reaches the bank through the L / M resampler
        if (resample && (interp < 1 || decim_in < 1)) throw std::runtime_error("amps::recc_wideband: resample: interp and decim_in are 1 ... 8");
        // frames of the largest push: behind a resampler kMaxPush items are up to interp / decim_in times as many samples at the bank
        cfg.max_samples_per_push = (uint32_t)((resample ? ((uint64_t)kMaxPush * (uint64_t)interp + decim_in - 1) / decim_in : (uint64_t)kMaxPush) / dmin + 72);
        cfg.max_bursts = kMaxRecs;
        cfg.device = -1;
        cfg.flags = AMPS_RECC_FLAG_KEEP_BURSTS | (slicer == 0 ? AMPS_RECC_FLAG_SLICER_ATAN : slicer == 1 ? AMPS_RECC_FLAG_SLICER_PRODUCT
                                                  : slicer == 2 ? AMPS_RECC_FLAG_SLICER_SINE : slicer == 3 ? AMPS_RECC_FLAG_SLICER_EXACT : 0u)
                    | (channel_power ? (narrow ? AMPS_RECC_FLAG_STREAM_POWER : AMPS_RECC_FLAG_CHANNEL_POWER) : 0u)
                    | (seizure_events ? AMPS_RECC_FLAG_SEIZURE_EVENTS : 0u) | (early_messages ? AMPS_RECC_FLAG_EARLY_MESSAGES : 0u);
        cfg.wideband_groups = (uint32_t)groups;
        cfg.wideband_group = (uint32_t)group;
        cfg.wideband_channels = (uint32_t)channels;
        cfg.wideband_decim = (uint32_t)decim;     // 0 = amps_recc_default_wideband_decim()
        cfg.wideband_taps_per_branch = 0;         // the bank's own: 8, or 3 at the banks of 10 kHz bins
        cfg.wideband_first_channel = (uint32_t)first_bin;
        int rc = amps_recc_create(&d_handle, &cfg);
        if (rc != 0) throw std::runtime_error(std::string("amps::recc_wideband: ") + amps_recc_strerror(rc));
        if (shift_hz != 0.0) {
            try { set_shift(shift_hz); } catch (...) { amps_recc_destroy(d_handle); throw; }
        }
        if (resample) {
            amps_recc_wideband_resample_cfg_t r = {};
            r.struct_size = sizeof(r); r.interp = (uint32_t)interp; r.decim = (uint32_t)decim_in; r.rate_hz = rate_hz;
            rc = amps_recc_set_wideband_resample(d_handle, &r);
            if (rc != 0) { amps_recc_destroy(d_handle); throw std::runtime_error(std::string("amps::recc_wideband: resample: ") + amps_recc_strerror(rc)); }
            d_resample = true;
        }
        message_port_register_out(pmt::mp("bursts"));
        message_port_register_out(pmt::mp("records"));
        if (d_power) message_port_register_out(pmt::mp("power"));
        if (d_seizures) message_port_register_out(pmt::mp("seizures"));
        if (d_early) message_port_register_out(pmt::mp("early"));
    }
    ~recc_wideband_impl() { amps_recc_destroy(d_handle); }

    void set_shift(double shift_hz)
    {
        int rc = amps_recc_set_wideband_shift(d_handle, shift_hz);
        if (rc != 0) throw std::runtime_error(std::string("amps::recc_wideband: shift: ") + amps_recc_strerror(rc));
    }

    void set_rccl(const std::string &id, int nranks, int rank, int root, int mode)
    {
        // (the blocks RCCL carries are fc32: amps_recc_push_wideband_dist has no integer form)
        if (d_format != AMPS_RECC_SAMPLES_FC32) throw std::runtime_error("amps::recc_wideband: set_rccl is not available on a block with 16-bit or 8-bit input; distribute an fc32 stream");
        // (... and at the bank's rate: the library answers the distributed push of a resampling handle with -ENOSYS)
        if (d_resample) throw std::runtime_error("amps::recc_wideband: set_rccl is not available on a block with a resampler (rate_hz); distribute a stream at the bank's rate");
        if (id.size() != AMPS_RECC_RCCL_ID_BYTES) throw std::runtime_error("amps::recc_wideband: the RCCL id is 128 bytes");
        if (mode != AMPS_RECC_DIST_BROADCAST && mode != AMPS_RECC_DIST_SCATTER_ALLGATHER) throw std::runtime_error("amps::recc_wideband: unknown distribution mode");
        int rc = amps_recc_rccl_init(d_handle, (const uint8_t *)id.data(), nranks, rank);
        if (rc != 0) throw std::runtime_error(std::string("amps::recc_wideband: rccl: ") + amps_recc_strerror(rc));
        d_bcast = true; d_root = root; d_rank = rank; d_mode = mode;
    }

    // one block through the seam (alone, or as this rank's part of one collective) + its records out on the ports; false = stop the flow graph
    bool push_and_publish(const void *in, size_t n)
    {
        int rc;
        size_t pushed = n;
        if (d_bcast) {
            // every rank in step, ONE collective per call; only the root's items are read (staged to the device by the library) and only
            // the root's n counts -- it travels in the header of the collective (the schedulers of the ranks' flow graphs do not agree on
            // noutput_items)
            const bool root = d_rank == d_root;
            rc = amps_recc_push_wideband_dist(d_handle, root ? (const float *)in : nullptr, root ? n : 0, AMPS_MEM_HOST, d_root, d_mode, &pushed);
            d_stream_samples += pushed;
        } else rc = amps_recc_push_wideband_as(d_handle, in, n, d_format, AMPS_MEM_HOST);
        if (rc == -ENODATA) { d_ended = true; return false; }   // the root's stream has ended: a clean WORK_DONE, the communicator is left alone
        if (rc != 0) { std::fprintf(stderr, "amps::recc_wideband: %s\n", amps_recc_strerror(rc)); return leave(); }
        if (d_seizures && !recc_publish_seizures(*this, "recc_wideband", d_handle)) return leave();
        if (d_early && !recc_publish_early(*this, "recc_wideband", d_handle)) return leave();
        if (!recc_drain_and_publish(*this, "recc_wideband", true, d_handle, d_recs.data(), d_bursts.data(), kMaxRecs, d_power ? d_pow.data() : nullptr,
                                    d_power ? d_nsnap.data() : nullptr)) return leave();
        return true;
    }
    // The flow graph has stopped (the ranks' sources end at different times).  The root tells the others -- one header
    // exchange, -ENODATA on every rank, no data collective; the others keep joining the root's collectives (and publishing their records)
    // until they see it, so the root's last blocks are not lost on ranks whose pacing source ended first.  A root that died instead
    // is what the bounded waits are for.
    bool stop() override
    {
        if (d_bcast && !d_ended) {
            if (d_rank == d_root) { (void)amps_recc_push_wideband_dist(d_handle, nullptr, 0, AMPS_MEM_HOST, d_root, d_mode, nullptr); d_ended = true; }
            else while (!d_ended && push_and_publish(nullptr, 0)) { }
        }
        return true;
    }
    // this rank stops: the others must not wait for it beyond their bound
    bool leave()
    {
        if (d_bcast) (void)amps_recc_rccl_abort(d_handle);
        return false;
    }

    int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &)
    {
        const char *in = (const char *)input_items[0];
        const size_t item = item_size(d_format);
        if (d_bcast && d_rank != d_root) {
            // A non-root rank: its items are pacing only.  The ranks stay in step by STREAM POSITION, not by call or item counts (which
            // the schedulers of different processes do not share): this rank joins collectives -- each of whatever size the root
            // announces in its header -- until the root's stream has covered the items its own pacing input has offered so far.
            d_paced_items += (unsigned long long)noutput_items;
            while (d_stream_samples < d_paced_items)
                if (!push_and_publish(nullptr, 0)) return WORK_DONE;
            consume_each(noutput_items);
            return 0;
        }
        int done = 0;
        while (done < noutput_items) {
            int n = noutput_items - done;
            if (n > kMaxPush) n = kMaxPush;
            if (!push_and_publish(in + item * (size_t)done, (size_t)n)) return WORK_DONE;
            done += n;
        }
        consume_each(noutput_items);
        return 0;
    }
};

recc_wideband::sptr recc_wideband::make(int n_channels, int first_bin, int slicer, int groups, int group, int decim, bool short_input, bool channel_power, int channels, int input_format, double shift_hz,
                                        double rate_hz, int interp, int decim_in, bool seizure_events, bool early_messages)
{
    return gnuradio::get_initial_sptr(new recc_wideband_impl(n_channels, first_bin, slicer, groups, group, decim, short_input, channel_power, channels, input_format, shift_hz, rate_hz, interp, decim_in, seizure_events, early_messages));
}

std::string recc_wideband::rccl_unique_id()
{
    std::string id(AMPS_RECC_RCCL_ID_BYTES, '\0');
    int rc = amps_recc_rccl_unique_id((uint8_t *)&id[0]);
    if (rc != 0) throw std::runtime_error(std::string("amps::recc_wideband: rccl: ") + amps_recc_strerror(rc));
    return id;
}

} // namespace amps
} // namespace gr
