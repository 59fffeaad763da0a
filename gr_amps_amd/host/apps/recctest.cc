// recctest.cc -- config 0 plumbing: the message part of grc/recctest.grc (connections :3238-3274)
// as a stand-alone program.  Modes:
//   recctest syms <file.u8>  [chunk]   u8 0/1 symbol file -> amps.recc -> amps.recc_decode
//   recctest iq   <file.fc32> [chunk]  200 ksps interleaved fc32 -> amps.recc_fused -> amps.recc_decode
//   recctest iqb  <file.fc32> [chunk]  the same through recc_fused's "bursts" port (the 3374-byte blob amps_recc publishes) instead of "records"
//   recctest bank <file.u8>  [chunk] [C]  C channels in ONE gr::amps::recc_bank block: channel c = the symbol file delayed by 37 c symbols;
//                                      every line is prefixed with the channel the burst came from
//   recctest wide <file.fc32> [chunk] [slicer] [decim]  one 30.72 Msps wideband capture -> gr::amps::recc_wideband (832 channels from bin 96); every
//                                      burst's lines are prefixed with its channel; decoded through the "bursts" port.  A file whose name ends
//                                      in .sc16 (or a sixth argument `sc16`) is read as interleaved 16-bit I/Q and goes through the block's
//                                      16-bit input; .sc8 / .cs8 (or `sc8`) is read as int8 pairs and .cu8 (or `cu8`) as offset-binary uint8
//                                      pairs, through the block's input format (what HackRF and RTL-SDR tools write; the silence behind a
//                                      .cu8 file is the codes 127 / 128 alternating).  An argument `power` behind those (the seventh, or the eighth behind `sc16`) makes the block
//                                      keep received power: every burst's lines are followed by `MSG power channel <c> <10 log10(mean power)> dB
//                                      n=<snapshots>`; without it the output is what it always was.  An argument `channels=<M>` anywhere behind
//                                      the file (M = 512, 256 or 128) reads the capture as a stream at M x 30 ksps -- 15.36, 7.68 or 3.84 Msps --
//                                      through the M-branch bank: all M bins from bin 0 (recc_wideband::make(M, 0, ..., channels = M)); M = 2500,
//                                      2000, 1000 or 500: a capture at M x 10 kHz (25, 20, 10, 5 Msps) through the bank of M branches of
//                                      10 kHz, the M / 3 channels on bins 0, 3, 6 ... at decim = M / 4, which recctest sets itself.  An argument
//                                      `shift=<hz>` anywhere behind the file, with channels=<M>, corrects a tuner that delivered everything <hz>
//                                      too high inside the bank (recc_wideband::make(..., shift_hz)); `resample=<rate_hz>:<L>/<M>` likewise reads a file at
//                                      rate_hz and resamples it by L / M into the bank (recc_wideband::make(..., rate_hz, interp, decim_in))
//   recctest widerank <file.fc32> <chunk> <idfile> <nranks> <rank> [mode]   ONE rank of the same band over `nranks` processes (2, 4 or 8; one per GPU of a
//                                      node): gr::amps::recc_wideband::make(832, 96, -1, nranks, rank) + set_rccl -- rank 0 owns the capture and the
//                                      library distributes it (mode 0 = ncclBroadcast, 1 = scatter + all-gather); the other ranks' items only pace
//                                      them (they may use any chunk).  The 128-byte communicator id travels through <idfile> (rank 0 writes it).
//                                      Each rank prints the bursts of ITS channel group; the union is what `recctest wide` prints
//   recctest raw  <file.fc32> [chunk] [center_hz] [cutoff_hz]   the flow graph's own capture format (grc/recctest.grc:591): 400 ksps fc32,
//                                      channel at center_hz (default +160 kHz, :889-937) -> channel filter + fused chain on the GPU;
//                                      cutoff_hz (default 0 = the flow graph's 10 kHz) widens the channel filter for mobiles off their carrier.
//                                      A last argument `power` makes the block keep received power: every burst's lines are followed by
//                                      `MSG power channel 0 <10 log10(mean power)> dB n=<blocks>`, as `wide ... power` prints them; a last
//                                      argument `offset` makes it measure the carrier offset: `MSG offset channel 0 <Hz> Hz n=<blocks>` behind
//                                      every burst's lines.  Both may be given, in either order; `offset unit` selects the unit-amplitude
//                                      statistic, which is right behind the default 10 kHz filter too.  Behind them `retune=<sample>:<hz>`
//                                      moves the centre by <hz> before the first chunk at or beyond input sample <sample> (recc_fused::retune)
//   recctest sub  <file.raw> <chunk> <rate_hz> <decim> <c0,c1,...>   one narrowband fc32 capture at rate_hz holding several channels -> gr::amps::recc_subband
//                 (<decim> may be L/M, e.g. 5/64 for a 2.048 Msps capture: the rational resampler)
//                                      (the channel filter per centre c0, c1, ... in Hz relative to the capture's centre, decimation `decim` -- 1, 2, 4,
//                                      5, 6, 8, 10, 12, 16 or 20, with rate_hz / decim = 200 ksps: 2.4 Msps / 12, 2.0 / 10, 3.2 / 16, 1.0 / 5 ... -- and 10
//                                      samples per symbol behind it; a refused rate is answered with the pairs that rate admits); prints for every record what `wide` prints: its channel (the index into the list), then
//                                      its lines, decoded through the "bursts" port.  The file's extension gives its sample format: .sc16 is
//                                      interleaved int16, .sc8 / .cs8 int8, .cu8 offset-binary uint8 (what USRP-class, HackRF and RTL-SDR tools
//                                      write), read as they are through the block's input format; anything else is fc32.  A last argument
//                                      `power` (behind the centres) adds `MSG power channel <c> <10 log10(mean power)> dB n=<blocks>` behind
//                                      every burst's lines, a last argument `offset` `MSG offset channel <c> <Hz> Hz n=<blocks>` (the burst's
//                                      carrier offset from its centre, amps_recc_burst_offset; `offset unit`: of the unit-amplitude
//                                      statistic); both may be given, in either order; behind them `retune=<sample>:<hz>` moves every centre
//                                      by <hz> before the first chunk at or beyond input sample <sample> (recc_subband::retune); without
//                                      them the output is what it always was
// raw, sub and wide: an argument `seizures` (raw, sub: among the last ones, in any order with `power` and `offset`; wide: anywhere behind
// the file) makes the block keep seizure events (make(..., seizure_events = true)): every event of the "seizures" port is printed as
// `MSG seizure channel <c> position <n_c> found_at <n> dcc <7 bits, or - where the event came without them> bad <pairs>`, in front of
// the lines of the records that the same push delivered -- and long before the lines of its own record.
// Likewise an argument `early` makes the block keep early messages (make(..., early_messages = true)): every message of the "early" port
// is printed as `MSG early channel <c> position <n_c> found_at <n> words <n_words> class <msg_class> min <MIN>`, in front of the lines of
// the records that the same push delivered -- 120 ms (two words) or 96 ms (three) before the lines of its own record.
// Every message published on recc_decode's output ports is printed as one text line, which is what
// tests/test_gpu_host_blocks.py compares with the oracle.
#include <amps/recc.h>
#include <amps/recc_decode.h>
#include <amps/recc_bank.h>
#include <amps/recc_fused.h>
#include <amps/recc_wideband.h>
#include <amps/recc_subband.h>
#include "amps_recc_seizure.h"
#include "amps_recc_early.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <thread>
#include <chrono>
#include <vector>

static std::string bits(const pmt::pmt_t &blob)
{
    std::string s;
    const uint8_t *p = (const uint8_t *)pmt::blob_data(blob);
    for (size_t i = 0; i < pmt::blob_length(blob); i++) s += p[i] ? '1' : '0';
    return s;
}

namespace {
struct sink : gr::block {   // prints what ampsbs.grc would route to focc / fvc / mutes / command_processor
    sink() : gr::block("sink", gr::io_signature::make(0, 0, 0), gr::io_signature::make(0, 0, 0))
    {
        const char *ports[] = { "focc_words", "fvc_words", "audio_mute", "fvc_mute", "command_out" };
        for (const char *p : ports) {
            message_port_register_in(pmt::mp(p));
            std::string name = p;
            set_msg_handler(pmt::mp(p), [name](pmt::pmt_t m) {
                if (name == "focc_words")
                    std::printf("MSG focc_words stream=%ld n=%ld w1=%s w2=%s\n", pmt::to_long(pmt::tuple_ref(m, 0)), pmt::to_long(pmt::tuple_ref(m, 1)),
                                bits(pmt::tuple_ref(m, 2)).c_str(), bits(pmt::tuple_ref(m, 3)).c_str());
                else if (name == "fvc_words")
                    std::printf("MSG fvc_words n=%ld w1=%s repeat=%llu\n", pmt::to_long(pmt::tuple_ref(m, 0)), bits(pmt::tuple_ref(m, 1)).c_str(),
                                (unsigned long long)pmt::to_uint64(pmt::tuple_ref(m, 2)));
                else if (name == "command_out") {
                    size_t n = 0;
                    const uint8_t *p = pmt::u8vector_elements(pmt::cdr(m), n);
                    std::printf("MSG command_out %.*s\n", (int)n, (const char *)p);
                } else
                    std::printf("MSG %s %d\n", name.c_str(), pmt::to_bool(m) ? 1 : 0);
            });
        }
    }
    int general_work(int n, gr_vector_int &, gr_vector_const_void_star &, gr_vector_void_star &) override { return n; }
};

// a message of a block's "power" port: pmt::cons(channel, blob{ float mean_power; uint32_t n_snaps; }) (amps/recc_wideband.h)
void print_power(const pmt::pmt_t &m)
{
    float p = 0.f;
    uint32_t n = 0;
    const uint8_t *b = (const uint8_t *)pmt::blob_data(pmt::cdr(m));
    std::memcpy(&p, b, 4);
    std::memcpy(&n, b + 4, 4);
    std::printf("MSG power channel %ld %.2f dB n=%u\n", pmt::to_long(pmt::car(m)), 10.0 * std::log10((double)p), (unsigned)n);
}
// a message of a block's "offset" port: pmt::cons(channel, blob{ float offset_hz; uint32_t n_blocks; }) (amps/recc_subband.h)
void print_offset(const pmt::pmt_t &m)
{
    float hz = 0.f;
    uint32_t n = 0;
    const uint8_t *b = (const uint8_t *)pmt::blob_data(pmt::cdr(m));
    std::memcpy(&hz, b, 4);
    std::memcpy(&n, b + 4, 4);
    std::printf("MSG offset channel %ld %.1f Hz n=%u\n", pmt::to_long(pmt::car(m)), (double)hz, (unsigned)n);
}
// a message of a block's "seizures" port: pmt::cons(channel, blob(amps_recc_seizure_t)) (include/amps_recc_seizure.h)
void print_seizure(const pmt::pmt_t &m)
{
    amps_recc_seizure_t e;
    std::memcpy(&e, pmt::blob_data(pmt::cdr(m)), sizeof(e));
    std::string dcc = "-";
    if (e.flags & AMPS_SEIZURE_FLAG_DCC_COMPLETE) { dcc.clear(); for (int j = 0; j < 7; j++) dcc += e.dcc[j] ? '1' : '0'; }
    std::printf("MSG seizure channel %ld position %llu found_at %llu dcc %s bad %u\n", pmt::to_long(pmt::car(m)), (unsigned long long)e.position,
                (unsigned long long)e.found_at, dcc.c_str(), (unsigned)e.dcc_bad);
}
// a message of a block's "early" port: pmt::cons(channel, blob(amps_recc_early_t)) (include/amps_recc_early.h)
void print_early(const pmt::pmt_t &m)
{
    amps_recc_early_t e;
    std::memcpy(&e, pmt::blob_data(pmt::cdr(m)), sizeof(e));
    std::printf("MSG early channel %ld position %llu found_at %llu words %u class %u min %.10s\n", pmt::to_long(pmt::car(m)), (unsigned long long)e.rec.position,
                (unsigned long long)e.found_at, (unsigned)e.n_words, (unsigned)e.rec.msg_class, e.rec.min);
}
struct power_sink : gr::block {   // the "power", "offset", "seizures" and "early" ports of a block whose other ports go to recc_decode directly
    power_sink() : gr::block("power_sink", gr::io_signature::make(0, 0, 0), gr::io_signature::make(0, 0, 0))
    {
        message_port_register_in(pmt::mp("seizures"));
        set_msg_handler(pmt::mp("seizures"), [](pmt::pmt_t m) { print_seizure(m); });
        message_port_register_in(pmt::mp("early"));
        set_msg_handler(pmt::mp("early"), [](pmt::pmt_t m) { print_early(m); });
        message_port_register_in(pmt::mp("power"));
        set_msg_handler(pmt::mp("power"), [](pmt::pmt_t m) { print_power(m); });
        message_port_register_in(pmt::mp("offset"));
        set_msg_handler(pmt::mp("offset"), [](pmt::pmt_t m) { print_offset(m); });
    }
    int general_work(int n, gr_vector_int &, gr_vector_const_void_star &, gr_vector_void_star &) override { return n; }
};
} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s syms|iq|iqb|raw|bank|wide|sub <file> [chunk] [center_hz | C | slicer | rate_hz decim c0,c1,...]\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    // sub and raw: a last argument `power` asks for received power (wide finds its own further down, behind its positional arguments)
    // and `offset` for the carrier offset; the two may come in either order
    // `offset unit` selects the unit-amplitude statistic (the one that is right behind the default channel filter).  Behind all of
    // them `retune=<sample>:<hz>` moves every centre by <hz> before the first chunk that begins at or beyond input sample <sample>
    bool power_last = false, offset_last = false, unit_last = false, seizures = false, early = false;
    long long retune_at = -1;
    double retune_hz = 0.0;
    if ((mode == "sub" || mode == "raw") && argc > 3 && std::strncmp(argv[argc - 1], "retune=", 7) == 0) {
        char *end = nullptr;
        retune_at = std::strtoll(argv[argc - 1] + 7, &end, 10);
        if (retune_at < 0 || *end != ':') { std::fprintf(stderr, "%s: retune=<sample>:<hz>\n", argv[argc - 1]); return 2; }
        retune_hz = std::atof(end + 1);
        argc--;
    }
    while ((mode == "sub" || mode == "raw") && argc > 3) {
        const std::string last = argv[argc - 1];
        if (last == "power" && !power_last) power_last = true;
        else if (last == "offset" && !offset_last) offset_last = true;
        else if (last == "seizures" && !seizures) seizures = true;
        else if (last == "early" && !early) early = true;
        else if (last == "unit" && !offset_last && argc > 4 && std::string(argv[argc - 2]) == "offset") { offset_last = unit_last = true; argc--; }
        else break;
        argc--;
    }
    // wide: `channels=<M>` anywhere behind the file selects a narrow bank; the positional arguments are what is left
    // and `shift=<hz>` the tuner correction of such a bank
    int wide_channels = 1024;
    double wide_shift = 0.0, wide_rate = 0.0;                   // resample=<rate_hz>:<L>/<M>: the file is at rate_hz, resampled by L / M into the bank
    int wide_interp = 1, wide_decim_in = 1;
    for (int i = 3; mode == "wide" && i < argc;) {
        if (std::strncmp(argv[i], "channels=", 9) == 0) wide_channels = std::atoi(argv[i] + 9);
        else if (std::strncmp(argv[i], "shift=", 6) == 0) wide_shift = std::atof(argv[i] + 6);
        else if (std::strcmp(argv[i], "seizures") == 0) seizures = true;
        else if (std::strcmp(argv[i], "early") == 0) early = true;
        else if (std::strncmp(argv[i], "resample=", 9) == 0) {
            if (std::sscanf(argv[i] + 9, "%lf:%d/%d", &wide_rate, &wide_interp, &wide_decim_in) != 3 || !(wide_rate > 0.0)) { std::fprintf(stderr, "resample=<rate_hz>:<L>/<M>\n"); return 2; }
        }
        else { i++; continue; }
        for (int j = i; j + 1 < argc; j++) argv[j] = argv[j + 1];
        argc--;
    }
    const int chunk = argc > 3 ? std::atoi(argv[3]) : 4096;
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) { std::perror(argv[2]); return 2; }
    std::vector<char> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    try {
        auto dec = gr::amps::recc_decode::make();
        auto snk = std::make_shared<sink>();
        for (const char *p : { "focc_words", "fvc_words", "audio_mute", "fvc_mute", "command_out" }) gr::msg_connect(dec, p, snk, p);
        gr_vector_void_star outs;
        if (mode == "bank") {
            const int C = argc > 4 ? std::atoi(argv[4]) : 8;
            auto src = gr::amps::recc_bank::make(C);
            // demultiplex: (channel, blob) -> print the channel, hand the blob to the one recc_decode
            struct demux : gr::block {
                std::shared_ptr<gr::basic_block> dec;
                demux() : gr::block("demux", gr::io_signature::make(0, 0, 0), gr::io_signature::make(0, 0, 0))
                {
                    message_port_register_in(pmt::mp("bursts"));
                    set_msg_handler(pmt::mp("bursts"), [this](pmt::pmt_t m) {
                        std::printf("MSG channel %ld\n", pmt::to_long(pmt::car(m)));
                        dec->dispatch("bursts", pmt::cdr(m));
                    });
                }
                int general_work(int n, gr_vector_int &, gr_vector_const_void_star &, gr_vector_void_star &) override { return n; }
            };
            auto dm = std::make_shared<demux>();
            dm->dec = dec;
            gr::msg_connect(src, "bursts", dm, "bursts");
            std::vector<std::vector<char>> chans((size_t)C);
            for (int c = 0; c < C; c++) {                       // channel c: 37 c idle symbols in front of the file
                chans[c].assign((size_t)37 * c, 0);
                chans[c].insert(chans[c].end(), data.begin(), data.end());
                chans[c].resize(data.size() + (size_t)37 * C, 0);
            }
            const size_t total = data.size() + (size_t)37 * C;
            for (size_t off = 0; off < total; off += (size_t)chunk) {
                int n = (int)std::min<size_t>((size_t)chunk, total - off);
                gr_vector_const_void_star ins;
                for (int c = 0; c < C; c++) ins.push_back(chans[c].data() + off);
                if (src->work(n, ins, outs) != 0) return 1;
            }
        } else if (mode == "wide" || mode == "widerank") {
            const bool ranks = mode == "widerank";
            if (ranks && argc < 7) { std::fprintf(stderr, "usage: %s widerank <file> <chunk> <idfile> <nranks> <rank> [mode]\n", argv[0]); return 2; }
            const int nranks = ranks ? std::atoi(argv[5]) : 0, rank = ranks ? std::atoi(argv[6]) : 0;
            const std::string path = argv[2];
            const size_t dot = path.rfind('.');
            const std::string ext = dot == std::string::npos ? "" : path.substr(dot), arg6 = argc > 6 ? argv[6] : "";
            const int format = ranks ? 0 : ext == ".sc16" || arg6 == "sc16" ? 1 : ext == ".sc8" || ext == ".cs8" || arg6 == "sc8" ? 2 : ext == ".cu8" || arg6 == "cu8" ? 3 : 0;   // AMPS_RECC_SAMPLES_*
            const size_t item = format == 0 ? 8 : format == 1 ? 4 : 2;   // bytes per wideband sample
            bool power = false;
            for (int i = 6; !ranks && i < argc && i < 9; i++) power = power || std::string(argv[i]) == "power";
            const bool grid10 = wide_channels == 2500 || wide_channels == 2000 || wide_channels == 1000 || wide_channels == 500;   // bins of 10 kHz
            auto src = ranks ? gr::amps::recc_wideband::make(832, 96, -1, nranks, rank)
                             : grid10 ? gr::amps::recc_wideband::make(wide_channels / 3, 0, argc > 4 ? std::atoi(argv[4]) : -1, 0, 0, wide_channels / 4, false, power, wide_channels, format, wide_shift, wide_rate, wide_interp, wide_decim_in, seizures, early)
                             : wide_channels != 1024 ? gr::amps::recc_wideband::make(wide_channels, 0, argc > 4 ? std::atoi(argv[4]) : -1, 0, 0, argc > 5 ? std::atoi(argv[5]) : 0, false, power, wide_channels, format, wide_shift, wide_rate, wide_interp, wide_decim_in, seizures, early)
                             : gr::amps::recc_wideband::make(832, 96, argc > 4 ? std::atoi(argv[4]) : -1, 0, 0, argc > 5 ? std::atoi(argv[5]) : 0, false, power, 1024, format, wide_shift, wide_rate, wide_interp, wide_decim_in, seizures, early);
            if (ranks) {
                // the control plane is the application's: here, a file
                std::string id;
                const std::string idfile = argv[4];
                if (rank == 0) {
                    id = gr::amps::recc_wideband::rccl_unique_id();
                    std::ofstream o(idfile + ".tmp", std::ios::binary);
                    o.write(id.data(), (std::streamsize)id.size());
                    o.close();
                    std::rename((idfile + ".tmp").c_str(), idfile.c_str());
                } else {
                    for (int tries = 0; tries < 12000 && id.size() != 128; tries++) {
                        std::ifstream i(idfile, std::ios::binary);
                        if (i) id.assign((std::istreambuf_iterator<char>(i)), std::istreambuf_iterator<char>());
                        if (id.size() != 128) std::this_thread::sleep_for(std::chrono::milliseconds(10));
                    }
                }
                src->set_rccl(id, nranks, rank, 0, argc > 7 ? std::atoi(argv[7]) : 0);
            }
            struct demux : gr::block {
                std::shared_ptr<gr::basic_block> dec;
                demux() : gr::block("demux", gr::io_signature::make(0, 0, 0), gr::io_signature::make(0, 0, 0))
                {
                    message_port_register_in(pmt::mp("bursts"));
                    set_msg_handler(pmt::mp("bursts"), [this](pmt::pmt_t m) {
                        std::printf("MSG channel %ld\n", pmt::to_long(pmt::car(m)));
                        dec->dispatch("bursts", pmt::cdr(m));
                    });
                    message_port_register_in(pmt::mp("power"));       // { float mean_power; uint32_t n_snaps; } (amps/recc_wideband.h)
                    set_msg_handler(pmt::mp("power"), [](pmt::pmt_t m) { print_power(m); });
                }
                int general_work(int n, gr_vector_int &, gr_vector_const_void_star &, gr_vector_void_star &) override { return n; }
            };
            auto dm = std::make_shared<demux>();
            dm->dec = dec;
            gr::msg_connect(src, "bursts", dm, "bursts");
            if (power) gr::msg_connect(src, "power", dm, "power");
            auto ss = std::make_shared<power_sink>();
            if (seizures) gr::msg_connect(src, "seizures", ss, "seizures");
            if (early) gr::msg_connect(src, "early", ss, "early");
            std::vector<char> tail((size_t)64 * 768 * item, 0);       // silence: flushes the frames the fused form holds back (64 frames of at most 768 samples)
            if (format == 3)                                          // cu8 has no zero: (127, 128), (128, 127), ... = -+0.5, half a step either side of it
                for (size_t i = 0; i < tail.size(); i++) tail[i] = (char)(127 + (((i >> 1) ^ i) & 1));
            data.resize(data.size() / item * item);
            data.insert(data.end(), tail.begin(), tail.end());
            const size_t ns = data.size() / item;
            for (size_t off = 0; off < ns; off += (size_t)chunk) {
                int n = (int)std::min<size_t>((size_t)chunk, ns - off);
                gr_vector_const_void_star ins = { data.data() + item * off };
                if (src->work(n, ins, outs) != 0) return 1;
            }
            src->stop();                                              // as the scheduler does: the root announces its end of stream, the others join until they see it
        } else if (mode == "sub") {
            if (argc < 7) { std::fprintf(stderr, "usage: %s sub <file.raw> <chunk> <rate_hz> <decim> <c0,c1,...>\n"
                                                "  decim: 1, 2, 4, 5, 6, 8, 10, 12, 16 or 20, rate_hz / decim = 200000 (10 samples per symbol);\n"
                                                "         or L/M, the rational resampler: 5/64 at 2048000 (8 samples per symbol), 2/25 at 2500000\n", argv[0]); return 2; }
            std::vector<double> centers;
            for (const char *p = argv[6]; *p;) {
                char *end = nullptr;
                centers.push_back(std::strtod(p, &end));
                if (end == p) { std::fprintf(stderr, "%s: bad list of centres\n", argv[6]); return 2; }
                p = *end == ',' ? end + 1 : end;
            }
            const std::string path = argv[2];
            const size_t dot = path.rfind('.');
            const std::string ext = dot == std::string::npos ? "" : path.substr(dot);
            const int format = ext == ".sc16" ? 1 : ext == ".sc8" || ext == ".cs8" ? 2 : ext == ".cu8" ? 3 : 0;   // AMPS_RECC_SAMPLES_*
            const size_t item = format == 0 ? 8 : format == 1 ? 4 : 2;   // bytes per sample
            // <decim> is D, or L/M for the rational resampler; the samples per symbol are what the rate then gives (10 at rate / D = 200 ksps)
            const char *slash = std::strchr(argv[5], '/');
            const int interp = slash ? std::atoi(argv[5]) : 1, decim = std::atoi(slash ? slash + 1 : argv[5]);
            const double rate = std::atof(argv[4]);
            const int sps = decim > 0 && interp > 0 ? (int)std::lround(rate * interp / decim / 20e3) : 10;
            auto src = gr::amps::recc_subband::make(rate, centers, decim, sps, -1, 0.0, 0.0, format, interp, power_last, offset_last, unit_last, seizures, early);
            struct demux : gr::block {
                std::shared_ptr<gr::basic_block> dec;
                demux() : gr::block("demux", gr::io_signature::make(0, 0, 0), gr::io_signature::make(0, 0, 0))
                {
                    message_port_register_in(pmt::mp("bursts"));
                    set_msg_handler(pmt::mp("bursts"), [this](pmt::pmt_t m) {
                        std::printf("MSG channel %ld\n", pmt::to_long(pmt::car(m)));
                        dec->dispatch("bursts", pmt::cdr(m));
                    });
                    message_port_register_in(pmt::mp("power"));
                    set_msg_handler(pmt::mp("power"), [](pmt::pmt_t m) { print_power(m); });
                    message_port_register_in(pmt::mp("offset"));
                    set_msg_handler(pmt::mp("offset"), [](pmt::pmt_t m) { print_offset(m); });
                }
                int general_work(int n, gr_vector_int &, gr_vector_const_void_star &, gr_vector_void_star &) override { return n; }
            };
            auto dm = std::make_shared<demux>();
            dm->dec = dec;
            gr::msg_connect(src, "bursts", dm, "bursts");
            if (power_last) gr::msg_connect(src, "power", dm, "power");
            if (offset_last) gr::msg_connect(src, "offset", dm, "offset");
            auto ss = std::make_shared<power_sink>();
            if (seizures) gr::msg_connect(src, "seizures", ss, "seizures");
            if (early) gr::msg_connect(src, "early", ss, "early");
            const size_t ns = data.size() / item;
            for (size_t off = 0; off < ns; off += (size_t)chunk) {
                int n = (int)std::min<size_t>((size_t)chunk, ns - off);
                if (retune_at >= 0 && off >= (size_t)retune_at) {
                    for (double &c : centers) c += retune_hz;
                    src->retune(centers);
                    retune_at = -1;
                }
                gr_vector_const_void_star ins = { data.data() + item * off };
                if (src->work(n, ins, outs) != 0) return 1;
            }
        } else if (mode == "syms") {
            auto src = gr::amps::recc::make();
            gr::msg_connect(src, "bursts", dec, "bursts");
            for (size_t off = 0; off < data.size(); off += (size_t)chunk) {
                int n = (int)std::min<size_t>((size_t)chunk, data.size() - off);
                gr_vector_const_void_star ins = { data.data() + off };
                if (src->work(n, ins, outs) != 0) return 1;
            }
        } else {
            const double center = argc > 4 ? std::atof(argv[4]) : 160e3;
            const double cutoff = argc > 5 ? std::atof(argv[5]) : 0.0;
            auto src = mode == "raw" ? gr::amps::recc_fused::make(10, 400e3, center, 2, cutoff, 0.0, power_last, offset_last, unit_last, seizures, early) : gr::amps::recc_fused::make(10);
            if (mode == "iqb") gr::msg_connect(src, "bursts", dec, "bursts"); else gr::msg_connect(src, "records", dec, "records");
            auto ps = std::make_shared<power_sink>();
            if (power_last) gr::msg_connect(src, "power", ps, "power");
            if (offset_last) gr::msg_connect(src, "offset", ps, "offset");
            if (seizures) gr::msg_connect(src, "seizures", ps, "seizures");
            if (early) gr::msg_connect(src, "early", ps, "early");
            const size_t ns = data.size() / 8;
            for (size_t off = 0; off < ns; off += (size_t)chunk) {
                int n = (int)std::min<size_t>((size_t)chunk, ns - off);
                if (retune_at >= 0 && off >= (size_t)retune_at) {
                    src->retune(center + retune_hz);
                    retune_at = -1;
                }
                gr_vector_const_void_star ins = { data.data() + 8 * off };
                if (src->work(n, ins, outs) != 0) return 1;
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
