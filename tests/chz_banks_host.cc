// Stand-alone host program (no HIP, no Python): the table of filter banks and the one verdict on a cfg's wideband fields
// (gr_amps_amd/csrc/recc_chz_banks.h).  tests/test_cpu_chz_banks.py compiles it with -fsanitize=address,undefined, runs it and compares
// what it prints with its own statement of the banks and of the admission rules.
//   "bank ..."  one line per row of the table
//   "geom ..."  one line per (row, admissible decimation): what follows from the two
//   then one line per cfg of the sweep, in the order of the loops below: verdict, and where it is 0 the resolved decimation, samples
//   per symbol, taps per branch and the handle's rows (zeros behind a refusal)
#include <cstdio>
#include <cstring>
#include <vector>
#include "recc_chz_banks.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main()
{
    using namespace amps;
    static char buf[1 << 20];
    std::setvbuf(stdout, buf, _IOFBF, sizeof(buf));

    for (const ChzBank &b : CHZ_BANKS) {
        CHECK(chz_bank_of(b.M) == &b);
        std::printf("bank %u family %d features %u bin_hz %u stride %u taps %u decim %u %u fr %u %u default %u max_channels %u rate %u\n", b.M, (int)b.family,
                    b.features, b.bin_hz, b.stride, b.taps, b.decim[0], b.decim[1], b.fr[0], b.fr[1], b.default_decim, b.max_channels(), b.sample_rate_hz());
        CHECK(b.decim_index(0) == -1 && b.decim_index(b.M) == -1 && b.decim_index(b.decim[0]) == 0);
        for (uint32_t D : b.decim)
            if (D) std::printf("geom %u %u sps %u cutoff %.0f hist %u carry_cap %zu period %u mask %u fused_mask %u\n", b.M, D, b.samples_per_symbol(D), b.cutoff_hz(D),
                               b.hist(D), b.carry_cap(D), b.period(D), ~b.frame_mask(D, false), ~b.frame_mask(D, true));
    }
    for (uint32_t M : { 0u, 64u, 127u, 129u, 300u, 2048u, 3000u }) CHECK(chz_bank_of(M) == nullptr);

    // a refusal leaves what it was given alone
    {
        amps_recc_cfg_t in, out;
        std::memset(&in, 0, sizeof(in));
        std::memset(&out, 0x5a, sizeof(out));
        const amps_recc_cfg_t mark = out;
        uint32_t rows = 12345;
        in.struct_size = sizeof(in); in.n_channels = 1; in.max_samples_per_push = 1024; in.wideband_channels = 300;
        CHECK(chz_resolve_cfg(in, &out, &rows) == -EINVAL && rows == 12345 && !std::memcmp(&out, &mark, sizeof(out)));
    }
    // chz_rows: the tables of a handle, wrapping past the last bin, one group of two
    {
        amps_recc_cfg_t c;
        std::memset(&c, 0, sizeof(c));
        c.n_channels = 100; c.wideband_first_channel = 1000; c.wideband_groups = 2; c.wideband_group = 1;
        std::vector<uint16_t> b2r;
        std::vector<uint32_t> r2c;
        const ChzBank &b = *chz_bank_of(1024);
        const uint32_t rows = chz_rows(b, c, &b2r, &r2c);
        CHECK(b2r.size() == 1024 && r2c.size() == rows && rows == chz_rows(b, c, nullptr, nullptr));
        uint32_t seen = 0;
        for (uint32_t k = 0; k < 1024; k++) {
            const bool in_band = (k + 1024 - 1000) % 1024 < 100, mine = in_band && (k & 63u) >= 32;
            CHECK((b2r[k] != 0xffffu) == mine);
            if (mine) { CHECK(b2r[k] < rows && (1000 + r2c[b2r[k]]) % 1024 == k); seen++; }
        }
        CHECK(seen == rows && rows == 56);   // of bins 1000 .. 1023, 0 .. 75: 1000 .. 1023 and 32 .. 63
    }

    const uint32_t channels[] = { 0, 64, 127, 128, 129, 256, 300, 500, 512, 1000, 1024, 2000, 2048, 2500, 3000 };
    const uint32_t flag_bits[] = { AMPS_RECC_FLAG_UNFUSED_WIDEBAND, AMPS_RECC_FLAG_CHANNEL_POWER, AMPS_RECC_FLAG_STREAM_POWER };
    unsigned long long n = 0, admitted = 0;
    for (uint32_t M : channels)
    for (uint32_t D : { 0u, M / 4, M / 4 + 1, M / 2, 3 * M / 4, M, 768u })
    for (uint32_t sps : { 0u, 2u, 3u, 10u })
    for (uint32_t taps : { 0u, 3u, 5u, 8u })
    for (uint32_t nch : { 1u, M / 3, M / 3 + 1, M, M + 1 })
    for (uint32_t first : { 0u, M - 1u, M })
    for (uint32_t groups : { 0u, 1u, 2u, 3u, 8u, 16u })
    for (uint32_t group : { 0u, 1u, groups })
    for (uint32_t max_samples : { 0u, 1024u })
    for (uint32_t f = 0; f < 8; f++) {
        amps_recc_cfg_t in, out;
        std::memset(&in, 0, sizeof(in));
        in.struct_size = sizeof(in); in.max_bursts = 1; in.device = -1;
        in.wideband_channels = M; in.wideband_decim = D; in.samples_per_symbol = sps; in.wideband_taps_per_branch = taps; in.n_channels = nch;
        in.wideband_first_channel = first; in.wideband_groups = groups; in.wideband_group = group; in.max_samples_per_push = max_samples;
        for (int i = 0; i < 3; i++) if (f >> i & 1) in.flags |= flag_bits[i];
        uint32_t rows = 0;
        const int rc = chz_resolve_cfg(in, &out, &rows);
        CHECK(rc == 0 || rc == -EINVAL);
        if (rc) std::fputs("-22    0  0 0    0\n", stdout);
        else {
            // nothing but the three defaults is filled in
            CHECK(out.struct_size == in.struct_size && out.n_channels == nch && out.max_samples_per_push == max_samples && out.max_bursts == 1 && out.device == -1 &&
                  out.flags == in.flags && out.wideband_channels == M && out.wideband_first_channel == first && out.sync_tolerance == 0 &&
                  out.wideband_groups == groups && out.wideband_group == group && out.stream == nullptr);
            CHECK((D == 0 || out.wideband_decim == D) && (sps == 0 || out.samples_per_symbol == sps) && (taps == 0 || out.wideband_taps_per_branch == taps));
            CHECK(out.wideband_decim < 10000 && out.samples_per_symbol < 100 && out.wideband_taps_per_branch < 10 && rows < 10000);
            std::printf("  0 %4u %2u %1u %4u\n", out.wideband_decim, out.samples_per_symbol, out.wideband_taps_per_branch, rows);
            admitted++;
        }
        n++;
    }
    std::printf("chz banks ok: %llu cfgs, %llu admitted\n", n, admitted);
    return 0;
}
