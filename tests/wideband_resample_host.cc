// Stand-alone host program (no HIP, no Python): what the wideband seam's resampler admits (gr_amps_amd/csrc/recc_wideband_resample.h,
// wbr_admit and wbr_limits).  tests/test_cpu_wideband_resample.py compiles it with -fsanitize=address,undefined, runs it and compares
// what it prints with the rule written out in Python.
//   one line per (bank, L, M, rate, width, cutoff) of the sweep, in the order of the loops below: the verdict, and the filter as
//   admitted (zeros behind -EINVAL)
#include <cstdio>
#include <cstring>
#include <limits>
#include "recc_wideband_resample.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main()
{
    using namespace amps;
    static char buf[1 << 20];
    std::setvbuf(stdout, buf, _IOFBF, sizeof(buf));

    const double widths[] = { 0.0, 5.61e3, 40e3, 1e9 };
    const double cutoffs[] = { 0.0, 1e6, 1e9 };
    for (const ChzBank &b : CHZ_BANKS)
        for (uint32_t L = 0; L <= 9; L++)
            for (uint32_t M = 0; M <= 9; M++) {
                // the rate that L / M brings to the bank's exactly, one just inside the tolerance and one outside, and a fixed one
                const double exact = L ? (double)b.sample_rate_hz() * M / L : 0.0;
                const double rates[] = { exact, exact * (1.0 + 5e-7), exact * (1.0 + 3e-6), 4e6 };
                for (double rate : rates)
                    for (double width : widths)
                        for (double cutoff : cutoffs) {
                            WbrFilter f;
                            const int rc = wbr_admit(b, L, M, rate, cutoff, width, &f);
                            CHECK(rc == 0 || rc == -EINVAL || rc == -E2BIG);
                            if (rc == -EINVAL) CHECK(f.ng == 0 && f.ntp == 0);          // a refusal leaves *f alone
                            if (rc == 0) CHECK(f.ntp % 8 == 0 && f.ntp >= f.npp && f.ntp <= WBR_MAX_TAPS && wbr_lds_bytes(L, M, f.ntp, WBR_TILE) <= WBR_LDS_BYTES);
                            std::printf("%u %u %u %.17g %.17g %.17g : %d %u %u %u %.17g %.17g %.17g\n", b.M, L, M, rate, width, cutoff, rc, f.ng, f.npp, f.ntp,
                                        f.cutoff_hz, f.width_hz, f.usable_hz);
                        }
            }

    // numbers that are none
    {
        const ChzBank &b = *chz_bank_of(500);
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        WbrFilter f;
        for (double bad : { nan, inf, -inf, -1.0 }) {
            CHECK(wbr_admit(b, 5, 4, bad, 0.0, 0.0, &f) == -EINVAL);
            CHECK(wbr_admit(b, 5, 4, 4e6, bad, 0.0, &f) == -EINVAL);
            CHECK(wbr_admit(b, 5, 4, 4e6, 0.0, bad, &f) == -EINVAL);
        }
        CHECK(wbr_admit(b, 5, 4, 0.0, 0.0, 0.0, &f) == -EINVAL && f.ng == 0);
    }
    // the kernel's limits on their own: sizes the admission never produces
    CHECK(wbr_limits(5, 4, 56, WBR_TILE) == 0 && wbr_limits(5, 4, 520, WBR_TILE) == -E2BIG && wbr_limits(5, 4, 60, WBR_TILE) == -EINVAL);
    CHECK(wbr_limits(1, 2, 512, 4096) == -E2BIG && wbr_limits(1, 2, 512, 2048) == 0);      // 4 x 512 + 8 x (8192 + 512) = 71 680 bytes
    CHECK(wbr_limits(5, 4, 56, 1000) == -EINVAL && wbr_limits(5, 4, 56, 0) == -EINVAL);
    CHECK(wbr_window(5, 4, 56, 1024) == 820 + 56 && wbr_window(1, 2, 112, 1024) == 2048 + 112);
    // outputs delivered: ceil(L n / M), beyond 2^32 inputs too
    CHECK(wbr_outputs(5, 4, 0) == 0 && wbr_outputs(5, 4, 1) == 2 && wbr_outputs(5, 4, 4) == 5 && wbr_outputs(1, 2, 3) == 2);
    CHECK(wbr_outputs(8, 5, (1ull << 40) + 1) == ((8ull << 40) + 8 + 4) / 5);
    std::printf("wideband resample ok\n");
    return 0;
}
