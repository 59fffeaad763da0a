// Stand-alone host program (no HIP, no Python): the argument checks and the step arithmetic behind amps_recc_set_wideband_shift and
// amps_recc_wideband_shift (gr_amps_amd/csrc/recc_wideband_shift.h; which bank has the shift: recc_chz_banks.h).  tests/test_cpu_wideband_shift.py compiles it with
// -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "recc_chz_banks.h"
#include "recc_wideband_shift.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main()
{
    using namespace amps;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const WidebandShift MARK{ 0x1234567890abcdefull, 4321.0 };
    const auto untouched = [&](const WidebandShift &w) { return w.step == MARK.step && w.hz == MARK.hz; };
    // what the library hands over in the first argument of a handle with the wideband seam: whether its bank's row has a mixing twin
    const auto has_shift = [](uint32_t M) { const ChzBank *b = chz_bank_of(M); return b && b->has(CHZ_HAS_SHIFT); };

    // every bank the call serves: fs = M x 30 kHz or M x 10 kHz
    const struct { uint32_t M; double bin; } banks[] = { { 512, 30e3 }, { 256, 30e3 }, { 128, 30e3 }, { 2500, 10e3 }, { 2000, 10e3 }, { 1000, 10e3 }, { 500, 10e3 } };
    for (const auto &b : banks) {
        const double fs = b.M * b.bin;
        CHECK(has_shift(b.M) && chz_bank_of(b.M)->bin_hz == b.bin);
        WidebandShift w = MARK;
        // refused: the handle's state is as it was
        CHECK(wideband_shift_from(true, b.M, b.bin, nan, &w) == -EINVAL && untouched(w));
        CHECK(wideband_shift_from(true, b.M, b.bin, inf, &w) == -EINVAL && untouched(w));
        CHECK(wideband_shift_from(true, b.M, b.bin, -inf, &w) == -EINVAL && untouched(w));
        CHECK(wideband_shift_from(true, b.M, b.bin, fs, &w) == -EINVAL && untouched(w));
        CHECK(wideband_shift_from(true, b.M, b.bin, std::nextafter(0.5 * fs, inf), &w) == -EINVAL && untouched(w));
        CHECK(wideband_shift_from(true, b.M, b.bin, -std::nextafter(0.5 * fs, inf), &w) == -EINVAL && untouched(w));
        CHECK(wideband_shift_from(false, b.M, b.bin, 1e3, &w) == -ENOSYS && untouched(w));     // no wideband seam
        CHECK(wideband_shift_from(false, b.M, b.bin, nan, &w) == -EINVAL && untouched(w));
        CHECK(wideband_shift_from(true, b.M, b.bin, 1e3, nullptr) == -EINVAL);
        // the arithmetic: a fraction of a turn in 0.64 fixed point, two's complement for a negative shift
        CHECK(wideband_shift_from(true, b.M, b.bin, 0.0, &w) == 0 && w.step == 0 && w.hz == 0.0);
        CHECK(wideband_shift_from(true, b.M, b.bin, -0.0, &w) == 0 && w.step == 0 && w.hz == 0.0);
        CHECK(wideband_shift_from(true, b.M, b.bin, 0.25 * fs, &w) == 0 && w.step == 1ull << 62 && w.hz == 0.25 * fs);
        CHECK(wideband_shift_from(true, b.M, b.bin, -0.25 * fs, &w) == 0 && w.step == 3ull << 62 && w.hz == -0.25 * fs);
        CHECK(wideband_shift_from(true, b.M, b.bin, 0.5 * fs, &w) == 0 && w.step == 1ull << 63 && w.hz == 0.5 * fs);
        CHECK(wideband_shift_from(true, b.M, b.bin, -0.5 * fs, &w) == 0 && w.step == 1ull << 63 && w.hz == -0.5 * fs);
        for (double hz : { 9000.0, 6543.21, 0.37, 1234567.0 / 3.0 }) {
            if (hz > 0.5 * fs) continue;
            WidebandShift p, n;
            CHECK(wideband_shift_from(true, b.M, b.bin, hz, &p) == 0 && wideband_shift_from(true, b.M, b.bin, -hz, &n) == 0);
            CHECK(p.step != 0 && (n.step >> 63) == 1 && (p.step + n.step == 0 || p.step + n.step == ~0ull));   // two's complement, to the last bit's rounding
            // read back within fs 2^-64 of what was set (and the double that says so within a rounding of it)
            const double tol = fs * 0x1p-64 + std::fabs(hz) * 0x1p-52;
            CHECK(std::fabs(p.hz - hz) <= tol && std::fabs(n.hz + hz) <= tol);
        }
    }
    // the 1024 bank has no mixing form: its row of the bank table lacks CHZ_HAS_SHIFT
    {
        WidebandShift w = MARK;
        CHECK(chz_bank_of(1024) && !has_shift(1024));
        CHECK(wideband_shift_from(has_shift(1024), 1024, 30e3, 1e3, &w) == -ENOSYS && untouched(w));
        CHECK(wideband_shift_from(has_shift(1024), 1024, 30e3, 0.0, &w) == -ENOSYS && untouched(w));
        CHECK(wideband_shift_from(has_shift(1024), 1024, 30e3, nan, &w) == -EINVAL && untouched(w));
    }
    std::puts("wideband shift ok");
    return 0;
}
