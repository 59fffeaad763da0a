// Stand-alone host program (no HIP, no Python): the argument checks and the step arithmetic behind amps_recc_set_xlate* and
// amps_recc_retune_xlate (gr_amps_amd/csrc/recc_xlate_steps.h).  tests/test_cpu_stream_offset_unit.py compiles it with
// -fsanitize=address,undefined and runs it; the vectors are sized exactly, so a write past the configured rows is an error here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "recc_xlate_steps.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main()
{
    using namespace amps;
    const double rate = 2.4e6, nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const uint64_t MARK = 0x1234567890abcdefull;

    // the arithmetic: a fraction of a turn in 0.64 fixed point, two's complement for negative centres
    {
        const double c[5] = { 0.0, 600e3, -600e3, 2.4e6, -2.4e6 };
        uint64_t s[5];
        CHECK(xlate_steps_from(rate, c, 5, s) == 0);
        CHECK(s[0] == 0 && s[1] == 1ull << 62 && s[2] == 3ull << 62 && s[3] == 0 && s[4] == 0);
        CHECK(s[1] + s[2] == 0);
    }
    // refused: untouched output
    {
        std::vector<uint64_t> s(3, MARK);
        const double bad_nan[3] = { 1e3, nan, 2e3 }, bad_far[3] = { 1e3, 2e3, 2.5e6 }, bad_inf[3] = { -inf, 0, 0 }, ok[3] = { 1e3, 2e3, 3e3 };
        CHECK(xlate_steps_from(rate, bad_nan, 3, s.data()) == -EINVAL);
        CHECK(xlate_steps_from(rate, bad_far, 3, s.data()) == -EINVAL);
        CHECK(xlate_steps_from(rate, bad_inf, 3, s.data()) == -EINVAL);
        CHECK(xlate_steps_from(0.0, ok, 3, s.data()) == -EINVAL);
        CHECK(xlate_steps_from(nan, ok, 3, s.data()) == -EINVAL);
        CHECK(xlate_steps_from(rate, nullptr, 3, s.data()) == -EINVAL);
        CHECK(xlate_steps_from(rate, ok, 0, s.data()) == -EINVAL);
        CHECK(xlate_steps_from(rate, ok, 3, nullptr) == -EINVAL);
        for (uint64_t v : s) CHECK(v == MARK);
    }
    // retune, shared and resampled forms: exactly C centres
    {
        const uint32_t C = 5;
        std::vector<double> c = { -1.05e6, 615e3, 15e3, 1.11e6, 0.0 };
        std::vector<uint64_t> s(C, MARK), ref(C);
        CHECK(xlate_retune_steps(true, C, rate, c.data(), C - 1, s.data()) == -EINVAL);
        CHECK(xlate_retune_steps(true, C, rate, c.data(), C + 1, s.data()) == -EINVAL);
        CHECK(xlate_retune_steps(true, C, rate, c.data(), 1, s.data()) == -EINVAL);
        CHECK(xlate_retune_steps(true, C, rate, c.data(), 0, s.data()) == -EINVAL);
        CHECK(xlate_retune_steps(true, C, rate, nullptr, C, s.data()) == -EINVAL);
        c[3] = nan;
        CHECK(xlate_retune_steps(true, C, rate, c.data(), C, s.data()) == -EINVAL);
        for (uint64_t v : s) CHECK(v == MARK);
        c[3] = 1.11e6;
        CHECK(xlate_retune_steps(true, C, rate, c.data(), C, s.data()) == 0);
        CHECK(xlate_steps_from(rate, c.data(), C, ref.data()) == 0);   // what a configuration with these centres computes
        CHECK(s == ref);
    }
    // retune, per-row form: one centre for all rows
    {
        const uint32_t C = 4;
        const double one = 160e3, two[2] = { 160e3, 161e3 }, bad = -3e6;
        std::vector<uint64_t> s(C, MARK);
        uint64_t ref = 0;
        CHECK(xlate_retune_steps(false, C, 400e3, two, 2, s.data()) == -EINVAL);
        CHECK(xlate_retune_steps(false, C, 400e3, two, C, s.data()) == -EINVAL);
        CHECK(xlate_retune_steps(false, C, 400e3, &bad, 1, s.data()) == -EINVAL);
        CHECK(xlate_retune_steps(false, 0, 400e3, &one, 1, s.data()) == -EINVAL);
        for (uint64_t v : s) CHECK(v == MARK);
        CHECK(xlate_retune_steps(false, C, 400e3, &one, 1, s.data()) == 0);
        CHECK(xlate_steps_from(400e3, &one, 1, &ref) == 0);
        for (uint64_t v : s) CHECK(v == ref);
    }
    std::puts("xlate steps ok");
    return 0;
}
