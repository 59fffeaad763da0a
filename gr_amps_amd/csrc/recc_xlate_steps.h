// recc_xlate_steps.h -- the translate stage's per-channel phase steps from its centres: host arithmetic only, no HIP, so that the
// argument checks of amps_recc_set_xlate* and amps_recc_retune_xlate can be compiled and run stand-alone (tests/xlate_steps_host.cc).
#pragma once
#include <cerrno>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace amps {

// steps[c] = center_hz[c] / rate_hz as a 0.64 fixed-point fraction of a turn per input sample, two's complement for negative offsets.
// -EINVAL, with steps untouched, for no centres, rate_hz not positive, or a centre beyond +-rate_hz (a NaN included).
inline int xlate_steps_from(double rate_hz, const double *center_hz, size_t n, uint64_t *steps)
{
    if (n == 0 || !center_hz || !steps || !(rate_hz > 0.0)) return -EINVAL;
    for (size_t c = 0; c < n; c++)
        if (!(std::fabs(center_hz[c]) <= rate_hz)) return -EINVAL;
    for (size_t c = 0; c < n; c++) {
        const long double f = (long double)center_hz[c] / (long double)rate_hz;
        const long double fr = f - std::floor(f);
        steps[c] = (uint64_t)(fr * 18446744073709551616.0L);
    }
    return 0;
}

// amps_recc_retune_xlate's arguments against the configured form: `configured` centres (n_channels, or 1 for the per-row form, whose
// rows share one centre); the steps of all C rows into steps[C].  -EINVAL and steps untouched where the call is refused.
inline int xlate_retune_steps(bool shared, uint32_t C, double rate_hz, const double *center_hz, size_t n, uint64_t *steps)
{
    const size_t configured = shared ? C : 1;
    if (!center_hz || n != configured || C == 0) return -EINVAL;
    if (shared) return xlate_steps_from(rate_hz, center_hz, C, steps);
    uint64_t one = 0;
    if (int rc = xlate_steps_from(rate_hz, center_hz, 1, &one)) return rc;
    for (uint32_t c = 0; c < C; c++) steps[c] = one;
    return 0;
}

} // namespace amps
