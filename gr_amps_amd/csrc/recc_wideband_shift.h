// recc_wideband_shift.h -- the argument checks and the step arithmetic behind amps_recc_set_wideband_shift / amps_recc_wideband_shift:
// host arithmetic only, no HIP, so that they can be compiled and run stand-alone (tests/wideband_shift_host.cc).
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include "recc_xlate_steps.h"

namespace amps {

// the shift of a bank's input: the mixer's step, and the frequency that step stands for
struct WidebandShift {
    uint64_t step = 0;       // shift_hz / fs as a 0.64 fixed-point fraction of a turn per wideband sample; 0: the unmixed kernels run
    double hz = 0.0;         // the shift in force, as quantised: within fs 2^-64 of what was asked
};

// The shift of a bank of M branches, bin_hz apart (fs = M bin_hz), from what the caller asks.  has_shift: the handle has the wideband
// seam and its bank a mixing twin (CHZ_HAS_SHIFT of recc_chz_banks.h: the fused bank has none).  -EINVAL for a NaN, -ENOSYS without
// has_shift, -EINVAL beyond +-fs / 2.  *out is written only where the call succeeds.
inline int wideband_shift_from(bool has_shift, uint32_t M, double bin_hz, double shift_hz, WidebandShift *out)
{
    if (!out || std::isnan(shift_hz)) return -EINVAL;
    if (!has_shift) return -ENOSYS;
    const double fs = (double)M * bin_hz;
    if (!(std::fabs(shift_hz) <= 0.5 * fs)) return -EINVAL;
    uint64_t step = 0;
    if (int rc = xlate_steps_from(fs, &shift_hz, 1, &step)) return rc;
    // the step read back as a frequency on the side of zero the caller asked for (- fs / 2 and + fs / 2 share a step)
    const long double turns = (long double)step * 0x1p-64L - (shift_hz < 0.0 && step ? 1.0L : 0.0L);
    out->step = step;
    out->hz = (double)(turns * (long double)fs);
    return 0;
}

} // namespace amps
