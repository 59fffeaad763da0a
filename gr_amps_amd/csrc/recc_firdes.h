// recc_firdes.h -- firdes.low_pass as the flow graph calls it: the one filter design behind the translate seams and the wideband
// seam's resampler.  Host arithmetic only, no HIP, so that the admission functions that ask for a filter's length can be compiled and
// run stand-alone (tests/wideband_resample_host.cc).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace amps {

// firdes.low_pass(gain, fs, cutoff, width, WIN_BLACKMAN) as the flow graph calls it (grc/recctest.grc:115-155):
// ntaps = int(74 fs / (22 width)) made odd; windowed sinc normalised to DC gain `gain`
inline int xlate_ntaps(double fs, double width)
{
    const double want = 74.0 * fs / (22.0 * width);
    int n = want < 1e9 ? (int)want : 1000000000;                 // far beyond every kernel's limit
    if (!(n & 1)) n++;
    return n;
}
inline std::vector<float> xlate_design_taps(double gain, double fs, double cutoff, double width)
{
    const int n = xlate_ntaps(fs, width);
    const int m = (n - 1) / 2;
    std::vector<double> t((size_t)n);
    const double w0 = 2.0 * M_PI * cutoff / fs;
    double sum = 0.0;
    for (int i = 0; i < n; i++) {
        const int k = i - m;
        const double win = 0.42 - 0.5 * std::cos(2.0 * M_PI * i / (n - 1)) + 0.08 * std::cos(4.0 * M_PI * i / (n - 1));
        t[(size_t)i] = (k == 0 ? w0 / M_PI : std::sin(k * w0) / (k * M_PI)) * win;
        sum += t[(size_t)i];
    }
    std::vector<float> out((size_t)n);
    for (int i = 0; i < n; i++) out[(size_t)i] = (float)(t[(size_t)i] * gain / sum);
    return out;
}

} // namespace amps
