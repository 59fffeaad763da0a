// recc_wideband_resample.h -- what the wideband seam's L / M resampler accepts, stated once: the limits of wb_resample_kernel and the
// verdict on a (bank, L, M, rate, cut-off, width).  Host arithmetic only, no HIP, so that it can be compiled and run stand-alone
// (tests/wideband_resample_host.cc).  amps_recc_set_wideband_resample and amps_recc_wideband_resample_plan both ask wbr_admit, and
// the kernel asks wbr_limits again at its top.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include "recc_chz_banks.h"
#include "recc_firdes.h"

#ifndef __host__
#define WBR_HD
#else
#define WBR_HD __host__ __device__
#endif

namespace amps {

constexpr uint32_t WBR_MAX_LM = 8;               // L and M: 1 ... 8
constexpr uint32_t WBR_MAX_TAPS = 512;           // padded taps PER PHASE
constexpr uint32_t WBR_THREADS = 256;
constexpr uint32_t WBR_TILE = 1024;              // outputs of a workgroup: four per thread
constexpr int64_t WBR_LDS_BYTES = 64 * 1024;     // the L tap sets, then the tile's input window as fc32

WBR_HD constexpr uint32_t wbr_gcd(uint32_t a, uint32_t b) { return b == 0 ? a : wbr_gcd(b, a % b); }
// input samples a tile of outputs can reach, its ntp - 1 samples of history included
WBR_HD constexpr uint32_t wbr_window(uint32_t L, uint32_t M, uint32_t ntp, uint32_t tile) { return (tile * M + L - 1) / L + ntp; }
WBR_HD constexpr int64_t wbr_lds_bytes(uint32_t L, uint32_t M, uint32_t ntp, uint32_t tile) { return (int64_t)4 * L * ntp + (int64_t)8 * wbr_window(L, M, ntp, tile); }
// The limits of the kernel: 0, -EINVAL (no such ratio, or no such launch) or -E2BIG (taps per phase, or tap sets + window beyond the
// LDS a workgroup may ask for without an attribute: with WBR_TILE outputs a tile the tap limit binds first, 36.6 KB at 1 / 2 x 8 phases).
WBR_HD constexpr int wbr_limits(uint32_t L, uint32_t M, uint32_t ntp, uint32_t tile)
{
    if (L < 1 || L > WBR_MAX_LM || M < 1 || M > WBR_MAX_LM || L == M || wbr_gcd(L, M) != 1) return -EINVAL;
    if (2 * L < M || L > 4 * M) return -EINVAL;                       // 1/2 <= L / M <= 4
    if (ntp < 8 || (ntp & 7) || tile < WBR_THREADS || tile % WBR_THREADS) return -EINVAL;
    if (ntp > WBR_MAX_TAPS || wbr_lds_bytes(L, M, ntp, tile) > WBR_LDS_BYTES) return -E2BIG;
    return 0;
}

// what wbr_admit works out: the filter with its defaults filled in, and its lengths
struct WbrFilter {
    double cutoff_hz = 0.0, width_hz = 0.0;
    double usable_hz = 0.0;      // 2 (f_low / 2 - width): the band the pass band keeps flat
    uint32_t ng = 0;             // the prototype's length at the up-sampled rate
    uint32_t npp = 0;            // taps per phase, ceil(ng / L)
    uint32_t ntp = 0;            // ... zero-padded to a multiple of 8
};

// A stream at rate_hz resampled by L / M in front of `bank`.  cutoff_hz / width_hz = 0: width = f_low / 16 and cutoff = f_low / 2 -
// width / 2, f_low the lower of the two rates, so that the stop band begins at f_low / 2.  In the order the configuration answers:
// -EINVAL for a ratio wbr_limits has not, numbers that are none, a rate that L / M does not bring to the bank's within 1e-6, a filter
// the design cannot make (fewer than three taps, a cut-off beyond L rate_hz / 2); -E2BIG for wbr_limits' sizes.  *f is written only
// where the answer is 0 or -E2BIG.
inline int wbr_admit(const ChzBank &bank, uint32_t L, uint32_t M, double rate_hz, double cutoff_hz, double width_hz, WbrFilter *f)
{
    if (wbr_limits(L, M, 8, WBR_TILE) == -EINVAL) return -EINVAL;
    if (!(rate_hz > 0.0) || std::isinf(rate_hz) || !std::isfinite(cutoff_hz) || !std::isfinite(width_hz) || cutoff_hz < 0.0 || width_hz < 0.0) return -EINVAL;
    const double bank_rate = (double)bank.sample_rate_hz();
    if (std::fabs(rate_hz * L / M - bank_rate) > 1e-6 * bank_rate) return -EINVAL;
    WbrFilter w;
    const double f_low = rate_hz < bank_rate ? rate_hz : bank_rate;
    w.width_hz = width_hz == 0.0 ? f_low / 16.0 : width_hz;
    w.cutoff_hz = cutoff_hz == 0.0 ? 0.5 * f_low - 0.5 * w.width_hz : cutoff_hz;
    w.usable_hz = 2.0 * (0.5 * f_low - w.width_hz);
    w.ng = (uint32_t)xlate_ntaps(L * rate_hz, w.width_hz);
    if (w.ng < 3 || !(w.cutoff_hz > 0.0) || !(w.cutoff_hz <= 0.5 * L * rate_hz)) return -EINVAL;
    w.npp = (w.ng + L - 1) / L;
    w.ntp = (w.npp + 7) / 8 * 8;
    *f = w;
    return w.ng > 1000000u ? -E2BIG : wbr_limits(L, M, w.ntp, WBR_TILE);
}

// outputs the stream has delivered after n inputs: the k with k M / L <= n - 1, ceil(L n / M)
inline uint64_t wbr_outputs(uint32_t L, uint32_t M, uint64_t n) { return (n * L + M - 1) / M; }

} // namespace amps
