// recc_ring_window.h -- the window arithmetic of the block rings (recc_block_ring.hip.h): which entries a ring holds, which of them a
// capture takes, and how a range of entries leaves a ring of `slots`.  Host arithmetic only, no HIP, so that the window rule
// include/amps_recc.h states can be compiled and run stand-alone (tests/ring_window_host.cc).
#pragma once
#include <algorithm>
#include <cstdint>
#include "amps_recc.h"

namespace amps {

// which entries exist and which belong to a capture.  One "entry width" does not say both: a snapshot AT sample position + span still
// counts, a block must END at or before it.
enum class PowerRule { SNAPSHOT, BLOCK };

struct PowerWindow { uint64_t lo, hi; };          // entries [lo, hi) are held, hi = one past the newest
struct PowerRange { uint64_t j0; uint32_t count; };   // entries j0 ... j0 + count - 1; count = 0: not (all) held

// the entries the ring holds once the stream is idle at n_done: snapshot j exists iff 256 j < n_done, block j iff 256 (j + 1) <= n_done;
// nothing from before the origin, and no more than `slots`
constexpr PowerWindow power_ring_window(PowerRule rule, uint32_t slots, uint64_t n_done, uint64_t origin)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    const uint64_t hi = rule == PowerRule::SNAPSHOT ? (n_done + S - 1) / S : n_done / S;
    uint64_t lo = std::max<uint64_t>((origin + S - 1) / S, hi > slots ? hi - slots : 0);
    if (lo > hi) lo = hi;                         // nothing yet: a stream that has not reached its first whole block (never a snapshot stream: origin <= n_done)
    return PowerWindow{ lo, hi };
}

// the entries inside a capture of `span` samples at `position`: the snapshots j with position <= 256 j <= position + span, the blocks
// wholly inside [position, position + span); count = 0 unless every one of them is inside the window
constexpr PowerRange power_ring_range(PowerRule rule, uint64_t position, uint32_t span, PowerWindow w)
{
    const uint64_t S = AMPS_RECC_POWER_STRIDE;
    const uint64_t j0 = (position + S - 1) / S, j1 = (position + span) / S;
    if (rule == PowerRule::SNAPSHOT) {            // snapshots [j0, j1]
        const bool held = j1 >= j0 && j0 >= w.lo && j1 < w.hi;
        return PowerRange{ j0, held ? (uint32_t)(j1 - j0 + 1) : 0u };
    }
    const bool held = j1 > j0 && j0 >= w.lo && j1 <= w.hi;   // blocks [j0, j1)
    return PowerRange{ j0, held ? (uint32_t)(j1 - j0) : 0u };
}

// a copy-out of the n entries from `first` on: all of them held (first = hi with n = 0 is the empty answer, not an error)
constexpr bool power_ring_holds(PowerWindow w, uint64_t first, uint64_t n) { return first >= w.lo && first <= w.hi && n <= w.hi - first; }

// entry j lies in slot j mod slots (a power of two), so n <= slots entries from `first` on are one run of n1 slots from slot s0, and
// where the range wraps a second run of n - n1 from slot 0
struct RingRuns { uint64_t s0, n1; };
constexpr RingRuns ring_runs(uint64_t first, uint64_t n, uint32_t slots)
{
    const uint64_t s0 = first & (slots - 1);
    return RingRuns{ s0, std::min<uint64_t>(n, slots - s0) };
}

// the rings are entry-major: n entries of `rows` rows each, an entry `width` floats, from snap[n][rows][width] to the caller's
// out[rows][out_ld][width]
inline void ring_transpose(const float *snap, uint64_t n, uint64_t rows, uint64_t width, float *out, uint64_t out_ld)
{
    for (uint64_t c = 0; c < rows; c++)
        for (uint64_t i = 0; i < n; i++)
            for (uint64_t k = 0; k < width; k++) out[(c * out_ld + i) * width + k] = snap[(i * rows + c) * width + k];
}

// the documented counts (include/amps_recc.h): a capture is AMPS_RECC_CAPTURE_SYMS symbols
namespace power_ring_check {
constexpr PowerWindow ALL{ 0, 1u << 20 };
constexpr uint32_t count(PowerRule r, uint64_t pos, uint32_t sps) { return power_ring_range(r, pos, (uint32_t)AMPS_RECC_CAPTURE_SYMS * sps, ALL).count; }
static_assert(count(PowerRule::SNAPSHOT, 512, 2) == 27 && count(PowerRule::SNAPSHOT, 513, 2) == 26, "snapshots at 2 samples per symbol");
static_assert(count(PowerRule::SNAPSHOT, 512, 3) == 40 && count(PowerRule::SNAPSHOT, 513, 3) == 39, "snapshots at 3 samples per symbol");
static_assert(count(PowerRule::BLOCK, 512, 10) == 131 && count(PowerRule::BLOCK, 513, 10) == 130, "blocks at 10 samples per symbol");
static_assert(count(PowerRule::BLOCK, 512, 12) == 158 && count(PowerRule::BLOCK, 513, 12) == 157, "blocks at 12 samples per symbol");
static_assert(power_ring_range(PowerRule::SNAPSHOT, 512, 6748, ALL).j0 == 2 && power_ring_range(PowerRule::BLOCK, 513, 33740, ALL).j0 == 3, "first entry");
} // namespace power_ring_check

} // namespace amps
