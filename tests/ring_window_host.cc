// Stand-alone host program (no HIP, no Python): the window arithmetic of the block rings (gr_amps_amd/csrc/recc_ring_window.h).
// tests/test_cpu_ring_window.py compiles it with -fsanitize=address,undefined, runs it and checks the table it prints against the
// Python restatements of the window rule; the fake rings below are sized exactly, so an index past either run of a copy-out is an
// error here.
#include <cstdio>
#include <vector>
#include "recc_ring_window.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

using namespace amps;

// v right-aligned in `width` characters and a separator behind it: every line of the table has the same length
static char *put(char *p, uint64_t v, int width, char sep)
{
    for (int i = width - 1; i >= 0; i--, v /= 10) p[i] = (v || i == width - 1) ? (char)('0' + v % 10) : ' ';
    p[width] = sep;
    return p + width + 1;
}

// (a) one line per case: "rule slots origin n_done position sps   lo hi   j0 count"
static void table()
{
    const PowerRule rules[2] = { PowerRule::SNAPSHOT, PowerRule::BLOCK };
    const uint32_t all_slots[2] = { 8, 64 }, all_sps[3] = { 2, 3, 10 };
    const uint64_t origins[4] = { 0, 64, 960, 1024 };
    char line[64];
    for (PowerRule rule : rules)
        for (uint32_t slots : all_slots)
            for (uint64_t origin : origins)
                for (uint64_t n_done = origin; n_done <= origin + 3 * 256 * slots + 320; n_done += 64) {
                    const PowerWindow w = power_ring_window(rule, slots, n_done, origin);
                    for (uint64_t position = (origin + 36) / 37 * 37; position <= n_done; position += 37)
                        for (uint32_t sps : all_sps) {
                            const PowerRange r = power_ring_range(rule, position, (uint32_t)AMPS_RECC_CAPTURE_SYMS * sps, w);
                            char *p = line;
                            *p++ = rule == PowerRule::SNAPSHOT ? 'S' : 'B';
                            *p++ = ' ';
                            p = put(p, slots, 2, ' '); p = put(p, origin, 4, ' '); p = put(p, n_done, 5, ' '); p = put(p, position, 5, ' ');
                            p = put(p, sps, 2, ' '); p = put(p, w.lo, 3, ' '); p = put(p, w.hi, 3, ' '); p = put(p, r.j0, 3, ' ');
                            p = put(p, r.count, 3, '\n');
                            std::fwrite(line, 1, (size_t)(p - line), stdout);
                        }
                }
}

// the value of component k of entry j of row c
static float entry(uint64_t j, uint64_t c, uint64_t k) { return (float)(j * 8 + c * 2 + k); }

// (b) block_ring_channels with the device copies as host copies: the n entries from `first` on out of a ring that holds [hi - slots, hi),
// every element checked.  0: fine; else the line that failed
static int copy_out(uint32_t slots, uint64_t C, uint64_t W, uint64_t hi, uint64_t first, uint64_t n, uint64_t pad)
{
    const uint64_t ew = C * W;
    std::vector<float> ring(slots * ew);                          // exactly slots * C entries
    for (uint64_t j = hi - slots; j < hi; j++)
        for (uint64_t c = 0; c < C; c++)
            for (uint64_t k = 0; k < W; k++) ring[((j & (slots - 1)) * C + c) * W + k] = entry(j, c, k);
    const RingRuns r = ring_runs(first, n, slots);
    if (r.n1 > n || r.s0 + r.n1 > slots || n - r.n1 > r.s0) return __LINE__;   // the runs lie inside the ring and do not overlap
    std::vector<float> snap(n * ew);
    std::copy(ring.begin() + r.s0 * ew, ring.begin() + (r.s0 + r.n1) * ew, snap.begin());
    if (n > r.n1) std::copy(ring.begin(), ring.begin() + (n - r.n1) * ew, snap.begin() + r.n1 * ew);
    const uint64_t out_ld = n + pad;
    std::vector<float> out(C * out_ld * W, -1.f);
    ring_transpose(snap.data(), n, C, W, out.data(), out_ld);
    for (uint64_t c = 0; c < C; c++)
        for (uint64_t i = 0; i < out_ld; i++)
            for (uint64_t k = 0; k < W; k++)
                if (out[(c * out_ld + i) * W + k] != (i < n ? entry(first + i, c, k) : -1.f)) return __LINE__;
    return 0;
}

int main()
{
    static char buf[1 << 20];
    std::setvbuf(stdout, buf, _IOFBF, sizeof(buf));
    table();

    uint64_t straight = 0, wrapped = 0, whole = 0;
    const uint32_t all_slots[2] = { 8, 64 };
    for (uint32_t slots : all_slots)
        for (uint64_t C = 1; C <= 3; C += 2)
            for (uint64_t W = 1; W <= 2; W++)
                for (uint64_t turn = 0; turn < 3; turn++) {
                    const uint64_t hi = turn == 0 ? slots : turn == 1 ? slots + 5 : 3 * slots + 1;
                    // the window of a block stream idle at 256 hi + 100 that began at 0: the last `slots` entries
                    const PowerWindow w = power_ring_window(PowerRule::BLOCK, slots, 256 * hi + 100, 0);
                    CHECK(w.hi == hi && w.lo == hi - slots);
                    CHECK(power_ring_holds(w, w.hi, 0) && !power_ring_holds(w, w.hi, 1) && !power_ring_holds(w, w.hi + 1, 0));
                    CHECK(w.lo == 0 || !power_ring_holds(w, w.lo - 1, 1));
                    for (uint64_t first = w.lo; first <= w.hi; first++)
                        for (uint64_t n = 1; n <= w.hi - first; n++) {
                            CHECK(power_ring_holds(w, first, n) && !power_ring_holds(w, first, w.hi - first + 1));
                            CHECK(copy_out(slots, C, W, hi, first, n, n % 3) == 0);
                            if (n == slots) whole++;
                            else if ((first & (slots - 1)) + n > slots) wrapped++;
                            else straight++;
                        }
                }
    CHECK(straight > 0 && wrapped > 0 && whole > 0);
    std::printf("copy-outs: %llu straight, %llu wrapped, %llu whole rings\n", (unsigned long long)straight, (unsigned long long)wrapped,
                (unsigned long long)whole);
    std::puts("ring window ok");
    return 0;
}
