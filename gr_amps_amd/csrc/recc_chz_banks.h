// recc_chz_banks.h -- what a filter bank of the wideband seam IS, stated once: the table of the eight bank sizes, what follows from a
// row and a decimation, and the one verdict on a cfg's wideband fields (chz_resolve_cfg).  Host arithmetic only, no HIP, so that it
// can be compiled and run stand-alone (tests/chz_banks_host.cc).  Admission (amps_recc_create), the host state and the dispatch
// (recc_channelizer.hip.h) and the plan calls read this table; a new sample rate is a row here and a `case` in chz_bank_kernel_for.
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "amps_recc.h"

namespace amps {

// FUSED1024: chz12_kernel, the slicer fused behind the FFT (or the same kernel writing the channel-major block: the unfused form).
// NARROW, GRID10: chz_narrow_kernel and chz_grid10_kernel, the two-kernel form only -- the block goes through the IQ seam's streaming kernel.
enum class ChzFamily { FUSED1024, NARROW, GRID10 };

// what a family's banks can do beyond channelising
enum : uint32_t {
    CHZ_HAS_FUSED = 1u << 0,          // the fused form: slicer bits straight to the bit ring, launches of whole 64-frame words
    CHZ_HAS_GROUPS = 1u << 1,         // cfg.wideband_groups > 1 (the fused form's: a rank skips everybody else's bins)
    CHZ_HAS_CHANNEL_POWER = 1u << 2,  // AMPS_RECC_FLAG_CHANNEL_POWER: the snapshot kernel re-reads a fused launch's block and carry
    CHZ_HAS_RCCL = 1u << 3,           // one band over several GPUs (amps_recc_rccl_init)
    CHZ_HAS_SHIFT = 1u << 4,          // amps_recc_set_wideband_shift: the mixing twins
    CHZ_HAS_STREAM_RINGS = 1u << 5,   // AMPS_RECC_FLAG_STREAM_POWER / _STREAM_OFFSET / _STREAM_OFFSET_UNIT, filled by the IQ seam's streaming kernel
    CHZ_FEATURES_1024 = CHZ_HAS_FUSED | CHZ_HAS_GROUPS | CHZ_HAS_CHANNEL_POWER | CHZ_HAS_RCCL,
    CHZ_FEATURES_TWO_KERNEL = CHZ_HAS_SHIFT | CHZ_HAS_STREAM_RINGS,
};

constexpr int CHZ_PRE = 4;   // FUSED1024: frames of history the carry keeps beyond the filter's own L - D samples: what the exact half of a workgroup's pre-roll reaches back to

struct ChzBank {
    uint32_t M;              // branches = FFT size = cfg.wideband_channels
    ChzFamily family;
    uint32_t features;       // CHZ_HAS_*
    uint32_t bin_hz;         // width of a bin: fs = M bin_hz
    uint32_t stride;         // bins from one 30 kHz channel to the next
    uint32_t taps;           // per branch: the prototype has taps M coefficients
    uint32_t decim[2];       // the admissible input samples per frame, the library's default ratio first; 0: no second one
    uint32_t fr[2];          // frames per workgroup at decim[i] (held to chz_narrow_fr / chz_grid10_fr by static_assert, where the kernels
                             // take them from); 0 at FUSED1024, whose launches size their workgroups' runs themselves
    uint32_t default_decim;  // what cfg.wideband_decim = 0 selects; 0: the caller must state it

    constexpr bool has(uint32_t feature) const { return (features & feature) != 0; }
    constexpr uint32_t max_channels() const { return M / stride; }
    constexpr uint32_t sample_rate_hz() const { return M * bin_hz; }
    // index of D among the admissible decimations, -1: not one of them
    constexpr int decim_index(uint32_t D) const { return D == 0 ? -1 : D == decim[0] ? 0 : D == decim[1] ? 1 : -1; }
    // samples per Manchester symbol (20 kHz) of a channel's stream, fs / D: 3 at D = M / 2, 2 at D = 3 M / 4 and on the 10 kHz grid
    constexpr uint32_t samples_per_symbol(uint32_t D) const { return sample_rate_hz() / (D * 20000u); }
    // the prototype's -6 dB point: 40 ksps per channel leave the slicer two sampling phases per symbol instead of three, and the wider
    // pass band gives back, under a carrier offset, what the coarser timing costs (profiles/r06/decim768_cpu_gonogo.txt; oracle/channelizer.py: cutoff_for_decim)
    constexpr double cutoff_hz(uint32_t D) const { return samples_per_symbol(D) == 2 ? 15.0e3 : 13.0e3; }
    // samples of history the carry holds in front of a launch's frame 0: the filter's own L - D, and in the fused family the pre-roll's
    // CHZ_PRE frames (a workgroup of the other families stages its frames' whole history)
    constexpr uint32_t hist(uint32_t D) const { return taps * M - D + (family == ChzFamily::FUSED1024 ? CHZ_PRE * D : 0u); }
    constexpr size_t carry_cap(uint32_t D) const { return (size_t)hist(D) + 64u * D; }   // + leftover (< 64 frames)
    // frames after which the fold's roll (n0 mod M) repeats, M / gcd(M, D): 2 at D = M / 2, 4 at 3 M / 4 and M / 4.  A launch starts
    // where the stream position is a multiple of M, so it produces whole periods -- and the fused form whole words of the bit ring
    constexpr uint32_t period(uint32_t D) const { uint32_t a = M, b = D; while (b) { const uint32_t r = a % b; a = b; b = r; } return M / a; }
    constexpr uint32_t frame_mask(uint32_t D, bool fused) const { return fused ? ~63u : ~(period(D) - 1u); }
};

constexpr ChzBank CHZ_BANKS[] = {
    //  M    family                features                 bin_hz stride taps  decim          fr        default
    { 1024, ChzFamily::FUSED1024, CHZ_FEATURES_1024,       30000u, 1u, 8u, { 768u, 512u }, { 0u, 0u },   768u },
    {  512, ChzFamily::NARROW,    CHZ_FEATURES_TWO_KERNEL, 30000u, 1u, 8u, { 384u, 256u }, { 4u, 8u },   384u },
    {  256, ChzFamily::NARROW,    CHZ_FEATURES_TWO_KERNEL, 30000u, 1u, 8u, { 192u, 128u }, { 16u, 16u }, 192u },
    {  128, ChzFamily::NARROW,    CHZ_FEATURES_TWO_KERNEL, 30000u, 1u, 8u, {  96u,  64u }, { 32u, 32u },  96u },
    { 2500, ChzFamily::GRID10,    CHZ_FEATURES_TWO_KERNEL, 10000u, 3u, 3u, { 625u,   0u }, { 4u, 0u },     0u },
    { 2000, ChzFamily::GRID10,    CHZ_FEATURES_TWO_KERNEL, 10000u, 3u, 3u, { 500u,   0u }, { 4u, 0u },     0u },
    { 1000, ChzFamily::GRID10,    CHZ_FEATURES_TWO_KERNEL, 10000u, 3u, 3u, { 250u,   0u }, { 4u, 0u },     0u },
    {  500, ChzFamily::GRID10,    CHZ_FEATURES_TWO_KERNEL, 10000u, 3u, 3u, { 125u,   0u }, { 8u, 0u },     0u },
};

constexpr const ChzBank *chz_bank_of(uint32_t M)
{
    for (const ChzBank &b : CHZ_BANKS) if (b.M == M) return &b;
    return nullptr;
}

// bins and rows of a handle: row i = the i-th channel (in band order) of the band selection -- n channels from bin `first` on, a
// channel stride apart -- that belongs to the handle's group -- all of them without groups.  Returns the row count; the cfg is a
// resolved one (chz_resolve_cfg), or one whose channels, first bin and group that function is about to admit.
inline uint32_t chz_rows(const ChzBank &b, const amps_recc_cfg_t &cfg, std::vector<uint16_t> *bin2row, std::vector<uint32_t> *row2chan)
{
    const uint32_t W = 64u / (cfg.wideband_groups > 1 ? cfg.wideband_groups : 1u);
    if (bin2row) bin2row->assign(b.M, (uint16_t)0xffffu);
    if (row2chan) row2chan->clear();
    uint32_t rows = 0;
    for (uint32_t c = 0; c < cfg.n_channels; c++) {
        const uint32_t k = (cfg.wideband_first_channel + b.stride * c) % b.M;
        if ((k & 63u) / W != cfg.wideband_group) continue;
        if (bin2row) (*bin2row)[k] = (uint16_t)rows;
        if (row2chan) row2chan->push_back(c);
        rows++;
    }
    return rows;
}

// The verdict on everything in a cfg that depends on the bank: the wideband_* fields, samples_per_symbol and max_samples_per_push of a
// wideband handle, and the flags a bank has or lacks.  Fills the defaults into *out (decimation, samples per symbol, taps per branch;
// a handle without the seam keeps its fields), gives the handle's rows (its channels, or its group's share of them), and answers 0 or
// -EINVAL, in which case *out and *rows are as they were.  What is not about a bank (n_channels and max_bursts at least 1, the IQ
// seam's samples per symbol, the slicer flags, sync_tolerance) stays with amps_recc_create.
inline int chz_resolve_cfg(const amps_recc_cfg_t &in, amps_recc_cfg_t *out, uint32_t *rows)
{
    amps_recc_cfg_t c = in;
    const ChzBank *b = nullptr;
    uint32_t nrows = c.n_channels;
    if (c.wideband_channels) {
        if (!(b = chz_bank_of(c.wideband_channels))) return -EINVAL;
        if (c.wideband_decim == 0) c.wideband_decim = b->default_decim;
        if (b->decim_index(c.wideband_decim) < 0) return -EINVAL;
        // the bit-domain kernels behind a bank are built for exactly the rate it delivers; a prototype for exactly its taps per branch
        // (the register ring of chz12_kernel and chz_narrow_kernel's fold are laid out for eight, chz_grid10_kernel's for three)
        if (c.samples_per_symbol == 0) c.samples_per_symbol = b->samples_per_symbol(c.wideband_decim);
        if (c.wideband_taps_per_branch == 0) c.wideband_taps_per_branch = b->taps;
        if (c.samples_per_symbol != b->samples_per_symbol(c.wideband_decim) || c.wideband_taps_per_branch != b->taps || c.max_samples_per_push == 0) return -EINVAL;
        if (c.n_channels > b->max_channels() || c.wideband_first_channel >= b->M) return -EINVAL;
        const uint32_t G = c.wideband_groups > 1 ? c.wideband_groups : 1u;
        if ((G != 1 && G != 2 && G != 4 && G != 8) || c.wideband_group >= G) return -EINVAL;
        // a channel-group handle owns only its group's rows, and exists in the fused form only
        if (G > 1 && (!b->has(CHZ_HAS_GROUPS) || (c.flags & AMPS_RECC_FLAG_UNFUSED_WIDEBAND))) return -EINVAL;
        if ((nrows = chz_rows(*b, c, nullptr, nullptr)) < 1) return -EINVAL;
    }
    // received power behind the filter bank exists where the fused form runs
    if ((c.flags & AMPS_RECC_FLAG_CHANNEL_POWER) && (!b || !b->has(CHZ_HAS_CHANNEL_POWER) || (c.flags & AMPS_RECC_FLAG_UNFUSED_WIDEBAND))) return -EINVAL;
    // on the IQ and translate seams the channel-rate stream itself is read once more, for its power and for the carrier offset: flags
    // of their own, for handles with the IQ seam and no fused bank (a two-kernel bank's block goes through the IQ seam's streaming
    // kernel, which fills the rings there too)
    if ((c.flags & (AMPS_RECC_FLAG_STREAM_POWER | AMPS_RECC_FLAG_STREAM_OFFSET | AMPS_RECC_FLAG_STREAM_OFFSET_UNIT)) &&
        ((b && !b->has(CHZ_HAS_STREAM_RINGS)) || c.max_samples_per_push == 0 || (c.flags & AMPS_RECC_FLAG_CHANNEL_POWER))) return -EINVAL;
    *out = c;
    *rows = nrows;
    return 0;
}

} // namespace amps
