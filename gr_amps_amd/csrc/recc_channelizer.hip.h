// recc_channelizer.hip.h -- polyphase channelizer front end for gfx950: one wideband fc32 stream
// (fs = M * 30 kHz) -> C active 30 kHz channels at fs / D, with the RECC slicer fused behind the FFT.
//
// It stands where the reference wires one freq_xlating_fir_filter_ccc (299 complex taps, decim 2) per
// channel in front of the RECC chain (grc/recctest.grc:889-937, taps :115-155).  Replicating that FIR per
// channel is ~150 flop per input byte; a weighted-overlap-add filter bank does all M
// channels at once for ~17 flop/B:
//     frame m:  n0 = (m+1) D - L,  L = P*M taps
//               u[r] = sum_{i : (n0+i) mod M = r} h[i] x[n0+i]          (fold, "polyphase")
//               Y_k[m] = FFT_M(u)[k] = sum_i h[i] x[n0+i] e^{-j 2 pi k (n0+i)/M}
// i.e. channel k (centre k*fs/M) mixed to DC with an absolute phase reference, low-pass filtered by the
// prototype h and decimated by D = M/2 (2x oversampled: 60 ksps = 3 samples per Manchester symbol at M = 1024).
//
// Mapping to the hardware: ONE 768-thread workgroup owns a CU and its twelve waves split three ROLES, four waves each, so
// that every SIMD holds one wave of each role -- a VALU-dense one, and two that alternate LDS round trips with VALU work in
// different phases (chz12_kernel below):
//   fold  : polyphase delay lines in a register ring, the fold as v_pk_fma chains, radix-4 pass 1 on its own registers
//   pass 2: radix 16, one frame per wave, in place in LDS
//   pass 3: radix 16 (FFT-1024 = 4 x 16 x 16), then the slicer: a lane owns the same four channels for ever
// Half-batches of four frames travel through a four-slot LDS ring (16 frame buffers, 136 KB), one workgroup barrier per four
// frames.  Only slicer bits (1/64 of the input) reach HBM.  No MFMA: the contraction per channel is 8 taps deep and differs per
// branch, and the FFT is a butterfly network (a DFT-16 as a matrix product costs 12x its flops at the f32 MFMA rate = the VALU rate).
//
// The parts, one concern per header: recc_chz_banks.h (the table of bank sizes and the verdict on a cfg's wideband fields, free of HIP),
// recc_chz_common.hip.h (constants, ChzArgs, sample types and their one list, packed fp32), recc_chz_fft.hip.h (the
// passes and LDS layouts), recc_chz_fold.hip.h (register ring, loaders, fold; D = 512 and D = 768), recc_chz_slicer.hip.h (the fused
// slicer), recc_chz12_body.hip.h (the kernel's body, as text).  This file: the kernels' entry points, the carry kernels and the host state.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <type_traits>
#include <vector>
#include "amps_recc.h"
#include "amps_recc_numerics.h"
#include "recc_devmem.hip.h"
#include "recc_timing.hip.h"      // TimelineBuf (CHZ_TIMELINE builds)
#include "recc_chz_common.hip.h"
#include "recc_chz_fft.hip.h"
#include "recc_chz_fold.hip.h"
#include "recc_chz_slicer.hip.h"
#include "recc_power.hip.h"       // chz_power_launch: the power snapshots behind a fused launch
#include "recc_chz_narrow.hip.h"  // the banks of 512, 256 and 128 branches: a kernel of their own behind the same state, carry and host code
#include "recc_wideband_shift.h"  // WidebandShift: the tuner correction of the banks below 1024 branches
#include "recc_chz_grid10.hip.h"  // the banks of 2500, 2000, 1000 and 500 branches of 10 kHz (25, 20, 10 and 5 Msps): likewise
#include "recc_wideband_resample.hip.h"   // WbResampleState: the L / M resampler in front of a bank, for the rates that are no bank's

namespace amps {

// ---- the three-role pipeline ----
// Round 2's kernel had two roles (4 fold waves, 8 FFT waves that also ran the slicer): the eight FFT waves moved in lock step
// -- all reading LDS, all computing, all writing -- so LDS bursts and VALU bursts alternated instead of overlapping, two FFT
// waves in the same phase shared every SIMD, and the slicer sat on their critical path behind a second barrier (VALU issue
// slots 0.57 busy, waves parked 39 % of their cycles).  Here a time step is FOUR frames and every SIMD holds three waves in
// three different phases:
//   "fold"  : thread t keeps branches t + 256 j as a register ring, folds the four frames of half-batch h and runs
//                         the radix-4 pass 1 (+ pass 2's input twiddles) on its own registers -> slot h & 3.  Pure VALU +
//                         prefetched global loads.
//   waves 4..7  "pass 2": wave w transforms frame w of half-batch h - 1 (radix 16, p = 4), in place.
//   waves 8..11 "pass 3": wave w first slices half-batch h - 3 (all four frames, four channels per lane, planar operands),
//                         then transforms frame w of half-batch h - 2 (radix 16, p = 64) into the planar layout.
// ONE workgroup barrier per four frames (round 2: two per eight, with the slicer between them).  A half-batch lives four time
// steps in a four-slot ring of 4 x 4 frame buffers = 136 KB of LDS; every role stays below 168 VGPRs: three waves per SIMD.
// The unfused form is the same kernel with a different epilogue (MODE = CHZ12_IQ: the bins leave as 32-byte runs of the
// channel-major block), so fused and unfused forms stay bit-identical by construction.

// Timeline hook (builds with -DCHZ_TIMELINE only; scripts/chz_timeline.py): every wave of workgroup 0 accumulates, in registers,
// the s_memtime spent between its phase boundaries over the time steps >= CHZ_TL_FIRST and writes the sums once, at the end
// (no memory traffic inside the loop: stores would count in the fold role's vmcnt window and stall it)
constexpr int CHZ_TL_FIRST = 40;
#ifdef CHZ_TIMELINE
#define CHZ_TL_DECL long long tl_acc[6] = {}, tl_last = 0
#define CHZ_STAMP(step, k) do { if ((step) >= CHZ_TL_FIRST) { const long long now_ = (long long)__builtin_amdgcn_s_memtime(); \
        if (tl_last) tl_acc[k] += now_ - tl_last; tl_last = now_; if ((k) == 4) tl_acc[5]++; } } while (0)
#define CHZ_TL_FLUSH do { if (a.tl && blockIdx.x == 0 && lane == 0) for (int k_ = 0; k_ < 6; k_++) a.tl[wave * 8 + k_] = (unsigned long long)tl_acc[k_]; } while (0)
constexpr size_t CHZ_TL_STAMPS = 12 * 8;                         // [wave][8]
inline TimelineBuf &chz_timeline() { static TimelineBuf &b = *new TimelineBuf(); return b; }   // kept for the life of the process
#else
#define CHZ_TL_DECL
#define CHZ_STAMP(step, k) do { } while (0)
#define CHZ_TL_FLUSH do { } while (0)
#endif

// carry_out[k] = virtual sample (consumed - hist + k), k in [0, hist + leftover_new)
template <typename T>
__device__ __forceinline__ float2 chz_carry_sample(const T *block, const float2 *carry_in, uint32_t carry_len, uint32_t nsamp,
                                                   uint32_t hist, uint32_t consumed, uint32_t k)
{
    const int64_t lead = (int64_t)carry_len - hist;
    const int64_t v = (int64_t)consumed - hist + k;   // launch-relative virtual index
    const int64_t ci = v + hist;
    float2 s = make_float2(0.f, 0.f);
    if (ci >= 0) {
        if (ci < (int64_t)carry_len) s = carry_in[ci];
        else {
            const int64_t bi = v - lead;
            if constexpr (chz_is_short<T>::value) { if (bi < (int64_t)nsamp) { const cf2 c = chz_cvt(block[bi]); s = make_float2(c.x, c.y); } }
            else { if (bi < (int64_t)nsamp) s = block[bi]; }
        }
    }
    return s;
}
// stand-alone form: a push too short to produce a frame only moves the carry
__global__ __launch_bounds__(256) void chz_carry_kernel(const float2 *block, const float2 *carry_in, float2 *carry_out,
                                                         uint32_t carry_len, uint32_t nsamp, uint32_t hist, uint32_t consumed,
                                                         uint32_t out_len)
{
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < out_len; k += gridDim.x * 256)
        carry_out[k] = chz_carry_sample(block, carry_in, carry_len, nsamp, hist, consumed, k);
}
// the same behind a push of 16-bit I/Q: the carry it leaves is fc32 like any other
__global__ __launch_bounds__(256) void chz_carry_short_kernel(const chz_sc16 *block, const float2 *carry_in, float2 *carry_out,
                                                               uint32_t carry_len, uint32_t nsamp, uint32_t hist, uint32_t consumed,
                                                               uint32_t out_len)
{
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < out_len; k += gridDim.x * 256)
        carry_out[k] = chz_carry_sample(block, carry_in, carry_len, nsamp, hist, consumed, k);
}
// ... and behind a push of 8-bit I/Q (T = xl_sc8 or xl_cu8: amps_recc_push_wideband_as)
template <typename T>
__global__ __launch_bounds__(256) void chz_carry_b8_kernel(const T *block, const float2 *carry_in, float2 *carry_out,
                                                            uint32_t carry_len, uint32_t nsamp, uint32_t hist, uint32_t consumed,
                                                            uint32_t out_len)
{
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < out_len; k += gridDim.x * 256)
        carry_out[k] = chz_carry_sample(block, carry_in, carry_len, nsamp, hist, consumed, k);
}
// sc16 -> fc32, a sample per thread: in front of the fc32 filter bank where the checking modes (unfused form, amps_recc_debug_channelize)
// and the AMPS_RECC_SHORT_PREPASS experiment take a 16-bit block
__global__ __launch_bounds__(256) void chz_short_to_float_kernel(const chz_sc16 *in, float2 *out, uint32_t n)
{
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) { const cf2 c = chz_cvt(in[k]); out[k] = make_float2(c.x, c.y); }
}
// sc8 / cu8 -> fc32 likewise: in front of the 1024 bank always (no radio delivers 8 bits at 30.72 Msps; converted capture files do),
// so that every form of that bank -- fused or not, channel groups, the power ring -- runs as on an fc32 block
template <typename T>
__global__ __launch_bounds__(256) void chz_b8_to_float_kernel(const T *in, float2 *out, uint32_t n)
{
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) { const cf2 c = chz_cvt(in[k]); out[k] = make_float2(c.x, c.y); }
}

// The kernel's body is recc_chz12_body.hip.h, once per sample type of the block (see there for why it is text, not a function).
template <int P, int MODE, int DEC = CHZ_D>
__global__ __launch_bounds__(768, 3) void chz12_kernel(ChzArgs a)
{
    using T = float2;
#define CHZ12_BODY_SHORT 0
#include "recc_chz12_body.hip.h"
#undef CHZ12_BODY_SHORT
}
// the fused filter bank on a block of 16-bit I/Q, read in place (a.block points at chz_sc16): 4 bytes per sample from HBM
template <int P, int MODE, int DEC = CHZ_D>
__global__ __launch_bounds__(768, 3) void chz12_short_kernel(ChzArgs a)
{
    using T = chz_sc16;
#define CHZ12_BODY_SHORT 1
#include "recc_chz12_body.hip.h"
#undef CHZ12_BODY_SHORT
}

struct ChannelizerState {
    bool enabled = false;
    const ChzBank *bank = nullptr;  // the row of recc_chz_banks.h this handle runs: branches, family (which kernel), bin width, taps per branch, features
    uint32_t D = CHZ_D;             // input samples per frame: one of the bank's decimations
    bool has(uint32_t feature) const { return enabled && bank->has(feature); }   // CHZ_HAS_*: false without the seam
    uint32_t C = 0;                 // rows this handle decodes (= the band's channels, or one group of them)
    uint32_t groups = 1, group = 0; // cfg.wideband_groups / wideband_group
    DevBuf<uint16_t> bin2row;       // device [M]
    std::vector<uint32_t> row2chan; // row -> channel number within the band selection (what the records carry)
    uint32_t max_frames = 0;        // per push
    uint32_t target_wgs = 256;      // resident workgroups of the filter-bank kernel (one 768-thread workgroup per CU)
    DevBuf<float> taps;             // [L]
    DevBuf<float2> twiddle;         // the two-kernel families: [M], e^{-2 pi i k / M}
    DevBuf<float2> carry[2];
    int carry_cur = 0;
    uint32_t carry_len = 0;         // L - D + leftover
    uint64_t frames_done = 0;
    WidebandShift shift;            // amps_recc_set_wideband_shift (CHZ_HAS_SHIFT): a non-zero step launches the mixing twins.  Kept over a reset
    DevBuf<float2> out;             // [C][ld]
    uint64_t ld = 0;
    HostStage stage;                // host-resident wideband input as the caller's samples (fc32, sc16, sc8 or cu8), sized in bytes: the largest block so far
    DevBuf<float2> cvt;             // an integer block expanded to fc32, the fused family only: sc16 in the checking modes and the pre-pass experiment, sc8 / cu8 always
    bool short_prepass = false;     // AMPS_RECC_SHORT_PREPASS=1 at create: sc16 blocks go through chz_short_to_float_kernel + the fc32 kernel
    WbResampleState rs;             // amps_recc_set_wideband_resample: blocks arrive at rs.rate_hz and reach the bank through the resampler.  Kept over a reset
    bool started = false;           // the seam has taken a block since create or reset: the resampler can no longer be set or removed
};

inline double bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 64; k++) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; if (t < 1e-18 * s) break; }
    return s;
}

// Kaiser(beta = 8) windowed sinc at the bank's sample rate, unit DC gain; -6 dB at the bank's cut-off for D input samples per frame
// (ChzBank::cutoff_hz: 13 kHz in front of three samples per symbol, 15 kHz in front of two)
inline std::vector<float> chz_design_taps(const ChzBank &bank, uint32_t D)
{
    const int L = (int)(bank.taps * bank.M);
    const double fc = bank.cutoff_hz(D) / bank.sample_rate_hz();   // cycles per sample
    const double beta = 8.0, i0b = bessel_i0(beta);
    std::vector<double> h(L);
    double sum = 0.0;
    for (int i = 0; i < L; i++) {
        const double m = i - 0.5 * (L - 1);
        const double x = 2.0 * fc * m;
        const double sinc = std::fabs(x) < 1e-12 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double r = 2.0 * i / (L - 1) - 1.0;
        const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        h[i] = 2.0 * fc * sinc * w;
        sum += h[i];
    }
    std::vector<float> out(L);
    for (int i = 0; i < L; i++) out[i] = (float)(h[i] / sum);
    return out;
}

inline int channelizer_reset(ChannelizerState &z, hipStream_t s)
{
    if (!z.enabled) return 0;
    const size_t cap = z.bank->carry_cap(z.D);
    if (hipMemsetAsync(z.carry[0].get(), 0, sizeof(float2) * cap, s) != hipSuccess) return -EIO;
    if (hipMemsetAsync(z.carry[1].get(), 0, sizeof(float2) * cap, s) != hipSuccess) return -EIO;
    z.carry_cur = 0;
    z.carry_len = z.bank->hist(z.D);                 // all-zero history, no leftover
    z.frames_done = 0;
    z.started = false;
    return wb_resample_reset(z.rs, s);
}

inline void channelizer_destroy(ChannelizerState &z) { z = ChannelizerState(); }

// The filter bank of a cfg that chz_resolve_cfg has admitted and filled in: what can still fail here is allocation and copies.
inline int channelizer_create(ChannelizerState &z, const amps_recc_cfg_t &cfg)
{
    const ChzBank &bank = *chz_bank_of(cfg.wideband_channels);
    const uint32_t M = bank.M, D = cfg.wideband_decim;
    std::vector<uint16_t> b2r;
    z.C = chz_rows(bank, cfg, &b2r, &z.row2chan);
    z.bank = &bank; z.D = D;
    z.groups = cfg.wideband_groups > 1 ? cfg.wideband_groups : 1u; z.group = cfg.wideband_group;
    if (z.bin2row.alloc(M)) return -ENOMEM;
    if (hipMemcpy(z.bin2row.get(), b2r.data(), sizeof(uint16_t) * M, hipMemcpyHostToDevice) != hipSuccess) return -EIO;
    z.max_frames = cfg.max_samples_per_push;
    z.ld = ((uint64_t)z.max_frames + 7) & ~7ull;
    const std::vector<float> h = chz_design_taps(bank, D);
    if (z.taps.alloc(h.size())) return -ENOMEM;
    if (hipMemcpy(z.taps.get(), h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice) != hipSuccess) return -EIO;
    if (z.carry[0].alloc(bank.carry_cap(D)) || z.carry[1].alloc(bank.carry_cap(D))) return -ENOMEM;
    if (bank.family != ChzFamily::FUSED1024) {
        const std::vector<float2> w = chz_narrow_twiddles((int)M);
        if (z.twiddle.alloc(M)) return -ENOMEM;
        if (hipMemcpy(z.twiddle.get(), w.data(), sizeof(float2) * M, hipMemcpyHostToDevice) != hipSuccess) return -EIO;
    }
    // z.out (the channel-major block, C x ld x 8 B: 1.7 GB for a full band at 2^18 frames per push) is allocated by the first
    // unfused / debug run: the fused form never touches it
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            z.target_wgs = (uint32_t)prop.multiProcessorCount;
    }
    z.short_prepass = env_read("AMPS_RECC_SHORT_PREPASS", env_one);   // at every create, not once: scripts/bench_short_input.py changes it between two handles of one process
    z.enabled = true;
    return 0;
}

static_assert(CHZ_BANKS[0].M == (uint32_t)CHZ_M && CHZ_BANKS[0].decim[0] == (uint32_t)CHZ_D768 && CHZ_BANKS[0].decim[1] == (uint32_t)CHZ_D && CHZ_BANKS[0].taps == 8u,
              "recc_chz_banks.h states the 1024 bank as chz12_kernel is built");
typedef void (*chz_kernel_t)(ChzArgs);
// the filter-bank instantiation for (input samples per frame, fused slicer or channel-major IQ out, slicer spec, sample type of the
// block: fc32, or sc16 read in place -- fused form only)
template <int DEC, bool SHORT, int MODE> chz_kernel_t chz12_kernel_of()
{
    if constexpr (SHORT) return chz12_short_kernel<8, MODE, DEC>;
    else return chz12_kernel<8, MODE, DEC>;
}
template <int DEC, bool SHORT> chz_kernel_t chz12_kernel_of(int slicer)
{
    switch (slicer) {
    case AMPS_SLICER_PRODUCT: return chz12_kernel_of<DEC, SHORT, AMPS_SLICER_PRODUCT>();
    case AMPS_SLICER_SINE: return chz12_kernel_of<DEC, SHORT, AMPS_SLICER_SINE>();
    case AMPS_SLICER_EXACT: return chz12_kernel_of<DEC, SHORT, AMPS_SLICER_EXACT>();
    default: return chz12_kernel_of<DEC, SHORT, AMPS_SLICER_ATAN_BOXCAR>();
    }
}
inline chz_kernel_t chz12_kernel_for(int D, bool fused, int slicer, bool sc16 = false)
{
    if (!fused) {
        if (sc16) return nullptr;
        return D == CHZ_D768 ? chz12_kernel_of<CHZ_D768, false, CHZ12_IQ>() : chz12_kernel_of<CHZ_D, false, CHZ12_IQ>();
    }
    if (D == CHZ_D768) return sc16 ? chz12_kernel_of<CHZ_D768, true>(slicer) : chz12_kernel_of<CHZ_D768, false>(slicer);
    return sc16 ? chz12_kernel_of<CHZ_D, true>(slicer) : chz12_kernel_of<CHZ_D, false>(slicer);
}

// The two-kernel families' instantiation for (branches, input samples per frame, sample type of the block, read in place), behind
// Args = ChzNarrowArgs, or behind Args = ChzMixArgs its mixing twin.  The 8-bit types of the narrow banks go by a name of their own.
template <class Args> using chz_bank_kernel_t = void (*)(Args);
template <class Args, int M, int DEC, typename T> constexpr chz_bank_kernel_t<Args> chz_bank_kernel_of()
{
    constexpr bool mix = std::is_same<Args, ChzMixArgs>::value;
    if constexpr (chz_grid10_size(M)) { if constexpr (mix) return chz_grid10_mix_kernel<M, T>; else return chz_grid10_kernel<M, T>; }
    else if constexpr (mix) return chz_narrow_mix_kernel<M, DEC, T>;
    else if constexpr (sizeof(T) == 2) return chz_narrow_b8_kernel<M, DEC, T>;
    else return chz_narrow_kernel<M, DEC, T>;
}
// ... for (bank, one of its decimations, AMPS_RECC_SAMPLES_*); nullptr for a bank or a format there is none for
template <class Args> inline chz_bank_kernel_t<Args> chz_bank_kernel_for(const ChzBank &bank, uint32_t D, int format)
{
    return chz_with_sample_type(format, [&](auto t) -> chz_bank_kernel_t<Args> {
        using T = decltype(t);
        const bool first = D == bank.decim[0];                    // 3 M / 4 at the narrow banks
        switch (bank.M) {
        case 512: return first ? chz_bank_kernel_of<Args, 512, 384, T>() : chz_bank_kernel_of<Args, 512, 256, T>();
        case 256: return first ? chz_bank_kernel_of<Args, 256, 192, T>() : chz_bank_kernel_of<Args, 256, 128, T>();
        case 128: return first ? chz_bank_kernel_of<Args, 128, 96, T>() : chz_bank_kernel_of<Args, 128, 64, T>();
        case 2500: return chz_bank_kernel_of<Args, 2500, 625, T>();
        case 2000: return chz_bank_kernel_of<Args, 2000, 500, T>();
        case 1000: return chz_bank_kernel_of<Args, 1000, 250, T>();
        case 500: return chz_bank_kernel_of<Args, 500, 125, T>();
        default: return nullptr;
        }
    });
}
// the carry kernel behind a push of T, and the conversion to fc32 in front of the fused family's kernels (none for fc32 itself)
template <typename T> constexpr auto chz_carry_kernel_of()
{
    if constexpr (std::is_same<T, float2>::value) return chz_carry_kernel;
    else if constexpr (std::is_same<T, chz_sc16>::value) return chz_carry_short_kernel;
    else return chz_carry_b8_kernel<T>;
}
template <typename T> constexpr auto chz_to_float_kernel_of()
{
    if constexpr (std::is_same<T, chz_sc16>::value) return chz_short_to_float_kernel;
    else return chz_b8_to_float_kernel<T>;
}

// What channelizer_run is given: the block, the form, and what the fused form writes into.
struct ChzRunIn {
    const void *iq = nullptr;                // `nsamp` new wideband samples, host or device (`mem`: AMPS_MEM_*)
    size_t nsamp = 0;
    int mem = AMPS_MEM_DEVICE;
    int format = AMPS_RECC_SAMPLES_FC32;     // AMPS_RECC_SAMPLES_*.  sc16: read in place by the fused form and the narrow banks, expanded to fc32 first otherwise;
                                             // sc8 / cu8: read in place by the narrow banks, expanded to fc32 first at M = 1024
    bool fused = false;                      // false: the channel-major block (*chan_iq / *ld / *nframes; even number of frames); true: slicer bits only, 64 frames at a time
    uint64_t *gring = nullptr;               // fused: the slicer-bit ring, written at absolute sample index n_done..
    uint32_t ring_words = 0;
    uint64_t n_done = 0;
    int slicer = AMPS_SLICER_ATAN_BOXCAR;
    const PowerRing *power = nullptr;        // fused: the power ring of a handle that keeps one (AMPS_RECC_FLAG_CHANNEL_POWER)
    void (*after_main)(void *) = nullptr;    // called behind the filter-bank launch, in front of the carry and power launches (timing)
    void *after_ctx = nullptr;
};

// Channelise in.nsamp new wideband samples.
inline int channelizer_run(ChannelizerState &z, const ChzRunIn &in, hipStream_t s, const float2 **chan_iq, uint64_t *ld, uint32_t *nframes_out)
{
    if (!z.enabled) return -ENOSYS;
    const ChzBank &bank = *z.bank;
    const bool chz12 = bank.family == ChzFamily::FUSED1024;       // chz12_kernel; the other families: the two-kernel form whatever was asked, every sample format read in place
    const bool fused = in.fused && bank.has(CHZ_HAS_FUSED);
    // behind a resampler the bank sees the resampler's outputs: their number is host arithmetic, so that a push that is too large is
    // refused below before anything moves
    const uint64_t nsamp64 = z.rs.enabled ? wb_resample_count(z.rs, in.nsamp) : in.nsamp;
    if (z.rs.enabled && nsamp64 > 0xffffffffull) return -E2BIG;
    const size_t nsamp = (size_t)nsamp64;
    int format = in.format;
    if (!chz_sample_bytes(format)) return -EINVAL;
    if (!fused && z.groups > 1) return -ENOSYS;                   // channel groups exist in the fused form only
    const void *d = in.iq;
    if (in.mem == AMPS_MEM_HOST) {                                // one row of bytes, as the caller's samples
        const size_t bytes = chz_sample_bytes(format) * in.nsamp;
        const uint8_t *staged = nullptr;
        uint64_t pitch = 0;
        if (int rc = z.stage.stage((const uint8_t *)in.iq, bytes, bytes, 1, bytes, &staged, &pitch)) return rc;
        d = staged;
    }
    if (!fused && !z.out && z.out.alloc((size_t)z.C * z.ld)) return -ENOMEM;
    const uint32_t hist = bank.hist(z.D);
    const uint32_t leftover = z.carry_len - hist;
    const uint64_t avail = (uint64_t)leftover + nsamp;
    // frames consumed: whole periods of the roll (a launch starts where the stream position is a multiple of M: frame parity 0 at
    // D = M / 2, frame phase 0 of 4 at D = 3 M / 4 and at D = M / 4), and in the fused form a multiple of 64 (whole words of the RECC bit ring); the rest waits in the carry
    const uint32_t nframes = (uint32_t)(avail / z.D) & bank.frame_mask(z.D, fused);
    if (nframes > z.max_frames) return -E2BIG;
    if (z.rs.enabled) {
        // the block at the delivered rate -> fc32 at the bank's rate in a buffer of the resampler's, then everything as for a device fc32 block
        uint32_t n = 0;
        if (int rc = wb_resample_run(z.rs, d, in.nsamp, format, s, &n)) return rc;
        d = z.rs.out.get();
        format = AMPS_RECC_SAMPLES_FC32;
    }
    if (chz12 && format != AMPS_RECC_SAMPLES_FC32 && (format != AMPS_RECC_SAMPLES_SC16 || !fused || z.short_prepass)) {
        // the block as fc32 in a buffer of its own, then everything as for an fc32 block.  Stream order keeps the buffer safe: the
        // kernels of the previous push that read it run before this conversion
        if (z.cvt.capacity() < nsamp) {
            if (z.cvt && hipStreamSynchronize(s) != hipSuccess) return -EIO;       // ... so they must have run before it is freed to grow
            if (z.cvt.reserve(nsamp)) return -ENOMEM;
        }
        const uint32_t blocks = (uint32_t)std::min<size_t>((nsamp + 255) / 256, 65536);
        chz_with_sample_type(format, [&](auto t) {
            using T = decltype(t);
            if constexpr (!std::is_same<T, float2>::value) hipLaunchKernelGGL(chz_to_float_kernel_of<T>(), dim3(blocks), dim3(256), 0, s, (const T *)d, z.cvt.get(), (uint32_t)nsamp);
            return 0;
        });
        d = z.cvt.get();
        format = AMPS_RECC_SAMPLES_FC32;
    }
    const bool sc16 = format == AMPS_RECC_SAMPLES_SC16;          // what is left of the formats in front of chz12_kernel
    const uint32_t consumed = nframes * z.D;                          // virtual samples consumed (incl. leftover)
    const uint32_t new_left = (uint32_t)(avail - consumed);
    bool carry_in_kernel = false;
    ChzArgs a{};
    if (nframes && !chz12) {
        ChzNarrowArgs na{};
        na.block = d; na.carry = z.carry[z.carry_cur].get(); na.taps = z.taps.get(); na.twiddle = z.twiddle.get(); na.out = z.out.get(); na.ld = z.ld;
        na.bin2row = z.bin2row.get(); na.carry_len = z.carry_len; na.nsamp = (uint32_t)nsamp; na.nframes = nframes; na.n_channels = z.C;
        const uint32_t fr = bank.fr[bank.decim_index(z.D)];
        const dim3 grid((nframes + fr - 1) / fr);
        if (z.shift.step) {
            // every launch mixes all it stages, carry included (the carry keeps unmixed input), by the sample's absolute index
            const ChzMixArgs ma{ na, (int64_t)(z.frames_done * (uint64_t)z.D) - (int64_t)hist, z.shift.step };
            const auto kern = chz_bank_kernel_for<ChzMixArgs>(bank, z.D, format);
            if (!kern) return -EINVAL;
            hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, ma);
        } else {
            const auto kern = chz_bank_kernel_for<ChzNarrowArgs>(bank, z.D, format);
            if (!kern) return -EINVAL;
            hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, na);
        }
    } else if (nframes) {
        a.block = (const float2 *)d; a.carry = z.carry[z.carry_cur].get(); a.taps = z.taps.get(); a.out = z.out.get(); a.ld = z.ld;
        a.carry_len = z.carry_len; a.nsamp = (uint32_t)nsamp; a.nframes = nframes; a.hist = hist;
        // one resident round of 768-thread workgroups, one per CU; each refills its delay lines and re-runs eight pre-roll
        // frames when fused, so fewer, longer runs are cheaper
        uint32_t fpw = std::max<uint32_t>(64u, (nframes + z.target_wgs - 1) / z.target_wgs);
        fpw = (fpw + 63) / 64 * 64;
        a.frames_per_wg = fpw; a.n_channels = z.C;
        a.bin2row = z.bin2row.get(); a.grp_w = 64u / z.groups; a.grp_r = z.group;
        a.gring = in.gring; a.ring_words = in.ring_words; a.n_done = in.n_done;
        a.stream_start = z.frames_done == 0 ? 1u : 0u;
        const dim3 g12((nframes + fpw - 1) / fpw), b12(768);
        carry_in_kernel = g12.x >= 64;                                // a slice of at most ~700 samples per workgroup; smaller grids leave it to the copy kernel
        if (carry_in_kernel) { a.carry_out = z.carry[z.carry_cur ^ 1].get(); a.consumed = consumed; a.carry_out_len = hist + new_left; }
#ifdef CHZ_TIMELINE
        if (!(a.tl = chz_timeline().clear(CHZ_TL_STAMPS, CHZ_TL_STAMPS, s))) return -ENOMEM;
#endif
        hipLaunchKernelGGL(chz12_kernel_for(z.D, fused, in.slicer, sc16), g12, b12, 0, s, a);
    }
    if (in.after_main) in.after_main(in.after_ctx);                            // timing: the span ends behind the filter-bank kernel, before the carry copy
    // power snapshots (opt-in): behind the filter bank, from the block and the carry it read -- the carry buffers swap below
    if (fused && in.power && nframes) chz_power_launch(*in.power, z.D, a, sc16, s);
#ifdef CHZ_TIMELINE
    if (a.tl) chz_timeline().dump("AMPS_RECC_CHZ_TIMELINE", CHZ_TL_STAMPS, s);   // the last launch's stamps
#endif
    if (!carry_in_kernel) {
        chz_with_sample_type(format, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(chz_carry_kernel_of<T>(), dim3((hist + new_left + 255) / 256), dim3(256), 0, s, (const T *)d, z.carry[z.carry_cur].get(),
                               z.carry[z.carry_cur ^ 1].get(), z.carry_len, (uint32_t)nsamp, hist, consumed, hist + new_left);
            return 0;
        });
    }
    if (hipGetLastError() != hipSuccess) return -EIO;
    if (in.mem == AMPS_MEM_HOST) { if (int rc = z.stage.arm(s)) return rc; }
    z.carry_cur ^= 1;
    z.carry_len = hist + new_left;
    z.frames_done += nframes;
    z.started = true;
    if (chan_iq) *chan_iq = z.out.get();
    if (ld) *ld = z.ld;
    *nframes_out = nframes;
    return 0;
}

} // namespace amps
