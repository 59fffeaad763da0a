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
// The parts, one concern per header: recc_chz_common.hip.h (constants, ChzArgs, sample types, packed fp32), recc_chz_fft.hip.h (the
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
    int P = 8;
    int M = CHZ_M;                  // branches: 1024 (chz12_kernel), or 512, 256, 128 (chz_narrow_kernel) or 2500, 2000, 1000, 500 (chz_grid10_kernel): the two-kernel form only
    int D = CHZ_D;                  // input samples per frame: M / 2 (3 samples per symbol) or 3 M / 4 (2); M / 4 (2) at the banks of 10 kHz bins
    uint32_t C = 0;                 // rows this handle decodes (= the band's channels, or one group of them)
    uint32_t groups = 1, group = 0; // cfg.wideband_groups / wideband_group
    DevBuf<uint16_t> bin2row;       // device [M]
    std::vector<uint32_t> row2chan; // row -> channel number within the band selection (what the records carry)
    uint32_t max_frames = 0;        // per push
    uint32_t target_wgs = 256;      // resident workgroups of the filter-bank kernel (one 768-thread workgroup per CU)
    DevBuf<float> taps;             // [L]
    DevBuf<float2> twiddle;         // M < 1024: [M], e^{-2 pi i k / M}
    DevBuf<float2> carry[2];
    int carry_cur = 0;
    uint32_t carry_len = 0;         // L - D + leftover
    uint64_t frames_done = 0;
    WidebandShift shift;            // amps_recc_set_wideband_shift (M < 1024): a non-zero step launches the mixing twins.  Kept over a reset
    DevBuf<float2> out;             // [C][ld]
    uint64_t ld = 0;
    HostStage stage;                // host-resident wideband input as the caller's samples (fc32, sc16, sc8 or cu8), sized in bytes: the largest block so far
    DevBuf<float2> cvt;             // an integer block expanded to fc32, M = 1024 only: sc16 in the checking modes and the pre-pass experiment, sc8 / cu8 always
    bool short_prepass = false;     // AMPS_RECC_SHORT_PREPASS=1 at create: sc16 blocks go through chz_short_to_float_kernel + the fc32 kernel
};

inline double bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 64; k++) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; if (t < 1e-18 * s) break; }
    return s;
}

// Kaiser(beta = 8) windowed sinc at fs = M * bin_hz (30 kHz; 10 kHz at the banks of recc_chz_grid10.hip.h), unit DC gain; -6 dB at 13 kHz behind the D = M / 2 bank, at 15 kHz behind the D = 3 M / 4 one
// (40 ksps per channel leave the slicer two sampling phases per symbol instead of three: the wider pass band gives back, under a
// carrier offset, what the coarser timing costs -- profiles/r06/decim768_cpu_gonogo.txt; oracle/channelizer.py: cutoff_for_decim)
// The banks of 10 kHz bins (D = M / 4) deliver 40 ksps per channel too and take the same 15 kHz.
inline double chz_cutoff_hz(int D, int M = CHZ_M) { return (4 * D == 3 * M || chz_grid10_geometry(M, D)) ? 15.0e3 : 13.0e3; }
inline std::vector<float> chz_design_taps(int P, int D = CHZ_D, int M = CHZ_M, double bin_hz = 30.0e3)
{
    const int L = P * M;
    const double fc = chz_cutoff_hz(D, M) / (M * bin_hz);        // cycles per sample
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

// samples of history the carry holds in front of a launch's frame 0: the filter's own L - D, and at M = 1024 the pre-roll's CHZ_PRE
// frames (the narrow banks have no pre-roll: a workgroup stages its frames' whole history)
inline uint32_t chz_hist(int P, int D, int M = CHZ_M) { return (uint32_t)(P * M - D + (M == CHZ_M ? CHZ_PRE * D : 0)); }
inline size_t chz_carry_cap(int P, int D, int M = CHZ_M) { return (size_t)chz_hist(P, D, M) + 64 * D; }   // + leftover (< 64 frames)

inline int channelizer_reset(ChannelizerState &z, hipStream_t s)
{
    if (!z.enabled) return 0;
    const size_t cap = chz_carry_cap(z.P, z.D, z.M);
    if (hipMemsetAsync(z.carry[0].get(), 0, sizeof(float2) * cap, s) != hipSuccess) return -EIO;
    if (hipMemsetAsync(z.carry[1].get(), 0, sizeof(float2) * cap, s) != hipSuccess) return -EIO;
    z.carry_cur = 0;
    z.carry_len = chz_hist(z.P, z.D, z.M);           // all-zero history, no leftover
    z.frames_done = 0;
    return 0;
}

inline void channelizer_destroy(ChannelizerState &z) { z = ChannelizerState(); }

// the bank sizes of chz_narrow_kernel
inline bool chz_is_narrow(uint32_t M) { return M == 512 || M == 256 || M == 128; }
// the bank sizes of chz_grid10_kernel: bins of 10 kHz, an AMPS channel on every third
inline bool chz_is_grid10(uint32_t M) { return chz_grid10_size((int)M); }
// what a bank of M branches is laid out for: the width of a bin, the bins from one channel to the next, the taps per branch
inline double chz_bin_hz(uint32_t M) { return chz_is_grid10(M) ? CHZ_GRID10_BIN_HZ : 30.0e3; }
inline uint32_t chz_channel_stride(uint32_t M) { return chz_is_grid10(M) ? (uint32_t)CHZ_GRID10_STRIDE : 1u; }
inline uint32_t chz_taps_per_branch(uint32_t M) { return chz_is_grid10(M) ? (uint32_t)CHZ_GRID10_P : 8u; }
// The geometries the seam serves: M = 1024, 512, 256 or 128 branches of 30 kHz at D = M / 2 or 3 M / 4 input samples per frame, and
// M = 2500, 2000, 1000 or 500 branches of 10 kHz at D = M / 4
inline bool chz_geometry_ok(uint32_t M, uint32_t D)
{
    if (chz_is_grid10(M)) return 4 * D == M;
    return (M == (uint32_t)CHZ_M || chz_is_narrow(M)) && (2 * D == M || 4 * D == 3 * M);
}

// bins and rows of a handle: row i = the i-th channel (in band order) of the band selection -- n channels from bin `first` on, a bin
// apart, or three on the banks of 10 kHz bins -- that belongs to the handle's group -- all of them without groups.  Returns the row count, or a negative errno for an invalid split.
inline int chz_rows(const amps_recc_cfg_t &cfg, std::vector<uint16_t> *bin2row, std::vector<uint32_t> *row2chan)
{
    const uint32_t G = cfg.wideband_groups > 1 ? cfg.wideband_groups : 1u;
    const uint32_t M = chz_is_narrow(cfg.wideband_channels) || chz_is_grid10(cfg.wideband_channels) ? cfg.wideband_channels : (uint32_t)CHZ_M;
    const uint32_t stride = chz_channel_stride(M);
    if ((G != 1 && G != 2 && G != 4 && G != 8) || cfg.wideband_group >= G) return -EINVAL;
    if ((uint64_t)stride * cfg.n_channels > M || cfg.wideband_first_channel >= M) return -EINVAL;
    const uint32_t W = 64u / G;
    if (bin2row) bin2row->assign(M, (uint16_t)0xffffu);
    if (row2chan) row2chan->clear();
    uint32_t rows = 0;
    for (uint32_t c = 0; c < cfg.n_channels; c++) {
        const uint32_t k = (cfg.wideband_first_channel + stride * c) % M;
        if ((k & 63u) / W != cfg.wideband_group) continue;
        if (bin2row) (*bin2row)[k] = (uint16_t)rows;
        if (row2chan) row2chan->push_back(c);
        rows++;
    }
    return (int)rows;
}

inline int channelizer_create(ChannelizerState &z, const amps_recc_cfg_t &cfg)
{
    if (!chz_geometry_ok(cfg.wideband_channels, cfg.wideband_decim)) return -EINVAL;
    const int M = (int)cfg.wideband_channels;
    const bool narrow = M != CHZ_M;
    if (narrow && cfg.wideband_groups > 1) return -EINVAL;         // channel groups exist in the fused form, which the narrow banks do not have
    const int P = cfg.wideband_taps_per_branch ? (int)cfg.wideband_taps_per_branch : (int)chz_taps_per_branch((uint32_t)M);
    if (P != (int)chz_taps_per_branch((uint32_t)M)) return -EINVAL;   // the register ring of chz12_kernel is laid out for eight taps per branch, and so is chz_narrow_kernel's fold; chz_grid10_kernel's for three
    if ((uint64_t)chz_channel_stride((uint32_t)M) * cfg.n_channels > (uint32_t)M || cfg.wideband_first_channel >= (uint32_t)M || cfg.max_samples_per_push == 0) return -EINVAL;
    std::vector<uint16_t> b2r;
    const int rows = chz_rows(cfg, &b2r, &z.row2chan);
    if (rows < 1) return rows < 0 ? rows : -EINVAL;
    z.P = P; z.M = M; z.D = (int)cfg.wideband_decim; z.C = (uint32_t)rows;
    z.groups = cfg.wideband_groups > 1 ? cfg.wideband_groups : 1u; z.group = cfg.wideband_group;
    if (z.bin2row.alloc(M)) return -ENOMEM;
    if (hipMemcpy(z.bin2row.get(), b2r.data(), sizeof(uint16_t) * M, hipMemcpyHostToDevice) != hipSuccess) return -EIO;
    z.max_frames = cfg.max_samples_per_push;
    z.ld = ((uint64_t)z.max_frames + 7) & ~7ull;
    const size_t L = (size_t)P * M;
    std::vector<float> h = chz_design_taps(P, z.D, M, chz_bin_hz((uint32_t)M));
    if (z.taps.alloc(L)) return -ENOMEM;
    if (hipMemcpy(z.taps.get(), h.data(), sizeof(float) * L, hipMemcpyHostToDevice) != hipSuccess) return -EIO;
    if (z.carry[0].alloc(chz_carry_cap(P, z.D, M)) || z.carry[1].alloc(chz_carry_cap(P, z.D, M))) return -ENOMEM;
    if (narrow) {
        const std::vector<float2> w = chz_narrow_twiddles(M);
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
    const bool narrow = z.M != CHZ_M;                             // chz_narrow_kernel: the two-kernel form whatever was asked, every sample format read in place
    const bool fused = in.fused && !narrow;
    const size_t nsamp = in.nsamp;
    int format = in.format;
    if (!z.enabled) return -ENOSYS;
    if (!chz_sample_bytes(format)) return -EINVAL;
    if (!fused && z.groups > 1) return -ENOSYS;                   // channel groups exist in the fused form only
    const void *d = in.iq;
    if (in.mem == AMPS_MEM_HOST) {                                // one row of bytes, as the caller's samples
        const size_t bytes = chz_sample_bytes(format) * nsamp;
        const uint8_t *staged = nullptr;
        uint64_t pitch = 0;
        if (int rc = z.stage.stage((const uint8_t *)in.iq, bytes, bytes, 1, bytes, &staged, &pitch)) return rc;
        d = staged;
    }
    if (!fused && !z.out && z.out.alloc((size_t)z.C * z.ld)) return -ENOMEM;
    const uint32_t hist = chz_hist(z.P, z.D, z.M);
    const uint32_t leftover = z.carry_len - hist;
    const uint64_t avail = (uint64_t)leftover + nsamp;
    // frames consumed: a multiple of two or four (a launch starts where the stream position is a multiple of M: frame parity 0 at
    // D = M / 2, frame phase 0 of 4 at D = 3 M / 4 and at D = M / 4), and in the fused form a multiple of 64 (whole words of the RECC bit ring); the rest waits in the carry
    const uint32_t nframes = (uint32_t)(avail / (uint32_t)z.D) & (fused ? ~63u : 2 * z.D == z.M ? ~1u : ~3u);
    if (nframes > z.max_frames) return -E2BIG;
    const bool b8 = format == AMPS_RECC_SAMPLES_SC8 || format == AMPS_RECC_SAMPLES_CU8;
    if (!narrow && (b8 || (format == AMPS_RECC_SAMPLES_SC16 && (!fused || z.short_prepass)))) {
        // the block as fc32 in a buffer of its own, then everything as for an fc32 block.  Stream order keeps the buffer safe: the
        // kernels of the previous push that read it run before this conversion
        if (z.cvt.capacity() < nsamp) {
            if (z.cvt && hipStreamSynchronize(s) != hipSuccess) return -EIO;       // ... so they must have run before it is freed to grow
            if (z.cvt.reserve(nsamp)) return -ENOMEM;
        }
        const uint32_t blocks = (uint32_t)std::min<size_t>((nsamp + 255) / 256, 65536);
        if (format == AMPS_RECC_SAMPLES_SC8) hipLaunchKernelGGL(chz_b8_to_float_kernel<xl_sc8>, dim3(blocks), dim3(256), 0, s, (const xl_sc8 *)d, z.cvt.get(), (uint32_t)nsamp);
        else if (format == AMPS_RECC_SAMPLES_CU8) hipLaunchKernelGGL(chz_b8_to_float_kernel<xl_cu8>, dim3(blocks), dim3(256), 0, s, (const xl_cu8 *)d, z.cvt.get(), (uint32_t)nsamp);
        else hipLaunchKernelGGL(chz_short_to_float_kernel, dim3(blocks), dim3(256), 0, s, (const chz_sc16 *)d, z.cvt.get(), (uint32_t)nsamp);
        d = z.cvt.get();
        format = AMPS_RECC_SAMPLES_FC32;
    }
    const bool sc16 = format == AMPS_RECC_SAMPLES_SC16;          // what is left of the formats at M = 1024
    const uint32_t consumed = nframes * (uint32_t)z.D;                // virtual samples consumed (incl. leftover)
    const uint32_t new_left = (uint32_t)(avail - consumed);
    bool carry_in_kernel = false;
    ChzArgs a{};
    if (nframes && narrow) {
        ChzNarrowArgs na{};
        na.block = d; na.carry = z.carry[z.carry_cur].get(); na.taps = z.taps.get(); na.twiddle = z.twiddle.get(); na.out = z.out.get(); na.ld = z.ld;
        na.bin2row = z.bin2row.get(); na.carry_len = z.carry_len; na.nsamp = (uint32_t)nsamp; na.nframes = nframes; na.n_channels = z.C;
        const bool grid10 = chz_is_grid10((uint32_t)z.M);
        const uint32_t fr = (uint32_t)(grid10 ? chz_grid10_fr(z.M) : chz_narrow_fr(z.M, z.D));
        if (z.shift.step) {
            // every launch mixes all it stages, carry included (the carry keeps unmixed input), by the sample's absolute index
            const ChzMixArgs ma{ na, (int64_t)(z.frames_done * (uint64_t)z.D) - (int64_t)hist, z.shift.step };
            const chz_mix_kernel_t kern = grid10 ? chz_grid10_mix_kernel_for(z.M, format) : chz_narrow_mix_kernel_for(z.M, z.D, format);
            if (!kern) return -EINVAL;
            hipLaunchKernelGGL(kern, dim3((nframes + fr - 1) / fr), dim3(256), 0, s, ma);
        } else {
            const chz_narrow_kernel_t kern = grid10 ? chz_grid10_kernel_for(z.M, format) : chz_narrow_kernel_for(z.M, z.D, format);
            if (!kern) return -EINVAL;
            hipLaunchKernelGGL(kern, dim3((nframes + fr - 1) / fr), dim3(256), 0, s, na);
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
        if (sc16) hipLaunchKernelGGL(chz_carry_short_kernel, dim3((hist + new_left + 255) / 256), dim3(256), 0, s, (const chz_sc16 *)d, z.carry[z.carry_cur].get(),
                                     z.carry[z.carry_cur ^ 1].get(), z.carry_len, (uint32_t)nsamp, hist, consumed, hist + new_left);
        else if (format == AMPS_RECC_SAMPLES_SC8) hipLaunchKernelGGL(chz_carry_b8_kernel<xl_sc8>, dim3((hist + new_left + 255) / 256), dim3(256), 0, s, (const xl_sc8 *)d, z.carry[z.carry_cur].get(),
                                     z.carry[z.carry_cur ^ 1].get(), z.carry_len, (uint32_t)nsamp, hist, consumed, hist + new_left);
        else if (format == AMPS_RECC_SAMPLES_CU8) hipLaunchKernelGGL(chz_carry_b8_kernel<xl_cu8>, dim3((hist + new_left + 255) / 256), dim3(256), 0, s, (const xl_cu8 *)d, z.carry[z.carry_cur].get(),
                                     z.carry[z.carry_cur ^ 1].get(), z.carry_len, (uint32_t)nsamp, hist, consumed, hist + new_left);
        else hipLaunchKernelGGL(chz_carry_kernel, dim3((hist + new_left + 255) / 256), dim3(256), 0, s, (const float2 *)d, z.carry[z.carry_cur].get(),
                                z.carry[z.carry_cur ^ 1].get(), z.carry_len, (uint32_t)nsamp, hist, consumed, hist + new_left);
    }
    if (hipGetLastError() != hipSuccess) return -EIO;
    if (in.mem == AMPS_MEM_HOST) { if (int rc = z.stage.arm(s)) return rc; }
    z.carry_cur ^= 1;
    z.carry_len = hist + new_left;
    z.frames_done += nframes;
    if (chan_iq) *chan_iq = z.out.get();
    if (ld) *ld = z.ld;
    *nframes_out = nframes;
    return 0;
}

} // namespace amps
