// recc_chz_common.hip.h -- what every part of the filter bank (recc_channelizer.hip.h) shares, and what the translate seam borrows
// from it: the bank's constants and kernel arguments, the sample types of a block, the buffer descriptor of the fast loader and the
// packed-fp32 operations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "amps_recc.h"              // AMPS_RECC_SAMPLES_*
#include "recc_chz_banks.h"         // the table of bank sizes; CHZ_PRE

namespace amps {

constexpr int CHZ_M = 1024;          // branches = FFT size
constexpr int CHZ_D = 512;           // input samples per frame of the default form (2x oversampled: 60 ksps per channel, 3 samples per symbol)
constexpr int CHZ_D768 = 768;        // ... of the 4/3 x oversampled form (40 ksps per channel, 2 samples per symbol; round 6, recc_chz_fold.hip.h, section "D = 768")

struct ChzArgs {
    const float2 *block;     // new wideband samples of this push (chz12_short_kernel: the same pointer holds chz_sc16 samples)
    const float2 *carry;     // samples [f_done*D + D - L, f_done*D + leftover) of the stream so far
    const float *taps;       // [L] prototype
    float2 *out;             // [C][ld] channel-major output of this push
    uint64_t ld;
    uint32_t carry_len;      // L - D + leftover
    uint32_t nsamp;          // new samples
    uint32_t nframes;        // frames produced by this launch
    uint32_t frames_per_wg;  // multiple of 64
    uint32_t first_bin;      // unused by the kernels (they go by bin2row), left zero; kept so that no argument offset moves
    uint32_t n_channels;     // rows of `out` / `gring` this handle owns
    const uint16_t *bin2row; // [M]: row of FFT bin k in `out` / `gring`, >= n_channels for a bin this handle does not decode
    uint32_t grp_w, grp_r;   // channel groups (cfg.wideband_groups): this handle's bins are those with (k mod 64) in [grp_r * grp_w,
                             // (grp_r + 1) * grp_w); grp_w = 64, grp_r = 0: every bin
    uint32_t odd_start;      // unused by the kernels (a launch starts on frame parity 0), left zero; kept for the layout like first_bin
    uint32_t hist;           // samples of history the carry holds before v = 0  (L - D + CHZ_PRE * D)
    // fused form: slicer bits go straight to the RECC bit ring
    uint64_t *gring;         // [C][ring_words]
    uint32_t ring_words;
    uint64_t n_done;         // absolute channel-stream sample index of frame 0 (multiple of 64)
    uint32_t stream_start;   // frame 0 of this launch is the first frame of the stream (spec B: its first 3 bits are ones)
    // the carry of the NEXT launch, written by this one (every workgroup copies a slice; the two carry buffers alternate)
    float2 *carry_out;       // [carry_out_len]: virtual samples [consumed - hist, consumed - hist + carry_out_len)
    uint32_t consumed, carry_out_len;
    unsigned long long *tl;  // CHZ_TIMELINE builds: s_memtime stamps of workgroup 0 ([wave][step][8]), else unused
};

typedef float cf2 __attribute__((ext_vector_type(2)));
// A sample of the wideband block as the caller hands it over: fc32 (float2) or interleaved 16-bit I/Q ("sc16": I in the low half of
// the dword).  The sc16 form is DEFINED as the fc32 form on the plainly converted block (amps_recc_push_wideband_short): every int16 is
// exact in fp32, so both forms run the same fp32 operations on the same values.  Carry buffers stay fc32 whatever the block was.
struct alignas(4) chz_sc16 { int16_t x, y; };
template <typename T> struct chz_is_short { static constexpr bool value = false; };
template <> struct chz_is_short<chz_sc16> { static constexpr bool value = true; };
__device__ __forceinline__ cf2 chz_cvt(float2 s) { return (cf2){ s.x, s.y }; }
__device__ __forceinline__ cf2 chz_cvt(chz_sc16 s) { return (cf2){ (float)s.x, (float)s.y }; }
// The 8-bit wire formats of the translate seams and of the wideband seam's _as entry points (include/amps_recc.h,
// AMPS_RECC_SAMPLES_SC8 / _CU8), in the same style: two bytes per sample, I first.  xl_cvt is their one definition -- cu8 is offset
// binary, (float)i - 127.5f, 9 significant bits -- and chz_cvt hands its result to the filter bank.
struct alignas(2) xl_sc8 { int8_t x, y; };
struct alignas(2) xl_cu8 { uint8_t x, y; };
__device__ __forceinline__ float2 xl_cvt(xl_sc8 s) { return make_float2((float)s.x, (float)s.y); }
__device__ __forceinline__ float2 xl_cvt(xl_cu8 s) { return make_float2((float)s.x - 127.5f, (float)s.y - 127.5f); }
template <> struct chz_is_short<xl_sc8> { static constexpr bool value = true; };
template <> struct chz_is_short<xl_cu8> { static constexpr bool value = true; };
__device__ __forceinline__ cf2 chz_cvt(xl_sc8 s) { const float2 f = xl_cvt(s); return (cf2){ f.x, f.y }; }
__device__ __forceinline__ cf2 chz_cvt(xl_cu8 s) { const float2 f = xl_cvt(s); return (cf2){ f.x, f.y }; }
// The one list of sample formats (AMPS_RECC_SAMPLES_*): calls f with a value of the format's sample type -- a tag, only its type
// matters -- and returns what f returns; a value-initialised result (0, nullptr) for a format there is none for.  A new format is a
// `case` here and a chz_cvt above.
template <class F> inline auto chz_with_sample_type(int format, F &&f) -> decltype(f(float2{}))
{
    switch (format) {
    case AMPS_RECC_SAMPLES_FC32: return f(float2{});
    case AMPS_RECC_SAMPLES_SC16: return f(chz_sc16{});
    case AMPS_RECC_SAMPLES_SC8: return f(xl_sc8{});
    case AMPS_RECC_SAMPLES_CU8: return f(xl_cu8{});
    default: return {};
    }
}
// bytes of one sample of a format; 0: no such format
inline size_t chz_sample_bytes(int format) { return chz_with_sample_type(format, [](auto t) { return sizeof(t); }); }
// Buffer resource (V#) of the fast loader (round 6).  The fold role's prefetch used `global_load_dwordx2 v, v_off, s[base:base+1]` with
// a 64-bit scalar base per frame: clamp the frame index to the block, multiply, subtract, shift, add with carry -- nine scalar
// instructions per frame and two more per chunk, ~65 per half-step in the wave whose instruction count IS the kernel's critical path
// (a wave issues one instruction per slot, scalar or vector).  A raw buffer load takes a 32-bit scalar byte offset (+ a 12-bit
// immediate) against ONE descriptor per workgroup, and the hardware's range check (num_records) replaces the clamp: a prefetch that
// runs past the end of the block returns zeros nobody folds.  One s_add per pair of 2 KB chunks.
typedef int chz_rsrc_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ chz_rsrc_t chz_make_rsrc(const void *base, uint64_t bytes)
{
    const uint64_t a = (uint64_t)base;
    const uint32_t n = bytes > 0xffffffffull ? 0xffffffffu : (uint32_t)bytes;
    chz_rsrc_t r;
    r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    r.y = __builtin_amdgcn_readfirstlane((int)(uint32_t)((a >> 32) & 0xffffu));          // stride 0: a raw buffer, offsets and num_records in bytes
    r.z = __builtin_amdgcn_readfirstlane((int)n);
    r.w = 0x00020000;                                                                   // gfx9 family: DATA_FORMAT = 32 (untyped loads ignore it), type = buffer
    return r;
}

// Packed fp32 with operand modifiers.  hipcc materialises every swap / negate / broadcast of a packed operand with v_mov /
// v_xor and keeps broadcast constants as duplicated register PAIRS (the 32 fold coefficients cost 64 VGPRs, the six pass
// twiddles 24); the VOP3P modifiers do all of that for free, so the few shapes the pipeline needs are written as single
// instructions.  (The compiler treats an inline-asm producer conservatively for the gfx950 forwarding hazard and inserts
// the wait state itself.)  Every form computes exactly the IEEE operations of the plain expression next to it.
//
// (a.x b.x - a.y b.y, a.y b.x + a.x b.y):  m = (a.y * -b.y, a.x * b.y);  r = a * (b.x, b.x) + m
__device__ __forceinline__ cf2 cmul(cf2 a, cf2 b)
{
    cf2 m, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1] neg_lo:[0,1]" : "=v"(m) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(m));
    return r;
}
// the same with a wave-uniform twiddle held in an SGPR pair (the W16 constants of the radix-16 pass)
__device__ __forceinline__ cf2 cmul_s(cf2 a, cf2 b)
{
    cf2 m, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1] neg_lo:[0,1]" : "=v"(m) : "v"(a), "s"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(b), "v"(m));
    return r;
}
__device__ __forceinline__ cf2 mul_mi(cf2 a) { return (cf2){ a.y, -a.x }; }   // a * (-i)
// v + (-i) d = (v.x + d.y, v.y - d.x)   and   v - (-i) d = (v.x - d.y, v.y + d.x)
__device__ __forceinline__ cf2 add_mi(cf2 v, cf2 d)
{
    cf2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(v), "v"(d));
    return r;
}
__device__ __forceinline__ cf2 sub_mi(cf2 v, cf2 d)
{
    cf2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(v), "v"(d));
    return r;
}

// ---- frame geometry ----
// A half-batch = four frames (what the fold role produces per time step); a frame buffer holds one 1024-point frame.
constexpr int CHZ_BATCH = 4;
constexpr int CHZ_FB = CHZ_M + CHZ_M / 16;                     // padded frame buffer, cf2 elements
constexpr int CHZ_FBF = 2 * CHZ_FB;                            // ... in floats
constexpr int CHZ_SLOTS = 4;                                     // half-batches in flight
constexpr int CHZ_PREROLL = 8;                                   // frames re-run in front of a workgroup's range (two half-batches)
constexpr int CHZ12_IQ = -1;                                     // MODE: write the channel-major block; >= 0: AMPS_SLICER_* fused behind the FFT

} // namespace amps
