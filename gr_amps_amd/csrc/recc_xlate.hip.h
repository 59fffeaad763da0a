// recc_xlate.hip.h -- the front filter of grc/recctest.grc on gfx950, in two forms behind one host state:
// freq_xlating_fir_filter_ccc (grc/recctest.grc:889-937) with firdes.low_pass taps (:115-155): translate the
// channel at `center_hz` to DC, low-pass, decimate by D.  It stands in front of the fused IQ seam for the
// ".raw" fc32 400 ksps captures the reference's test flow graph reads (grc/recctest.grc:591).
//   per-row form (xlate_fir_kernel):   C input rows, one centre for all of them, C output rows;
//   shared form (xlate_shared_kernel): ONE input row (a modest SDR tuned to a system's control channels: a few hundred ksps
//                                      holding many 30 kHz channels), C centres, C output rows.
//
// The reference block multiplies by COMPLEX composite taps h[i] e^{j i phi} and then by a running rotator
// (4 real MACs per tap, rotator renormalised every 512 outputs).  Algebraically
//     y[k] = e^{-j phi D k} sum_i h[i] e^{j phi i} x[Dk - i] = sum_i h[i] z[Dk - i],   z[n] = x[n] e^{-j phi n}
// so a kernel mixes each input sample ONCE on its way into LDS (phase from an exact 64-bit phase
// accumulator evaluated per sample: no rotator drift, any push boundary gives the same bits) and then runs a REAL-tap FIR on complex
// data: one v_pk_fma per tap.  A lane produces 8/D adjacent outputs, so consecutive taps reuse the same LDS
// words (14 ds_read_b64 per 32 v_pk_fma at D = 2); the LDS window is padded by one sample per eight so that the
// lane stride of 8 samples is conflict free and the pad term of the address is wave-uniform (scalar) arithmetic.
//
// The arithmetic per output sample is written ONCE, in xl_window / xl_mix / xl_fir_store, and both kernels call it: the phasor of a
// sample comes from its ABSOLUTE index through xl_phasor, one fp32 cmul per staged sample, one fma chain over the zero-padded real
// taps in ascending tap order.  Row c of the shared form is therefore bit for bit what the per-row form gives a one-channel handle
// configured with centre c: the identity include/amps_recc.h defines the shared form by and the tests hold it to, and the reason
// nothing is "optimised" across channels in the float domain.  The two kernels stay two: they differ in what a workgroup stages.
//
// Per-row form: mixes while it stages, one workgroup per (tile, row); 31 808 bytes of LDS, 5 waves per SIMD, 1024 padded taps.
// This is the file-tool path (one or a few channels); the 832-channel front end is the polyphase channelizer.
//
// Shared form: STAGED.  The grid is (input tiles, channel groups).  A workgroup reads its raw tile plus the filter history from HBM /
// the carry ONCE into LDS and then, for each channel of its group: mixes the raw window into the padded window, barrier, FIR,
// store, barrier.  The raw tile is read once per group instead of once per channel, and one launch serves all channels.  The host
// picks the group size (xlate_shared_cpg) so that the grid has a few thousand workgroups where the block allows it -- balance over
// the CUs matters more than the re-read of the raw tile, which comes from L2 (measured) -- and one group of all
// channels only for very long blocks.  D = 8 (one output per lane) exists in this form only: 1.6 Msps at 10 samples per symbol, where
// the flow graph's filter spec gives 1195 taps -- hence XLS_MAX_TAPS = 1280.  Static LDS: raw 26 624 + mixed 30 016 + taps 5 120 =
// 61 760 bytes of the 65 536 one workgroup may own statically, 2 waves per SIMD.
//
// Shared form, wide (xlate_shared_wide_kernel): the decimations that do not divide 8 -- 5, 6, 10, 12, 16, 20, the rates SDRs deliver
// (1.0 ... 3.2 Msps, up to 2400 padded taps).  A tile is 256 OUTPUTS, one per lane, D is a kernel argument, one workgroup per (tile,
// channel) mixes straight from memory.  The mixed window is kept by PHASE: sample n at row n mod D, column n / D, so the lanes of a
// wave, which want samples D apart, read consecutive 8-byte words.  70 240 bytes of LDS, 2 workgroups per CU.
//
// Shared form, rational (xlate_shared_rational_kernel): resampling by L / M for the rates no integer decimation serves (2.048 Msps
// x 5/64, 2.5 Msps x 2/25, ...).  The polyphase resampler: output k sits at input q_k = floor(k M / L) and uses the
// taps of phase p_k = (k M) mod L.  The outputs of one residue k mod L are an integer decimation by M with ONE tap set, so a
// workgroup is L interleaved copies of the wide kernel's FIR: wave r owns residue r, the window is kept by phase mod M as above,
// and the L tap sets sit in LDS beside it.  L, M and the row length are kernel arguments; 80 KB of LDS, 2 workgroups per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <vector>
#include "amps_recc.h"              // AMPS_RECC_SAMPLES_*
#include "recc_chz_common.hip.h"    // cf2, cmul, chz_sc16
#include "recc_devmem.hip.h"
#include "recc_xlate_steps.h"
#include "recc_firdes.h"            // xlate_ntaps, xlate_design_taps

namespace amps {

constexpr int XL_TILE = 2048;        // input samples per workgroup (256 lanes x 8)
constexpr int XL_MAX_TAPS = 1024;    // padded tap count limit of xlate_fir_kernel
constexpr int XLS_MAX_TAPS = 1280;   // padded tap count limit of xlate_shared_kernel
constexpr int XLW_OUT = 256;         // outputs per workgroup of xlate_shared_wide_kernel (one per lane)
constexpr int XLW_MAX_TAPS = 2400;   // its padded tap count limit: the flow graph's filter spec at 3.2 Msps gives 2391
constexpr int XLW_MAX_D = 20;        // its largest decimation
// its mixed window: D rows (phases) of xlw_row(D) samples, and D xlw_row(D) < D (XLW_OUT + 3) + XLW_MAX_TAPS for every D
constexpr int XLW_ZS = XLW_MAX_D * (XLW_OUT + 3) + XLW_MAX_TAPS;
// The decimations of the wide kernel: the shared form only, D as a kernel argument, tiles of XLW_OUT outputs.
__host__ __device__ constexpr bool xlate_is_wide(uint32_t D) { return D == 5 || D == 6 || D == 10 || D == 12 || D == 16 || D == 20; }

// The block's sample types (include/amps_recc.h, AMPS_RECC_SAMPLES_*): float2 for fc32, and three PODs in the style of chz_sc16 for
// the integer wire formats, read IN PLACE: one dword (sc16) or one 16-bit load (sc8, cu8) per lane and sample, consecutive lanes on
// consecutive samples.  An integer form is DEFINED as the fc32 form on the plainly converted block, and every conversion below is
// exact in binary32 (cu8: (float)i is exact and i - 127.5 has 9 significant bits), so converting where the sample is fetched --
// xl_window, the one fetch of each kernel -- leaves every later operation on the bits it has in the fc32 form.  xl_sc8, xl_cu8 and
// their xl_cvt live in recc_chz_common.hip.h, which the wideband seam's narrow banks share.
using xl_sc16 = chz_sc16;
__device__ __forceinline__ float2 xl_cvt(float2 s) { return s; }
__device__ __forceinline__ float2 xl_cvt(xl_sc16 s) { return make_float2((float)s.x, (float)s.y); }

struct XlateArgs {
    const void *block;       // [rows][ld_in] new samples of the kernel's sample type; rows = C (per-row form) or 1 (shared form)
    const float2 *carry;     // [rows][carry_cap]: hist samples of history, then the leftover (< D) unconsumed samples
    const float *taps;       // [ntp], zero padded to a multiple of 8
    const uint64_t *steps;   // [C]: center_hz[c] / rate_hz as a 0.64 fixed-point fraction of a turn
    float2 *out;             // [C][ld_out]
    uint64_t ld_in, ld_out;
    uint64_t n_abs0;         // absolute input index of the first unconsumed sample (virtual index v = hist)
    uint32_t carry_cap, carry_len, hist, nsamp, nout, ntp, C;
    union {
        uint32_t cpg;        // shared form, staged: channels per workgroup (blockIdx.y = group)
        uint32_t D;          // shared form, wide: the decimation, which that kernel takes as an argument (a workgroup per channel)
    };
};

__host__ __device__ constexpr int xl_pad(int n) { return n + (n >> 3); }

// e^{-j 2 pi frac(n * step)}: the top 24 bits of the wrapped product are exact in fp32
__device__ __forceinline__ cf2 xl_phasor(uint64_t turns)
{
    float sn, cs;
    sincospif(-(float)(uint32_t)(turns >> 40) * 0x1p-23f, &sn, &cs);   // argument in half-turns, exact: no Payne-Hanek path
    return (cf2){ cs, sn };
}

// sample v of one input row's virtual stream: its carry (fc32 whatever the pushes were), then its block converted, zero beyond
template <typename T>
__device__ __forceinline__ float2 xl_window(const XlateArgs &a, const float2 *car, const T *blk, int64_t v)
{
    if (v < (int64_t)a.carry_len) return car[v];
    if (v < (int64_t)a.carry_len + a.nsamp) return xl_cvt(blk[v - a.carry_len]);
    return make_float2(0.f, 0.f);
}

// the mix of the sample with absolute index nabs: the phasor is evaluated per sample from the absolute index (not a running
// rotation), so a sample is mixed to the same bits whatever tile, push or handle it lands in
__device__ __forceinline__ cf2 xl_mix(float2 s, uint64_t nabs, uint64_t step)
{
    return cmul((cf2){ s.x, s.y }, xl_phasor(nabs * step));
}

// the FIR over the mixed, padded window zs (tile-local sample n at zs[xl_pad(n)]) and the store of lane t's 8/D outputs k0 + ..
template <int D>
__device__ __forceinline__ void xl_fir_store(const cf2 *zs, const float *hs, int t, int H, int ntp, float2 *out_row, uint32_t k0, uint32_t nout)
{
    constexpr int OPT = 8 / D;                                   // outputs per lane
    cf2 acc[OPT];
#pragma unroll
    for (int j = 0; j < OPT; j++) acc[j] = (cf2){ 0.f, 0.f };
    // tile-local sample of (output j, tap i+e) = 8t + u, u = (H - 7 - i) + (7 + D j - e): H - 7 - i is a multiple of 8,
    // so xl_pad(8t + u) = 9t + 9 (H - 7 - i)/8 + xl_pad(7 + D j - e) -- a moving base plus compile-time offsets
    const cf2 *zp = zs + 9 * t + 9 * ((H - 7) >> 3);
    for (int i = 0; i < ntp; i += 8, zp -= 9) {                  // ascending tap order: the summation order of the spec
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float h = hs[i + e];
#pragma unroll
            for (int j = 0; j < OPT; j++)
                acc[j] = __builtin_elementwise_fma(zp[xl_pad(7 + D * j - e)], (cf2){ h, h }, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < OPT; j++) {
        const uint32_t k = k0 + OPT * t + j;
        if (k < nout) out_row[k] = make_float2(acc[j].x, acc[j].y);
    }
}

template <int D, typename T>
__global__ __launch_bounds__(256) void xlate_fir_kernel(XlateArgs a)
{
    __shared__ cf2 zs[xl_pad(XL_TILE + XL_MAX_TAPS) + 8];
    __shared__ float hs[XL_MAX_TAPS];
    const int t = threadIdx.x;
    const uint32_t c = blockIdx.y;
    const uint32_t k0 = blockIdx.x * (XL_TILE / D);
    const int H = (int)a.hist;                                   // = ntp - 1
    const int ntp = (int)a.ntp;
    const T *blk = (const T *)a.block + (uint64_t)c * a.ld_in;
    const float2 *car = a.carry + (uint64_t)c * a.carry_cap;
    const int64_t v0 = (int64_t)D * k0;
    const uint64_t nabs0 = a.n_abs0 + (uint64_t)(v0 - H);        // wraps consistently for the (zero) pre-stream history
    const uint64_t step = a.steps[c];

    for (int i = t; i < ntp; i += 256) hs[i] = a.taps[i];
    // stage + mix: tile-local sample n <-> virtual index v = D*k0 + n;  lane t takes n = t, t+256, ...
    for (int n = t; n < XL_TILE + H; n += 256)
        zs[xl_pad(n)] = xl_mix(xl_window(a, car, blk, v0 + n), nabs0 + (uint64_t)n, step);
    __syncthreads();
    xl_fir_store<D>(zs, hs, t, H, ntp, a.out + (uint64_t)c * a.ld_out, k0, a.nout);
}

template <int D, typename T>
__global__ __launch_bounds__(256) void xlate_shared_kernel(XlateArgs a)
{
    __shared__ float2 xs[XL_TILE + XLS_MAX_TAPS];                // the raw window, staged once (fc32 for every sample type)
    __shared__ cf2 zs[xl_pad(XL_TILE + XLS_MAX_TAPS) + 8];       // the window mixed for the channel in hand
    __shared__ float hs[XLS_MAX_TAPS];
    static_assert(sizeof(float2) * (XL_TILE + XLS_MAX_TAPS) + sizeof(cf2) * (xl_pad(XL_TILE + XLS_MAX_TAPS) + 8) + sizeof(float) * XLS_MAX_TAPS <= 65536,
                  "static LDS of one workgroup");
    const int t = threadIdx.x;
    const uint32_t k0 = blockIdx.x * (XL_TILE / D);
    const int H = (int)a.hist;                                   // = ntp - 1
    const int ntp = (int)a.ntp;
    const int64_t v0 = (int64_t)D * k0;
    const uint64_t nabs0 = a.n_abs0 + (uint64_t)(v0 - H);        // wraps consistently for the (zero) pre-stream history

    for (int i = t; i < ntp; i += 256) hs[i] = a.taps[i];
    // stage: tile-local sample n <-> virtual index v = D*k0 + n;  lane t takes n = t, t+256, ...
    for (int n = t; n < XL_TILE + H; n += 256) xs[n] = xl_window(a, a.carry, (const T *)a.block, v0 + n);
    __syncthreads();

    const uint32_t c_end = min(a.C, (blockIdx.y + 1) * a.cpg);
    for (uint32_t c = blockIdx.y * a.cpg; c < c_end; c++) {
        const uint64_t step = a.steps[c];
        for (int n = t; n < XL_TILE + H; n += 256) zs[xl_pad(n)] = xl_mix(xs[n], nabs0 + (uint64_t)n, step);
        __syncthreads();
        xl_fir_store<D>(zs, hs, t, H, ntp, a.out + (uint64_t)c * a.ld_out, k0, a.nout);
        __syncthreads();                                         // the next channel overwrites the mixed window
    }
}

// row length of the wide kernel's phase-major window at decimation D: the columns an output tile can touch at the tap limit
// (XLW_OUT - 1 + ceil(XLW_MAX_TAPS / D)) and one more, made odd so that the D rows start on different banks (the stores of consecutive
// samples go to consecutive rows).  It depends on D alone, so the FIR's LDS offsets are compile-time constants per decimation.
__host__ __device__ constexpr int xlw_row(int D) { return (XLW_OUT + (XLW_MAX_TAPS + D - 1) / D) | 1; }

// lane t's output from the phase-major window: zp = zs + t, (output t, tap i) at zp[r L + b] with H - i = D b + r.  Ascending taps
// walk r downwards through column b (the head: the taps above the last whole column), then through whole columns towards column 0.
template <int D>
__device__ __forceinline__ cf2 xlw_fir(const cf2 *zp, const float *hs, int H, int ntp)
{
    constexpr int L = xlw_row(D);
    static_assert(D * L <= XLW_ZS, "the window of this decimation");
    cf2 acc = (cf2){ 0.f, 0.f };
    const cf2 *col = zp + H / D;
    int i = 0;
    for (int r = H % D; r >= 0; r--, i++) {
        const float h = hs[i];
        acc = __builtin_elementwise_fma(col[r * L], (cf2){ h, h }, acc);
    }
    for (col--; i < ntp; i += D, col--) {                        // ntp - i is a multiple of D here
#pragma unroll
        for (int e = 0; e < D; e++) {
            const float h = hs[i + e];
            acc = __builtin_elementwise_fma(col[(D - 1 - e) * L], (cf2){ h, h }, acc);
        }
    }
    return acc;
}

// The shared form for the decimations that do not divide 8.  One workgroup per (tile of XLW_OUT outputs, channel); lane t owns output
// k0 + t.  Tile-local sample n <-> virtual index v = D*k0 + n as above; (output m, tap i) is sample D m + (H - i).  The window is
// stored by phase, sample n at zs[(n % D) * L + n / D]: with H - i = D b + r, lane t reads zs[r L + b + t] -- the lanes of a wave
// on consecutive words, whatever D is, and (r, b) wave-uniform.  D is a kernel argument: the staging takes it as it comes, the FIR
// is unrolled once per decimation inside the one kernel (four instantiations, one per sample type).
template <typename T>
__global__ __launch_bounds__(256) void xlate_shared_wide_kernel(XlateArgs a)
{
    __shared__ cf2 zs[XLW_ZS];
    __shared__ float hs[XLW_MAX_TAPS];
    static_assert(sizeof(cf2) * XLW_ZS + sizeof(float) * XLW_MAX_TAPS <= 80 * 1024, "two workgroups per CU");
    const int t = threadIdx.x;
    const uint32_t c = blockIdx.y;
    const uint32_t k0 = blockIdx.x * XLW_OUT;
    const int D = (int)a.D;
    const int H = (int)a.hist;                                   // = ntp - 1
    const int ntp = (int)a.ntp;
    if (!xlate_is_wide(a.D) || ntp < 1 || ntp > XLW_MAX_TAPS) return;   // the host's limits (xlate_max_taps), held here too
    const int L = xlw_row(D);
    const int64_t v0 = (int64_t)D * k0;
    const uint64_t nabs0 = a.n_abs0 + (uint64_t)(v0 - H);        // wraps consistently for the (zero) pre-stream history
    const uint64_t step = a.steps[c];

    for (int i = t; i < ntp; i += 256) hs[i] = a.taps[i];
    const int W = D * (XLW_OUT - 1) + ntp;                       // the samples the tile's outputs read
    for (int n = t; n < W; n += 256) {
        const int col = n / D;
        zs[(n - col * D) * L + col] = xl_mix(xl_window(a, a.carry, (const T *)a.block, v0 + n), nabs0 + (uint64_t)n, step);
    }
    __syncthreads();

    cf2 acc;
    switch (D) {
    case 5: acc = xlw_fir<5>(zs + t, hs, H, ntp); break;
    case 6: acc = xlw_fir<6>(zs + t, hs, H, ntp); break;
    case 10: acc = xlw_fir<10>(zs + t, hs, H, ntp); break;
    case 12: acc = xlw_fir<12>(zs + t, hs, H, ntp); break;
    case 16: acc = xlw_fir<16>(zs + t, hs, H, ntp); break;
    default: acc = xlw_fir<20>(zs + t, hs, H, ntp); break;
    }
    const uint32_t k = k0 + t;
    if (k < a.nout) a.out[(uint64_t)c * a.ld_out + k] = make_float2(acc.x, acc.y);
}

// ---- the rational form: resampling by L / M
constexpr int XLR_MIN_L = 2, XLR_MAX_L = 5;   // interpolations (L = 1 is the integer forms above)
constexpr int XLR_MAX_M = 64;                 // largest decimation
constexpr int XLR_MAX_TAPS = 2400;            // padded taps PER PHASE
constexpr int XLR_MAX_WAVES = 5;              // waves of a workgroup: L residues x S sub-tiles of 64 L outputs
constexpr int XLR_LDS_BYTES = 80 * 1024;      // the L tap sets, then the mixed window
__host__ __device__ constexpr uint32_t xlr_gcd(uint32_t a, uint32_t b) { return b == 0 ? a : xlr_gcd(b, a % b); }
// sub-tiles of a workgroup: as many as keep it within XLR_MAX_WAVES waves (two at L = 2, else one)
__host__ __device__ constexpr int xlr_subtiles(int L) { return XLR_MAX_WAVES / L; }
// row length of the phase-major window (M rows): the columns that H + 64 S M staged samples reach, made odd as xlw_row is
__host__ __device__ constexpr int xlr_row(int M, int ntp, int S) { return (64 * S + (ntp - 1 + M - 1) / M) | 1; }
__host__ __device__ constexpr int64_t xlr_lds_bytes(int L, int M, int ntp, int S) { return (int64_t)sizeof(float) * L * ntp + (int64_t)sizeof(cf2) * M * xlr_row(M, ntp, S); }
// The limits of the rational kernel, in this one place: the host asks before it configures (xlate_resample_admit, xlate_create) and
// the kernel asks again at its top.  0, -EINVAL (no such ratio) or -E2BIG (taps per phase, or tap sets + window beyond the LDS).
__host__ __device__ constexpr int xlr_limits(uint32_t L, uint32_t M, uint32_t ntp, uint32_t S)
{
    if (L < (uint32_t)XLR_MIN_L || L > (uint32_t)XLR_MAX_L || M <= L || M > (uint32_t)XLR_MAX_M || xlr_gcd(L, M) != 1) return -EINVAL;
    if (S < 1 || L * S > (uint32_t)XLR_MAX_WAVES || ntp < 8 || (ntp & 7)) return -EINVAL;
    if (ntp > (uint32_t)XLR_MAX_TAPS || xlr_lds_bytes((int)L, (int)M, (int)ntp, (int)S) > XLR_LDS_BYTES) return -E2BIG;
    return 0;
}
// sub-tiles the host launches with: the most the LDS holds
__host__ __device__ constexpr uint32_t xlr_pick_subtiles(uint32_t L, uint32_t M, uint32_t ntp)
{
    uint32_t S = (uint32_t)xlr_subtiles((int)L);
    while (S > 1 && xlr_limits(L, M, ntp, S)) S--;
    return S;
}

struct XlateRationalArgs : XlateArgs {   // block, carry, steps, out, ld_*, n_abs0, carry_*, hist, nsamp, nout, ntp, C as above; D unused
    uint64_t k_abs0;         // absolute index of this push's first output
    uint32_t L, M;           // the stream is resampled by L / M; taps is [L][ntp], phase p at taps + p ntp
    uint32_t S, RL;          // sub-tiles per workgroup (blockDim = 64 L S) and the window's row length, xlr_row(M, ntp, S)
};

// One workgroup per (tile of 64 L S outputs, channel).  K0 = the tile's first absolute output, K0 M = L Q0 + P0.  Wave w = L s + r
// (sub-tile s, residue r), lane j owns output K0 + 64 L s + L j + r, which sits at input Q0 + (64 s + j) M + off with
// off = floor((P0 + r M) / L) < M and uses phase p = (P0 + r M) mod L: both wave-uniform.  Tile-local sample n <-> absolute input
// Q0 - H + n, kept at zs[(n % M) RL + n / M]; (that output, tap i) is sample (64 s + j) M + H + off - i: with H + off - i = M b + r',
// zs[r' RL + b + 64 s + j] -- the lanes of a wave on consecutive words.  Ascending taps walk r' downwards through column b, then
// through whole columns towards column 0, where they end at r' = off.
template <typename T>
__global__ __launch_bounds__(64 * XLR_MAX_WAVES) void xlate_shared_rational_kernel(XlateRationalArgs a)
{
    __shared__ float4 lds[XLR_LDS_BYTES / sizeof(float4)];
    const int L = (int)a.L, M = (int)a.M, S = (int)a.S, RL = (int)a.RL;
    const int H = (int)a.hist;                                   // = ntp - 1
    const int ntp = (int)a.ntp;
    // the host's limits (xlr_limits), held here too
    if (xlr_limits(a.L, a.M, a.ntp, a.S) || RL != xlr_row(M, ntp, S) || (int)blockDim.x != 64 * L * S || H != ntp - 1) return;
    float *hs = (float *)lds;
    cf2 *zs = (cf2 *)(hs + L * ntp);                              // L ntp is a multiple of 8 floats
    const int t = threadIdx.x, BD = 64 * L * S;
    const uint32_t c = blockIdx.y;
    const uint64_t KM = (a.k_abs0 + (uint64_t)blockIdx.x * (uint32_t)BD) * (uint32_t)M;
    const uint64_t Q0 = KM / (uint32_t)L;
    const int P0 = (int)(KM - Q0 * (uint32_t)L);
    const int64_t v0 = (int64_t)(Q0 - a.n_abs0);                  // virtual index of tile-local sample 0: Q0 >= n_abs0, see xlate_run
    const uint64_t nabs0 = Q0 - (uint64_t)H;                      // wraps consistently for the (zero) pre-stream history
    const uint64_t step = a.steps[c];

    for (int i = t; i < L * ntp; i += BD) hs[i] = a.taps[i];
    const int W = H + 64 * S * M;                                // the samples the tile's outputs can read, whatever P0 is
    const int dcol = BD / M, drow = BD - dcol * M;
    int col = t / M, row = t - col * M;
    for (int n = t; n < W; n += BD) {
        zs[row * RL + col] = xl_mix(xl_window(a, a.carry, (const T *)a.block, v0 + n), nabs0 + (uint64_t)n, step);
        row += drow; col += dcol;
        if (row >= M) { row -= M; col++; }
    }
    __syncthreads();

    const int w = __builtin_amdgcn_readfirstlane(t >> 6), j = t & 63;
    const int s = w / L, r = w - s * L;
    const int off = (P0 + r * M) / L, p = (P0 + r * M) - off * L;
    const float *h = hs + p * ntp;
    const cf2 *zl = zs + 64 * s + j;
    const int b0 = (H + off) / M, r0 = (H + off) - b0 * M;
    cf2 acc = (cf2){ 0.f, 0.f };
    int i = 0;
    for (int b = b0; b >= 0; b--) {                              // ascending tap order: the summation order of the spec
        const int hi = b == b0 ? r0 : M - 1, lo = b == 0 ? off : 0;
        const cf2 *zp = zl + hi * RL + b;
#pragma unroll 8
        for (int e = hi; e >= lo; e--, i++, zp -= RL) {
            const float hv = h[i];
            acc = __builtin_elementwise_fma(*zp, (cf2){ hv, hv }, acc);
        }
    }
    const uint64_t k = (uint64_t)blockIdx.x * (uint32_t)BD + (uint32_t)(L * (64 * s + j) + r);
    if (k < a.nout) a.out[(uint64_t)c * a.ld_out + k] = make_float2(acc.x, acc.y);
}

// carry_out[r][i] = virtual[r][consumed + i], i < new_len  (separate buffers: the ranges can overlap).  The carry is fc32: the samples
// taken from the block are converted here, which is what lets the sample type change from one push to the next.
template <typename T>
__global__ void xlate_carry_kernel(const void *block, uint64_t ld_in, const float2 *carry_in, float2 *carry_out,
                                   uint32_t carry_cap, uint32_t carry_len, uint32_t consumed, uint32_t new_len)
{
    const uint32_t c = blockIdx.y;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= new_len) return;
    const uint64_t v = (uint64_t)consumed + i;
    carry_out[(uint64_t)c * carry_cap + i] = v < carry_len ? carry_in[(uint64_t)c * carry_cap + v] : xl_cvt(((const T *)block)[(uint64_t)c * ld_in + (v - carry_len)]);
}

// What the two forms differ in on the host: the kernel for a decimation (none: the form does not have it) and the padded tap limit.
// What the sample formats differ in: the kernels' sample type, its size, and nothing else.
typedef void (*xlate_kernel_t)(XlateArgs);
typedef void (*xlate_carry_kernel_t)(const void *, uint64_t, const float2 *, float2 *, uint32_t, uint32_t, uint32_t, uint32_t);
template <typename T> inline xlate_kernel_t xlate_kernel_of(bool shared, uint32_t D)
{
    switch (D) {
    case 1: return shared ? xlate_shared_kernel<1, T> : xlate_fir_kernel<1, T>;
    case 2: return shared ? xlate_shared_kernel<2, T> : xlate_fir_kernel<2, T>;
    case 4: return shared ? xlate_shared_kernel<4, T> : xlate_fir_kernel<4, T>;
    case 8: return shared ? xlate_shared_kernel<8, T> : nullptr;
    default: return shared && xlate_is_wide(D) ? xlate_shared_wide_kernel<T> : nullptr;
    }
}
inline xlate_kernel_t xlate_kernel_for(bool shared, uint32_t D, int format = AMPS_RECC_SAMPLES_FC32)
{
    switch (format) {
    case AMPS_RECC_SAMPLES_FC32: return xlate_kernel_of<float2>(shared, D);
    case AMPS_RECC_SAMPLES_SC16: return xlate_kernel_of<xl_sc16>(shared, D);
    case AMPS_RECC_SAMPLES_SC8: return xlate_kernel_of<xl_sc8>(shared, D);
    case AMPS_RECC_SAMPLES_CU8: return xlate_kernel_of<xl_cu8>(shared, D);
    default: return nullptr;
    }
}
inline xlate_carry_kernel_t xlate_carry_kernel_for(int format)
{
    switch (format) {
    case AMPS_RECC_SAMPLES_FC32: return xlate_carry_kernel<float2>;
    case AMPS_RECC_SAMPLES_SC16: return xlate_carry_kernel<xl_sc16>;
    case AMPS_RECC_SAMPLES_SC8: return xlate_carry_kernel<xl_sc8>;
    case AMPS_RECC_SAMPLES_CU8: return xlate_carry_kernel<xl_cu8>;
    default: return nullptr;
    }
}
// bytes of one sample of a format; 0: no such format
inline size_t xlate_sample_bytes(int format)
{
    return chz_sample_bytes(format);
}
inline uint32_t xlate_max_taps(bool shared, uint32_t D) { return !shared ? XL_MAX_TAPS : xlate_is_wide(D) ? XLW_MAX_TAPS : XLS_MAX_TAPS; }
typedef void (*xlate_rational_kernel_t)(XlateRationalArgs);
inline xlate_rational_kernel_t xlate_rational_kernel_for(int format)
{
    switch (format) {
    case AMPS_RECC_SAMPLES_FC32: return xlate_shared_rational_kernel<float2>;
    case AMPS_RECC_SAMPLES_SC16: return xlate_shared_rational_kernel<xl_sc16>;
    case AMPS_RECC_SAMPLES_SC8: return xlate_shared_rational_kernel<xl_sc8>;
    case AMPS_RECC_SAMPLES_CU8: return xlate_shared_rational_kernel<xl_cu8>;
    default: return nullptr;
    }
}

struct XlateState {
    bool enabled = false;
    bool shared = false;             // one input row for all channels, else one per channel
    uint32_t C = 0, rows = 0, D = 0, ntp = 0, hist = 0, carry_cap = 0, carry_len = 0, max_out = 0;
    uint32_t L = 1;                  // rational form: the stream is resampled by L / D and taps is [L][ntp]; 1: the integer forms
    int cur = 0;
    uint64_t n_abs = 0;
    uint64_t k_abs = 0;              // rational form: absolute index of the next output
    double rate_hz = 0.0;            // of the input stream: what xlate_retune turns new centres into steps by
    DevBuf<float> taps;
    DevBuf<uint64_t> steps;          // [C]
    DevBuf<float2> carry[2];         // [rows][carry_cap] (hist + D samples a row; hist + 1 of the rational form), double-buffered
    DevBuf<float2> out;              // [C][max_out]
    HostStage stage;                 // host-resident blocks: [rows][D * max_out / L]
};

// the filter design, xlate_ntaps and xlate_design_taps: recc_firdes.h (host arithmetic only, shared with the wideband seam's resampler)

// What a form accepts of a stream at rate_hz decimated by D for a handle of sps samples per symbol, in the order the configuration
// answers: a filter the design formula can make, a kernel for D and the symbol rate met (-EINVAL), the filter's length within that
// kernel's limit (-E2BIG).  *ntaps = the filter's length wherever the rates are numbers.  amps_recc_set_xlate[_shared] and
// amps_recc_xlate_shared_plan both ask here.
// The design divides by ntaps - 1 (the window) and firdes.low_pass itself refuses a cut-off beyond rate / 2: a width of 74 rate / 44
// (1.68 rate) or more gives one tap, 0 / 0 = NaN, so fewer than three taps and a cut-off above Nyquist are no filter.
inline int xlate_admit(bool shared, uint32_t D, uint32_t sps, double rate_hz, double cutoff_hz, double width_hz, uint32_t *ntaps)
{
    *ntaps = 0;
    if (!(rate_hz > 0.0) || !(width_hz > 0.0) || std::isinf(rate_hz)) return -EINVAL;
    *ntaps = (uint32_t)xlate_ntaps(rate_hz, width_hz);
    if (*ntaps < 3 || !(cutoff_hz > 0.0) || !(cutoff_hz <= 0.5 * rate_hz)) return -EINVAL;
    if (!xlate_kernel_for(shared, D)) return -EINVAL;
    // the filtered stream must arrive at the symbol rate the handle was built for
    const double out_rate = rate_hz / D;
    if (std::fabs(out_rate - 20e3 * sps) > 1e-6 * out_rate) return -EINVAL;
    return (*ntaps + 7) / 8 * 8 > xlate_max_taps(shared, D) ? -E2BIG : 0;
}

// The rational form's counterpart: a stream at rate_hz resampled by L / M.  The prototype is designed at the up-sampled rate L rate_hz;
// *ntaps_per_phase = ceil(its length / L) wherever the rates are numbers.  -EINVAL: no filter, no such ratio, the symbol rate not met;
// -E2BIG: xlr_limits.  amps_recc_set_xlate_resampled and amps_recc_xlate_resample_plan both ask here.
inline int xlate_resample_admit(uint32_t L, uint32_t M, uint32_t sps, double rate_hz, double cutoff_hz, double width_hz, uint32_t *ntaps_per_phase)
{
    *ntaps_per_phase = 0;
    if (!(rate_hz > 0.0) || !(width_hz > 0.0) || std::isinf(rate_hz)) return -EINVAL;
    if (L < (uint32_t)XLR_MIN_L || L > (uint32_t)XLR_MAX_L) return -EINVAL;
    const uint32_t ng = (uint32_t)xlate_ntaps(L * rate_hz, width_hz);
    *ntaps_per_phase = (ng + L - 1) / L;
    if (ng < 3 || !(cutoff_hz > 0.0) || !(cutoff_hz <= 0.5 * L * rate_hz)) return -EINVAL;
    const uint32_t ntp = (*ntaps_per_phase + 7) / 8 * 8;
    if (xlr_limits(L, M, 8, 1) == -EINVAL) return -EINVAL;
    // the resampled stream must arrive at the symbol rate the handle was built for
    const double out_rate = rate_hz * L / M;
    if (std::fabs(out_rate - 20e3 * sps) > 1e-6 * out_rate) return -EINVAL;
    return ng > 1000000u ? -E2BIG : xlr_limits(L, M, ntp, 1);
}

inline void xlate_destroy(XlateState &x) { x = XlateState{}; }

inline int xlate_reset(XlateState &x, hipStream_t s)
{
    if (!x.enabled) return 0;
    if (hipMemsetAsync(x.carry[0].get(), 0, sizeof(float2) * (size_t)x.rows * x.carry_cap, s) != hipSuccess) return -EIO;
    if (hipMemsetAsync(x.carry[1].get(), 0, sizeof(float2) * (size_t)x.rows * x.carry_cap, s) != hipSuccess) return -EIO;
    x.cur = 0; x.carry_len = x.hist; x.n_abs = 0; x.k_abs = 0;
    return 0;
}

// center_hz is [C] (per-row form: C times the same centre).  A configuration that is refused (-EINVAL, -E2BIG) leaves x as it was.
// L > 1: the rational form (shared, D = M), taps = the prototype at the up-sampled rate, split here into its L phases.
inline int xlate_create(XlateState &x, bool shared, uint32_t C, uint32_t D, uint32_t max_out, double rate_hz, const double *center_hz,
                        const std::vector<float> &taps, hipStream_t s, uint32_t L = 1)
{
    const bool rational = L != 1;
    if (rational ? !shared || xlr_limits(L, D, 8, 1) == -EINVAL : !xlate_kernel_for(shared, D)) return -EINVAL;
    if (C == 0 || !center_hz || taps.empty() || !(rate_hz > 0.0)) return -EINVAL;
    std::vector<uint64_t> steps(C);
    if (xlate_steps_from(rate_hz, center_hz, C, steps.data())) return -EINVAL;   // a centre beyond +-rate_hz, a NaN included
    if (taps.size() > 1000000u) return -E2BIG;
    const uint32_t ntp = (uint32_t)(((taps.size() + L - 1) / L + 7) / 8 * 8);   // per phase
    if (rational ? xlr_limits(L, D, ntp, 1) != 0 : ntp > xlate_max_taps(shared, D)) return -E2BIG;
    xlate_destroy(x);
    x.shared = shared; x.C = C; x.rows = shared ? 1 : C; x.D = D; x.L = L; x.ntp = ntp; x.hist = ntp - 1; x.max_out = max_out;
    x.rate_hz = rate_hz;
    // the rational form's next output never sits before the stream's end (xlate_run): its carry is the history alone
    x.carry_cap = rational ? ntp : ntp + D;
    std::vector<float> padded((size_t)L * ntp, 0.0f);             // phase p, tap i = taps[L i + p], zero beyond
    for (size_t i = 0; i < taps.size(); i++) padded[(i % L) * ntp + i / L] = taps[i];
    int rc = x.taps.alloc(padded.size()) | x.steps.alloc(C) | x.carry[0].alloc((size_t)x.rows * x.carry_cap) | x.carry[1].alloc((size_t)x.rows * x.carry_cap)
           | x.out.alloc((size_t)C * max_out);
    if (!rc && hipMemcpy(x.taps.get(), padded.data(), sizeof(float) * padded.size(), hipMemcpyHostToDevice) != hipSuccess) rc = -EIO;
    if (!rc && hipMemcpy(x.steps.get(), steps.data(), sizeof(uint64_t) * C, hipMemcpyHostToDevice) != hipSuccess) rc = -EIO;
    if (rc) { xlate_destroy(x); return rc; }
    x.enabled = true;
    return xlate_reset(x, s);
}

// Retune (amps_recc_retune_xlate): new steps for the configured form, everything else kept.  The steps travel as kernel arguments, a
// chunk a launch, so the update is ordered on the stream behind the kernels already queued, the host waits for nothing and no host
// buffer is read after the call.  The kernels in front read the old steps, those behind the new ones: a sample's phasor comes from
// its absolute index, so the stage then delivers what a stage created with these centres would.
struct XlateStepChunk { uint64_t v[128]; };
__global__ __launch_bounds__(128) void xlate_steps_store_kernel(uint64_t *steps, uint32_t first, uint32_t n, XlateStepChunk c)
{
    if (threadIdx.x < n) steps[first + threadIdx.x] = c.v[threadIdx.x];
}
inline int xlate_retune(XlateState &x, const double *center_hz, size_t n, hipStream_t s)
{
    if (!x.enabled) return -ENOSYS;
    std::vector<uint64_t> steps(x.C);
    if (int rc = xlate_retune_steps(x.shared, x.C, x.rate_hz, center_hz, n, steps.data())) return rc;
    for (uint32_t first = 0; first < x.C; first += 128) {
        XlateStepChunk c{};
        const uint32_t m = std::min<uint32_t>(128, x.C - first);
        std::copy(steps.begin() + first, steps.begin() + first + m, c.v);
        hipLaunchKernelGGL(xlate_steps_store_kernel, dim3(1), dim3(128), 0, s, x.steps.get(), first, m, c);
    }
    return hipGetLastError() != hipSuccess ? -EIO : 0;
}

// channels per workgroup of the shared form: as many groups of as few channels as it takes to reach WANT workgroups; one group (the
// raw tile read once) when the tiles alone are that many.  The output bits do not depend on it.
inline uint32_t xlate_shared_cpg(uint32_t C, uint64_t tiles)
{
    constexpr uint64_t WANT = 4096;                              // workgroups: sixteen per CU of a 256-CU device (measured: DESIGN.md 4.7b)
    const uint64_t groups = std::min<uint64_t>(C, std::max<uint64_t>(1, (WANT + tiles - 1) / tiles));
    return (uint32_t)((C + groups - 1) / groups);
}

// filter nsamp new samples per input row ([rows][ld] samples of `format`, host or device, read as they are); *out_iq is [C][*out_ld]
// device memory holding *nout samples per row
inline int xlate_run(XlateState &x, const void *iq, uint64_t ld, size_t nsamp, int format, int mem, hipStream_t s,
                     const float2 **out_iq, uint64_t *out_ld, uint32_t *nout)
{
    *out_iq = x.out.get(); *out_ld = x.max_out; *nout = 0;
    const size_t sz = xlate_sample_bytes(format);
    if (!sz) return -EINVAL;
    if (!x.enabled) return -ENOSYS;
    if (nsamp == 0) return 0;
    // the inputs max_out outputs take: D each, or D / L of the rational form (L = 1 otherwise)
    const uint64_t max_in = (uint64_t)x.D * x.max_out / x.L;
    if (nsamp > max_in) return -E2BIG;
    const bool rational = x.L != 1;
    const void *d = iq;
    if (mem == AMPS_MEM_HOST) {
        // the block travels in its own format, staged by the byte; the reserve is that of the largest fc32 block, which covers them all
        const uint8_t *db = nullptr;
        uint64_t ld_bytes = 0;
        if (int rc = x.stage.stage((const uint8_t *)iq, ld * sz, nsamp * sz, x.rows, sizeof(float2) * x.rows * max_in, &db, &ld_bytes)) return rc;
        d = db; ld = nsamp;
    }
    const uint64_t avail = (uint64_t)(x.carry_len - x.hist) + nsamp;
    // Rational form: after N inputs in all the stream has delivered the outputs k with floor(k D / L) <= N - 1, ceil(L N / D) of them.
    // The next output therefore sits at or beyond the stream's end: every input is consumed at once (n_abs = N), the carry is the
    // history alone, and output k's newest sample floor(k D / L) >= n_abs has the virtual index hist + floor(k D / L) - n_abs.
    const uint64_t n_out = rational ? ((x.n_abs + nsamp) * x.L + x.D - 1) / x.D - x.k_abs : avail / x.D;
    if (n_out > x.max_out) return -E2BIG;
    XlateRationalArgs a{};
    a.block = d; a.carry = x.carry[x.cur].get(); a.taps = x.taps.get(); a.steps = x.steps.get(); a.out = x.out.get(); a.ld_in = ld; a.ld_out = x.max_out;
    a.n_abs0 = x.n_abs; a.carry_cap = x.carry_cap; a.carry_len = x.carry_len; a.hist = x.hist;
    a.nsamp = (uint32_t)nsamp; a.nout = (uint32_t)n_out; a.ntp = x.ntp; a.C = x.C;
    if (n_out && rational) {
        // a tile is 64 L S outputs, a workgroup per (tile, channel) of as many threads
        a.k_abs0 = x.k_abs; a.L = x.L; a.M = x.D; a.S = xlr_pick_subtiles(x.L, x.D, x.ntp); a.RL = (uint32_t)xlr_row((int)x.D, (int)x.ntp, (int)a.S);
        const uint32_t per = 64 * a.L * a.S;
        hipLaunchKernelGGL(xlate_rational_kernel_for(format), dim3((uint32_t)((n_out + per - 1) / per), x.C), dim3(per), 0, s, a);
    } else if (n_out) {
        // a tile is XL_TILE inputs, or XLW_OUT outputs of the wide kernel; a workgroup per (tile, row) but for the staged shared form
        const bool wide = x.shared && xlate_is_wide(x.D);
        const uint64_t tiles = wide ? (n_out + XLW_OUT - 1) / XLW_OUT : (n_out * x.D + XL_TILE - 1) / XL_TILE;
        const uint32_t cpg = x.shared && !wide ? xlate_shared_cpg(x.C, tiles) : 1;
        if (wide) a.D = x.D; else a.cpg = cpg;
        hipLaunchKernelGGL(xlate_kernel_for(x.shared, x.D, format), dim3((uint32_t)tiles, (x.C + cpg - 1) / cpg), dim3(256), 0, s, (XlateArgs)a);
    }
    const uint32_t consumed = rational ? (uint32_t)nsamp : (uint32_t)(n_out * x.D);
    const uint32_t new_len = x.hist + (uint32_t)(avail - (uint64_t)consumed);
    hipLaunchKernelGGL(xlate_carry_kernel_for(format), dim3((new_len + 255) / 256, x.rows), dim3(256), 0, s, d, ld, x.carry[x.cur].get(), x.carry[x.cur ^ 1].get(),
                       x.carry_cap, x.carry_len, consumed, new_len);
    if (hipGetLastError() != hipSuccess) return -EIO;
    if (mem == AMPS_MEM_HOST) { if (int rc = x.stage.arm(s)) return rc; }
    x.cur ^= 1; x.carry_len = new_len; x.n_abs += consumed; x.k_abs += rational ? n_out : 0;
    *nout = (uint32_t)n_out;
    return 0;
}

} // namespace amps
