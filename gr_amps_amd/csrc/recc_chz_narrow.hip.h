// recc_chz_narrow.hip.h -- the filter bank of the wideband seam at M = 512, 256 and 128 branches (15.36, 7.68 and 3.84 Msps: the rates
// one SDR delivers), D = M / 2 or 3 M / 4.  The same weighted-overlap-add bank as recc_channelizer.hip.h defines at its top and
// oracle/channelizer.py models -- P = 8 taps per branch, frame m over samples [(m+1) D - 8 M, (m+1) D), the fold modulo M with the
// absolute phase reference n0 mod M, an M-point DFT -- in the two-kernel form only: the active bins leave as rows of the channel-major
// fc32 block, which the streaming kernel of the IQ seam takes from there (capture_run_iq), as in the unfused form of the 1024 bank.
//
// Mapping: a 256-thread workgroup owns FR consecutive frames for all M bins.
//   stage : the (FR - 1) D + 8 M input samples of its frames, carry first and block behind it, expanded to fc32 (chz_cvt), once in LDS
//   fold  : a thread keeps the eight taps h[p M + j] of its branch j in registers (two branches at M = 512) and folds a frame with
//           eight FMAs per branch out of LDS; the roll n0 mod M is an index offset of the store (FR is a multiple of the roll's
//           period -- 2 frames at D = M / 2, 4 at D = 3 M / 4 -- and so is every launch: a workgroup's frame f has roll ((f+1) D) mod M)
//   FFT   : all FR frames at once, Stockham passes in place over LDS: every thread reads its butterflies, the workgroup meets, every
//           thread writes.  512 = 8 x 8 x 8, 256 = 16 x 16, 128 = 16 x 8; twiddles from a table the host computed in double precision
//   store : thread -> (bin, frame) with the frame running fastest: a row leaves as one run of FR x 8 bytes
// A frame's arithmetic is a fixed sequence of operations on its own 8 M samples: it depends neither on how the stream was cut into
// pushes nor on which workgroup computes it.  No atomics, nothing handed from one workgroup to another.
//
// FR per geometry (LDS <= 80 KiB, so that two workgroups fit a CU) and the share of the input a launch reads a second time,
// 8 M / (FR D) -- the 8 M - D samples of history in front of a workgroup's first frame, which its neighbour stages too (from L2):
//   M = 512: D = 256: FR =  8, 2.00     D = 384: FR =  4, 2.67
//   M = 256: D = 128: FR = 16, 1.00     D = 192: FR = 16, 0.67
//   M = 128: D =  64: FR = 32, 0.50     D =  96: FR = 32, 0.33
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "recc_chz_common.hip.h"
#include "recc_chz_fft.hip.h"
#include "recc_xlate.hip.h"         // xl_mix: the mixing twins (amps_recc_set_wideband_shift)

namespace amps {

struct ChzNarrowArgs {
    const void *block;       // new wideband samples of this push: float2 or chz_sc16 (chz_narrow_kernel), xl_sc8 or xl_cu8 (chz_narrow_b8_kernel)
    const float2 *carry;     // [carry_len]: the hist = 8 M - D samples in front of frame 0, then what earlier pushes left over
    const float *taps;       // [8 M] prototype
    const float2 *twiddle;   // [M]: e^{-2 pi i k / M}
    float2 *out;             // [n_channels][ld] channel-major output of this push
    uint64_t ld;
    const uint16_t *bin2row; // [M]: row of FFT bin k in `out`, >= n_channels for a bin this handle does not decode
    uint32_t carry_len;
    uint32_t nsamp;          // new samples
    uint32_t nframes;        // frames this launch produces: a multiple of the roll's period
    uint32_t n_channels;
};

// The mixing twins' arguments (chz_narrow_mix_kernel, chz_grid10_mix_kernel): the bank's, untouched, and the mixer's behind them, by
// value with every launch -- a new shift needs no device write.
struct ChzMixArgs {
    ChzNarrowArgs bank;
    int64_t abs0;            // absolute wideband index of carry element 0: frames_done D - hist, negative in front of the stream
    uint64_t step;           // shift_hz / fs as a 0.64 fixed-point fraction of a turn per sample (xlate_steps_from)
};
// what a thread staged for carry-relative sample ci, mixed: x e^{-j 2 pi frac(n step)} with n the sample's absolute index, by xl_mix
// as the translate seams define it -- per sample, no running rotation, so the bits depend on nothing but the sample and n
__device__ __forceinline__ cf2 chz_mix_staged(cf2 v, const ChzMixArgs &m, uint64_t ci) { return xl_mix(make_float2(v.x, v.y), (uint64_t)m.abs0 + ci, m.step); }

__host__ __device__ constexpr bool chz_narrow_geometry(int M, int D) { return (M == 512 || M == 256 || M == 128) && (2 * D == M || 4 * D == 3 * M); }
// frames per workgroup
__host__ __device__ constexpr int chz_narrow_fr(int M, int D) { return M == 512 ? (2 * D == M ? 8 : 4) : M == 256 ? 16 : 32; }
// ... which the host reads from the bank table: its NARROW rows are exactly this header's geometries and frames per workgroup
constexpr bool chz_narrow_table_agrees()
{
    int n = 0;
    for (const ChzBank &b : CHZ_BANKS) {
        if (b.family != ChzFamily::NARROW) continue;
        for (int i = 0; i < 2; i++, n++)
            if (!chz_narrow_geometry((int)b.M, (int)b.decim[i]) || b.taps != 8u || (int)b.fr[i] != chz_narrow_fr((int)b.M, (int)b.decim[i])) return false;
    }
    return n == 6;
}
static_assert(chz_narrow_table_agrees(), "recc_chz_banks.h states the narrow banks as the kernels are built");
// LDS layout of a frame: element n at n + n / 32 (a store of stride 8 or 16 elements across lanes then walks the banks), frames S
// elements apart, S odd (the store phase reads one bin of consecutive frames across lanes)
__host__ __device__ constexpr int chz_narrow_pos(int n) { return n + (n >> 5); }
__host__ __device__ constexpr int chz_narrow_stride(int M) { return M + M / 32 + 1; }
__host__ __device__ constexpr int chz_narrow_stage(int M, int D) { return (chz_narrow_fr(M, D) - 1) * D + 8 * M; }
__host__ __device__ constexpr size_t chz_narrow_lds_bytes(int M, int D) { return sizeof(float2) * ((size_t)chz_narrow_stage(M, D) + (size_t)chz_narrow_fr(M, D) * chz_narrow_stride(M)); }

// DFT-R in place, natural order
__device__ __forceinline__ void chz_dft(cf2 (&v)[2]) { const cf2 a = v[0], b = v[1]; v[0] = a + b; v[1] = a - b; }
__device__ __forceinline__ void chz_dft(cf2 (&v)[4]) { dft4(v[0], v[1], v[2], v[3], v); }
// radix 5 (the banks of recc_chz_grid10.hip.h): sums and differences of the pairs (1, 4) and (2, 3), then X[k] and X[5 - k] share
// their real-coefficient half (cos 2 pi / 5, cos 4 pi / 5) and differ in the sign of -i times the other (sin 2 pi / 5, sin 4 pi / 5)
__device__ __forceinline__ void chz_dft(cf2 (&v)[5])
{
    constexpr float C1 = 0.30901699437494742f, C2 = -0.80901699437494742f, S1 = 0.95105651629515357f, S2 = 0.58778525229247313f;
    const cf2 t1 = v[1] + v[4], t2 = v[2] + v[3], t3 = v[1] - v[4], t4 = v[2] - v[3];
    const cf2 m1 = v[0] + C1 * t1 + C2 * t2, m2 = v[0] + C2 * t1 + C1 * t2;
    const cf2 n1 = S1 * t3 + S2 * t4, n2 = S2 * t3 - S1 * t4;
    v[0] = v[0] + t1 + t2;
    v[1] = add_mi(m1, n1); v[4] = sub_mi(m1, n1);
    v[2] = add_mi(m2, n2); v[3] = sub_mi(m2, n2);
}
__device__ __forceinline__ void chz_dft(cf2 (&v)[8])
{
    constexpr float R2 = 0.70710678118654752f;
    cf2 e[4], o[4];
    dft4(v[0], v[2], v[4], v[6], e);
    dft4(v[1], v[3], v[5], v[7], o);
    o[1] = cmul_s(o[1], (cf2){ R2, -R2 });                      // W8^1
    o[2] = mul_mi(o[2]);                                        // W8^2 = -i
    o[3] = cmul_s(o[3], (cf2){ -R2, -R2 });                     // W8^3
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = e[k] + o[k]; v[k + 4] = e[k] - o[k]; }
}
// 4 x DFT4 over a (s = 4a + b), twiddle W16^{bc}, 4 x DFT4 over b -> X[c + 4d]: the butterfly of chz_p2
__device__ __forceinline__ void chz_dft(cf2 (&u)[16])
{
    cf2 v[4][4];
#pragma unroll
    for (int b = 0; b < 4; b++) dft4(u[b], u[4 + b], u[8 + b], u[12 + b], v[b]);
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
    v[1][1] = cmul_s(v[1][1], (cf2){ C1, -S1 });
    v[1][2] = cmul_s(v[1][2], (cf2){ R2, -R2 });
    v[1][3] = cmul_s(v[1][3], (cf2){ S1, -C1 });
    v[2][1] = cmul_s(v[2][1], (cf2){ R2, -R2 });
    v[2][2] = mul_mi(v[2][2]);
    v[2][3] = cmul_s(v[2][3], (cf2){ -R2, -R2 });
    v[3][1] = cmul_s(v[3][1], (cf2){ S1, -C1 });
    v[3][2] = cmul_s(v[3][2], (cf2){ -R2, -R2 });
    v[3][3] = cmul_s(v[3][3], (cf2){ -C1, S1 });
#pragma unroll
    for (int c = 0; c < 4; c++) {
        cf2 X[4];
        dft4(v[0][c], v[1][c], v[2][c], v[3][c], X);
#pragma unroll
        for (int d = 0; d < 4; d++) u[c + 4 * d] = X[d];
    }
}

// One Stockham pass of radix R over FR frames of M points, NS = the product of the radices before it: butterfly j of a frame reads
// elements j + r M / R, turns element r by W_{NS R}^{r (j mod NS)}, and writes DFT_R of them to (j / NS) NS R + (j mod NS) + r NS.
// In place: every element is read once and written once, and the workgroup meets between the two.
template <int M, int R, int NS, int FR>
__device__ __forceinline__ void chz_narrow_pass(cf2 *u, const float2 *tw, int t)
{
    constexpr int S = chz_narrow_stride(M), BPF = M / R, NB = FR * BPF / 256;
    static_assert(NB >= 1 && NB * 256 == FR * BPF, "whole butterflies per thread");
    cf2 v[NB][R];
#pragma unroll
    for (int q = 0; q < NB; q++) {
        const int g = t + 256 * q, f = g / BPF, j = g % BPF;
        const cf2 *A = u + f * S;
#pragma unroll
        for (int r = 0; r < R; r++) v[q][r] = A[chz_narrow_pos(j + r * BPF)];
        if constexpr (NS > 1) {
            const int k = j % NS;
#pragma unroll
            for (int r = 1; r < R; r++) { const float2 w = tw[r * k * (M / (NS * R))]; v[q][r] = cmul(v[q][r], (cf2){ w.x, w.y }); }
        }
        chz_dft(v[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NB; q++) {
        const int g = t + 256 * q, f = g / BPF, j = g % BPF;
        cf2 *A = u + f * S;
        const int j0 = (j / NS) * NS * R + j % NS;
#pragma unroll
        for (int r = 0; r < R; r++) A[chz_narrow_pos(j0 + r * NS)] = v[q][r];
    }
    __syncthreads();
}

// The kernel's body is recc_chz_narrow_body.inc, once per entry point (see there for why it is text, not a function).
template <int M, int DEC, typename T>
__global__ __launch_bounds__(256) void chz_narrow_kernel(ChzNarrowArgs a)
{
#include "recc_chz_narrow_body.inc"
}
// the same on a block of 8-bit I/Q read in place (T = xl_sc8 or xl_cu8), 2 bytes per sample from HBM: a name of their own for
// these instantiations, nothing else
template <int M, int DEC, typename T>
__global__ __launch_bounds__(256) void chz_narrow_b8_kernel(ChzNarrowArgs a)
{
    static_assert(sizeof(T) == 2, "an 8-bit pair");
#include "recc_chz_narrow_body.inc"
}

// the mixing twin, every sample type behind one name: the staging loop mixes, the rest is the body as it stands
template <int M, int DEC, typename T>
__global__ __launch_bounds__(256) void chz_narrow_mix_kernel(ChzMixArgs m)
{
    const ChzNarrowArgs &a = m.bank;
#define CHZ_BODY_MIX m
#include "recc_chz_narrow_body.inc"
#undef CHZ_BODY_MIX
}

// e^{-2 pi i k / M}, k < M, rounded once from double precision
inline std::vector<float2> chz_narrow_twiddles(int M)
{
    std::vector<float2> w(M);
    for (int k = 0; k < M; k++) {
        const double ph = -2.0 * M_PI * (double)k / (double)M;
        w[k] = make_float2((float)std::cos(ph), (float)std::sin(ph));
    }
    // the four axis points exactly
    w[0] = make_float2(1.f, 0.f); w[M / 4] = make_float2(0.f, -1.f); w[M / 2] = make_float2(-1.f, 0.f); w[3 * M / 4] = make_float2(0.f, 1.f);
    return w;
}

} // namespace amps
