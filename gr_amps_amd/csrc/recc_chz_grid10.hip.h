// recc_chz_grid10.hip.h -- the filter bank of the wideband seam at rates that are multiples of 10 kHz but not of 30 kHz: M = fs / 10 kHz
// = 2500, 2000, 1000 or 500 branches (25, 20, 10 and 5 Msps: what radios on a 100 or 200 MHz clock, and the 10 Msps dongles, deliver),
// D = M / 4 input samples per frame: 40 ksps per channel, two samples per Manchester symbol.  Bins are 10 kHz apart, so a 30 kHz
// channel sits on every third one (the host's bin2row says which).  The same weighted-overlap-add bank as recc_channelizer.hip.h
// defines at its top and oracle/channelizer.py models -- here P = 3 taps per branch (300 us of prototype), frame m over samples
// [(m+1) D - 3 M, (m+1) D), the fold modulo M with the absolute phase reference n0 mod M, an M-point DFT -- in the two-kernel form
// only, like the narrow banks (recc_chz_narrow.hip.h), whose argument block (ChzNarrowArgs: taps [3 M], hist = 3 M - D here), carry
// and host code it shares.
//
// Mapping: a 256-thread workgroup owns FR consecutive frames for all M bins.
//   stage : the (FR - 1) D + 3 M input samples of its frames, carry first and block behind it, expanded to fc32 (chz_cvt), once in LDS
//   fold  : a thread owns branches t + 256 b, keeps their three taps in registers and folds every frame of the workgroup with one
//           multiply and two FMAs per branch, in that order, out of LDS; the roll n0 mod M is an index offset of the store (FR and
//           every launch are multiples of the roll's period, four frames: a workgroup's frame f has roll ((f + 1) D) mod M).  The
//           folded frames take the staged input's place in LDS: a thread keeps its results in registers until the workgroup has
//           read all of the input, which halves the LDS of a workgroup and lets a second one share the CU at every size
//   FFT   : all FR frames at once, Stockham passes in place over LDS, the radix-5 passes first and the power of two last:
//           2500 = 5 x 5 x 5 x 5 x 4, 2000 = 5 x 5 x 5 x 16, 1000 = 5 x 5 x 5 x 8, 500 = 5 x 5 x 5 x 4.  FR M / R butterflies of a pass
//           are no multiple of 256: the loops over a thread's butterflies are guarded.  Twiddles from the host's table (double precision)
//   store : thread -> (bin, frame) with the frame running fastest: a row leaves in runs of FR x 8 bytes
// A frame's arithmetic is a fixed sequence of operations on its own 3 M samples: it depends neither on how the stream was cut into
// pushes nor on which workgroup computes it.  No atomics, nothing handed from one workgroup to another.
//
// LDS layout of a frame: element n at n, NO padding inside a frame.  The narrow banks pad n + n / 32 because their passes write with
// strides of 8, 16, 64 ... elements across lanes, which fold onto a few banks.  Here every access is either stride 1 across lanes
// (all reads of a pass: lane j reads j + r M / R, whatever M / 5 is; the fold; the write of the LAST pass, NS = M / R, which is why the
// power-of-two radix runs last) or a write of the radix-5 passes at runs of NS consecutive elements 5 NS apart, NS = 1, 5, 25, 125:
// odd strides, coprime with the 32 banks a write goes by.  Frames lie S elements apart with S = M rounded up to S mod 32 = 32 / FR:
// the store phase reads (frame f, bin b) at f S + b with f running fastest across lanes, and FR frames x 32 / FR bins then cover the
// 32 pairs of banks of a ds_read_b64 half-wave exactly once.
//
// FR, LDS (the larger of staged input and frame buffers) and the workgroups per CU it admits (the 3 M - D samples of history in front
// of a workgroup's first frame are staged by its neighbour too, from L2: 12 / FR of the input is read a second time):
//   M = 2500: FR = 4, 80 128 B, 2       M = 2000: FR = 4, 64 768 B, 2       M = 1000: FR = 4, 32 000 B, 5       M = 500: FR = 8, 33 024 B, 4
#pragma once
#include <hip/hip_runtime.h>
#include "recc_chz_common.hip.h"
#include "recc_chz_fft.hip.h"
#include "recc_chz_narrow.hip.h"   // ChzNarrowArgs, chz_dft, chz_narrow_twiddles

namespace amps {

constexpr int CHZ_GRID10_P = 3;                                  // taps per branch

__host__ __device__ constexpr bool chz_grid10_size(int M) { return M == 2500 || M == 2000 || M == 1000 || M == 500; }
// frames per workgroup
__host__ __device__ constexpr int chz_grid10_fr(int M) { return M == 500 ? 8 : 4; }
// ... which the host reads from the bank table: its GRID10 rows are exactly this header's sizes, taps and frames per workgroup
constexpr bool chz_grid10_table_agrees()
{
    int n = 0;
    for (const ChzBank &b : CHZ_BANKS) {
        if (b.family != ChzFamily::GRID10) continue;
        if (!chz_grid10_size((int)b.M) || 4u * b.decim[0] != b.M || b.decim[1] || b.taps != (uint32_t)CHZ_GRID10_P || (int)b.fr[0] != chz_grid10_fr((int)b.M)) return false;
        n++;
    }
    return n == 4;
}
static_assert(chz_grid10_table_agrees(), "recc_chz_banks.h states the banks of 10 kHz bins as the kernels are built");
// elements from one frame to the next in LDS: the smallest S >= M with S mod 32 = 32 / FR
__host__ __device__ constexpr int chz_grid10_stride(int M) { return M + ((32 / chz_grid10_fr(M) - M % 32) % 32 + 32) % 32; }
__host__ __device__ constexpr int chz_grid10_stage(int M) { return (chz_grid10_fr(M) - 1) * (M / 4) + CHZ_GRID10_P * M; }
// cf2 elements of a workgroup's LDS: the staged input first, the FR frame buffers in its place afterwards
__host__ __device__ constexpr int chz_grid10_lds_elems(int M) { return chz_grid10_stage(M) > chz_grid10_fr(M) * chz_grid10_stride(M) ? chz_grid10_stage(M) : chz_grid10_fr(M) * chz_grid10_stride(M); }
__host__ __device__ constexpr size_t chz_grid10_lds_bytes(int M) { return sizeof(float2) * (size_t)chz_grid10_lds_elems(M); }

// One Stockham pass as chz_narrow_pass defines it -- butterfly j of a frame reads elements j + r M / R, turns element r by
// W_{NS R}^{r (j mod NS)}, and writes DFT_R of them to (j / NS) NS R + (j mod NS) + r NS -- over frames S elements apart without padding,
// for any count of butterflies: a thread's last ones may not exist.  A sibling of chz_narrow_pass and not a generalisation of it: the
// narrow banks' instantiations stay instruction for instruction what they were (profiles/grid10_bank/isa_identity.txt).
template <int M, int R, int NS, int FR>
__device__ __forceinline__ void chz_grid10_pass(cf2 *u, const float2 *tw, int t)
{
    constexpr int S = chz_grid10_stride(M), BPF = M / R, NBF = FR * BPF, NB = (NBF + 255) / 256;
    static_assert(BPF * R == M && M % (NS * R) == 0, "NS R divides M");
    cf2 v[NB][R];
#pragma unroll
    for (int q = 0; q < NB; q++) {
        const int g = t + 256 * q, f = g / BPF, j = g % BPF;
        if (g < NBF) {
            const cf2 *A = u + f * S;
#pragma unroll
            for (int r = 0; r < R; r++) v[q][r] = A[j + r * BPF];
            if constexpr (NS > 1) {
                const int k = j % NS;
#pragma unroll
                for (int r = 1; r < R; r++) { const float2 w = tw[r * k * (M / (NS * R))]; v[q][r] = cmul(v[q][r], (cf2){ w.x, w.y }); }
            }
            chz_dft(v[q]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NB; q++) {
        const int g = t + 256 * q, f = g / BPF, j = g % BPF;
        if (g < NBF) {
            cf2 *A = u + f * S;
            const int j0 = (j / NS) * NS * R + j % NS;
#pragma unroll
            for (int r = 0; r < R; r++) A[j0 + r * NS] = v[q][r];
        }
    }
    __syncthreads();
}

// T: the sample type of a.block -- float2, chz_sc16, xl_sc8 or xl_cu8, every one read in place.  Only the staging loop knows it.
// The kernel's body is recc_chz_grid10_body.inc, once per entry point.
template <int M, typename T>
__global__ __launch_bounds__(256) void chz_grid10_kernel(ChzNarrowArgs a)
{
#include "recc_chz_grid10_body.inc"
}
// the mixing twin: the staging loop mixes, the rest is the body as it stands
template <int M, typename T>
__global__ __launch_bounds__(256) void chz_grid10_mix_kernel(ChzMixArgs m)
{
    const ChzNarrowArgs &a = m.bank;
#define CHZ_BODY_MIX m
#include "recc_chz_grid10_body.inc"
#undef CHZ_BODY_MIX
}

} // namespace amps
