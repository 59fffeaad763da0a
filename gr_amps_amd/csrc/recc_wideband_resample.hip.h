// recc_wideband_resample.hip.h -- a rational L / M resampler in front of the wideband seam's filter banks: the rates SDRs deliver that
// are no bank's rate (8 Msps x 5/4 -> 10, 12.5 x 2/1 -> 25, 16 x 5/4 -> 20, 6 x 5/3 -> 10, 3.2 x 6/5 -> 3.84; include/amps_recc.h,
// amps_recc_set_wideband_resample).  One stream, no mixing: frequencies in hertz stay where they are.
//
//     k M = L q_k + p_k, 0 <= p_k < L:     y[k] = sum_{i < ntp} h_{p_k}[i] x[q_k - i],     h_p[i] = g[L i + p]
//
// one fp32 fma chain per component in ascending i, k and q absolute indices since create or reset.  wb_resample_kernel<T> reads the
// block in place in its own sample type (8, 4 or 2 bytes per sample from HBM) and writes fc32, which the bank behind it takes as it
// takes any device fc32 block.
//
// One 256-thread workgroup per tile of `tile` outputs K0 ... K0 + tile - 1.  With K0 M = L Q0 + P0 these read the inputs
// Q0 - (ntp - 1) ... Q0 + floor((P0 + (tile - 1) M) / L): the workgroup stages them once in LDS as fc32 -- from the history buffer in
// front of the block, as the banks stage carry and block -- behind the L tap sets.  The tap sets lie in LDS as the prototype itself,
// hs[L i + p] = h_p[i]: the lanes of a wave hold consecutive k and so at most L different p, which read consecutive words for one i.
// A lane's input advances by M / L samples from lane to lane: the same or the next 8-byte word while resampling up, every second one
// at 1 / 2 (two lanes of a 32-lane group on a bank).  Thread t computes outputs t, t + 256, ...: the stores of a wave are 512
// consecutive bytes.  The limits (wbr_limits, recc_wideband_resample.h) are checked by the host before it configures and by the
// kernel at its top.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <vector>
#include "amps_recc.h"
#include "recc_chz_common.hip.h"    // cf2, the sample types and their one list
#include "recc_devmem.hip.h"
#include "recc_wideband_resample.h"

namespace amps {

struct WbResampleArgs {
    const void *block;       // this push's samples in their own type: absolute inputs n_abs0 ... n_abs0 + nsamp - 1
    const float2 *hist;      // [ntp - 1] fc32: absolute inputs n_abs0 - (ntp - 1) ... n_abs0 - 1, zeros before the stream's start
    const float *taps;       // [L][ntp], phase p at taps + p ntp
    float2 *out;             // [nout]: outputs k_abs0 ...
    uint64_t n_abs0, k_abs0;
    uint32_t nsamp, nout;
    uint32_t L, M, ntp, tile;
};

template <typename T>
__global__ __launch_bounds__(WBR_THREADS) void wb_resample_kernel(WbResampleArgs a)
{
    extern __shared__ float4 wbr_lds[];
    const uint32_t L = a.L, M = a.M, ntp = a.ntp, tile = a.tile, H = ntp - 1;
    if (wbr_limits(L, M, ntp, tile) || blockDim.x != WBR_THREADS) return;
    float *hs = (float *)wbr_lds;                                 // [ntp][L]
    cf2 *xs = (cf2 *)(hs + L * ntp);                              // L ntp is a multiple of 8 floats
    const uint32_t t = threadIdx.x;
    const uint32_t k0 = blockIdx.x * tile;                        // < nout
    const uint32_t nk = min(tile, a.nout - k0);
    const uint64_t KM = (a.k_abs0 + k0) * (uint64_t)M;
    const uint64_t Q0 = KM / L;
    const uint32_t P0 = (uint32_t)(KM - Q0 * L);
    const uint32_t W = (P0 + (nk - 1) * M) / L + ntp;             // <= wbr_window(L, M, ntp, tile): the LDS the host asked for
    // window sample n is absolute input Q0 - H + n, block sample b0 + n.  Q0 >= n_abs0 (the push's first output is the first k with
    // q_k >= n_abs0), so b0 >= -H: what lies in front of the block is in the history
    const int64_t b0 = (int64_t)(Q0 - a.n_abs0) - (int64_t)H;
    const T *block = (const T *)a.block;

    for (uint32_t i = t; i < L * ntp; i += WBR_THREADS) { const uint32_t p = i / ntp, j = i - p * ntp; hs[j * L + p] = a.taps[i]; }
    for (uint32_t n = t; n < W; n += WBR_THREADS) {
        const int64_t b = b0 + n;
        cf2 s = (cf2){ 0.f, 0.f };
        if (b < 0) { if (b + (int64_t)H >= 0) { const float2 c = a.hist[b + (int64_t)H]; s = (cf2){ c.x, c.y }; } }
        else if (b < (int64_t)a.nsamp) s = chz_cvt(block[b]);
        xs[n] = s;
    }
    __syncthreads();

    for (uint32_t j = t; j < nk; j += WBR_THREADS) {
        const uint32_t e = P0 + j * M, dq = e / L, p = e - dq * L;   // output k0 + j: q = Q0 + dq, phase p
        const cf2 *x = xs + dq + H;                                  // x[-i] = input q - i
        const float *h = hs + p;
        cf2 acc = (cf2){ 0.f, 0.f };
#pragma unroll 8
        for (uint32_t i = 0; i < ntp; i++) {                          // ascending tap order: the summation order of the definition
            const float hv = h[i * L];
            acc = __builtin_elementwise_fma(x[-(int)i], (cf2){ hv, hv }, acc);
        }
        a.out[k0 + j] = make_float2(acc.x, acc.y);
    }
}

// hist_out[i] = the stream's sample (end of this push) - (ntp - 1) + i, as fc32: out of the old history or the block, whose samples are
// converted here -- which is what lets the sample type change from one push to the next
template <typename T>
__global__ __launch_bounds__(256) void wb_resample_carry_kernel(const T *block, const float2 *hist_in, float2 *hist_out, uint32_t H, uint32_t nsamp)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    const uint64_t v = (uint64_t)nsamp + i;                       // index into history ++ block
    if (v < H) hist_out[i] = hist_in[v];
    else { const cf2 c = chz_cvt(block[v - H]); hist_out[i] = make_float2(c.x, c.y); }
}

// The resampler of a handle's wideband seam (ChannelizerState::rs).  Kept over a reset, which restarts the stream.
struct WbResampleState {
    bool enabled = false;
    uint32_t L = 1, M = 1, ntp = 0;
    double rate_hz = 0.0;            // of the delivered stream
    DevBuf<float> taps;              // [L][ntp]
    DevBuf<float2> hist[2];          // [ntp - 1], double-buffered: written by wb_resample_carry_kernel
    int cur = 0;
    uint64_t n_abs = 0, k_abs = 0;   // inputs taken and outputs delivered since create or reset
    DevBuf<float2> out;              // a push's outputs, grown on demand
};

inline int wb_resample_reset(WbResampleState &r, hipStream_t s)
{
    if (!r.enabled) return 0;
    for (auto &h : r.hist) if (hipMemsetAsync(h.get(), 0, sizeof(float2) * h.capacity(), s) != hipSuccess) return -EIO;
    r.cur = 0; r.n_abs = 0; r.k_abs = 0;
    return 0;
}

// A state for a filter wbr_admit has admitted: g is the prototype (f.ng taps), split here into its L phases.  *r is replaced only
// where everything succeeded.
inline int wb_resample_create(WbResampleState &r, uint32_t L, uint32_t M, double rate_hz, const WbrFilter &f, const std::vector<float> &g, hipStream_t s)
{
    WbResampleState n;
    n.L = L; n.M = M; n.ntp = f.ntp; n.rate_hz = rate_hz;
    std::vector<float> h((size_t)L * f.ntp, 0.f);
    for (size_t i = 0; i < g.size(); i++) h[(i % L) * f.ntp + i / L] = g[i];
    if (n.taps.alloc(h.size()) || n.hist[0].alloc(f.ntp - 1) || n.hist[1].alloc(f.ntp - 1)) return -ENOMEM;
    if (hipMemcpy(n.taps.get(), h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice) != hipSuccess) return -EIO;
    n.enabled = true;
    if (int rc = wb_resample_reset(n, s)) return rc;
    if (hipStreamSynchronize(s) != hipSuccess) return -EIO;
    r = std::move(n);
    return 0;
}

// outputs a push of nsamp samples delivers: host arithmetic, nothing moves
inline uint64_t wb_resample_count(const WbResampleState &r, size_t nsamp) { return wbr_outputs(r.L, r.M, r.n_abs + nsamp) - r.k_abs; }

// Resample the device block d (nsamp samples of `format`) into r.out and move the stream on: *nout outputs, fc32.  Stream order keeps
// r.out safe: the kernels of the previous push that read it run before this one writes it.
inline int wb_resample_run(WbResampleState &r, const void *d, size_t nsamp, int format, hipStream_t s, uint32_t *nout)
{
    const uint64_t n64 = wb_resample_count(r, nsamp);
    if (nsamp > 0xffffffffull || n64 > 0xffffffffull) return -E2BIG;
    const uint32_t n = (uint32_t)n64, H = r.ntp - 1;
    if (r.out.capacity() < n) {
        if (r.out && hipStreamSynchronize(s) != hipSuccess) return -EIO;       // ... so they must have run before it is freed to grow
        if (r.out.reserve(n)) return -ENOMEM;
    }
    WbResampleArgs a{};
    a.block = d; a.hist = r.hist[r.cur].get(); a.taps = r.taps.get(); a.out = r.out.get();
    a.n_abs0 = r.n_abs; a.k_abs0 = r.k_abs; a.nsamp = (uint32_t)nsamp; a.nout = n;
    a.L = r.L; a.M = r.M; a.ntp = r.ntp; a.tile = WBR_TILE;
    const int ok = chz_with_sample_type(format, [&](auto t) {
        using T = decltype(t);
        if (n) hipLaunchKernelGGL(wb_resample_kernel<T>, dim3((n + WBR_TILE - 1) / WBR_TILE), dim3(WBR_THREADS), (size_t)wbr_lds_bytes(r.L, r.M, r.ntp, WBR_TILE), s, a);
        hipLaunchKernelGGL(wb_resample_carry_kernel<T>, dim3((H + 255) / 256), dim3(256), 0, s, (const T *)d, r.hist[r.cur].get(), r.hist[r.cur ^ 1].get(), H, (uint32_t)nsamp);
        return 1;
    });
    if (!ok) return -EINVAL;
    if (hipGetLastError() != hipSuccess) return -EIO;
    r.cur ^= 1;
    r.n_abs += nsamp;
    r.k_abs += n;
    *nout = n;
    return 0;
}

} // namespace amps
