// recc_xlate_shared.hip.h -- the channel filter of recc_xlate.hip.h for MANY channels of ONE shared stream: one fc32 input row
// (a modest SDR tuned to a system's control channels: a few hundred ksps holding many 30 kHz channels), C centres, C output rows
// at rate / D in front of the fused IQ seam.
//
// Per output sample the arithmetic is exactly xlate_fir_kernel's: the phasor of a sample comes from its ABSOLUTE index through
// xl_phasor, one fp32 cmul per staged sample, one fma chain over the zero-padded real taps in ascending tap order.  Row c is
// therefore bit for bit what xlate_fir_kernel gives a one-channel handle configured with centre c: the identity the tests hold
// this kernel to, and the reason nothing here is "optimised" across channels in the float domain.
//
// Form: STAGED.  The grid is (input tiles, channel groups).  A workgroup reads its raw tile plus the filter history from HBM /
// the carry ONCE into LDS and then, for each channel of its group: mixes the raw window into the padded window (xl_pad, lane
// stride 8 conflict free as in xlate_fir_kernel), barrier, FIR, store, barrier.  The raw tile is read once per group instead of
// once per channel, and one launch serves all channels.  The host picks the group size (xlate_shared_cpg) so that the grid has a
// few thousand workgroups where the block allows it -- balance over the CUs matters more than the re-read of the raw tile, which
// comes from L2 (measured) -- and one group of all channels only for very long blocks.
//
// D = 8 (one output per lane) is new here: 1.6 Msps at 10 samples per symbol, where the flow graph's filter spec gives 1195
// taps -- hence XLS_MAX_TAPS = 1280.  Static LDS: raw 26 624 + mixed 30 016 + taps 5 120 = 61 760 bytes of the 65 536 one
// workgroup may own statically.
#pragma once
#include "recc_xlate.hip.h"

namespace amps {

constexpr int XLS_MAX_TAPS = 1280;   // padded tap count limit of this kernel (XL_MAX_TAPS stays xlate_fir_kernel's)

struct XlateSharedArgs {
    const float2 *block;     // [nsamp] new samples, one row
    const float2 *carry;     // [carry_cap]: hist samples of history, then the leftover (< D) unconsumed samples
    const float *taps;       // [ntp], zero padded to a multiple of 8
    const uint64_t *steps;   // [C]: center_hz[c] / rate_hz as a 0.64 fixed-point fraction of a turn
    float2 *out;             // [C][ld_out]
    uint64_t ld_out;
    uint64_t n_abs0;         // absolute input index of the first unconsumed sample (virtual index v = hist)
    uint32_t carry_len, hist, nsamp, nout, ntp, C, cpg;   // cpg: channels per workgroup (blockIdx.y = group)
};

template <int D>
__global__ __launch_bounds__(256) void xlate_shared_kernel(XlateSharedArgs a)
{
    constexpr int OPT = 8 / D;                                   // outputs per lane
    __shared__ float2 xs[XL_TILE + XLS_MAX_TAPS];                // the raw window, staged once
    __shared__ cf2 zs[xl_pad(XL_TILE + XLS_MAX_TAPS) + 8];       // the window mixed for the channel in hand
    __shared__ float hs[XLS_MAX_TAPS];
    static_assert(sizeof(float2) * (XL_TILE + XLS_MAX_TAPS) + sizeof(cf2) * (xl_pad(XL_TILE + XLS_MAX_TAPS) + 8) + sizeof(float) * XLS_MAX_TAPS <= 65536,
                  "static LDS of one workgroup");
    const int t = threadIdx.x;
    const uint32_t k0 = blockIdx.x * (XL_TILE / D);
    const int H = (int)a.hist;                                   // = ntp - 1
    const int ntp = (int)a.ntp;
    const int64_t vtot = (int64_t)a.carry_len + a.nsamp;
    const int64_t v0 = (int64_t)D * k0;

    for (int i = t; i < ntp; i += 256) hs[i] = a.taps[i];
    // stage: tile-local sample n <-> virtual index v = D*k0 + n;  lane t takes n = t, t+256, ...
    for (int n = t; n < XL_TILE + H; n += 256) {
        const int64_t v = v0 + n;
        float2 s = make_float2(0.f, 0.f);
        if (v < (int64_t)a.carry_len) s = a.carry[v];
        else if (v < vtot) s = a.block[v - a.carry_len];
        xs[n] = s;
    }
    __syncthreads();

    const uint64_t nabs0 = a.n_abs0 + (uint64_t)(v0 - H);        // wraps consistently for the (zero) pre-stream history
    const uint32_t c_end = min(a.C, (blockIdx.y + 1) * a.cpg);
    for (uint32_t c = blockIdx.y * a.cpg; c < c_end; c++) {
        // mix: the phasor is evaluated per sample from the absolute index, so a sample is mixed to the same bits whatever tile,
        // push or handle it lands in
        const uint64_t step = a.steps[c];
        for (int n = t; n < XL_TILE + H; n += 256) {
            const float2 s = xs[n];
            zs[xl_pad(n)] = cmul((cf2){ s.x, s.y }, xl_phasor((nabs0 + (uint64_t)n) * step));
        }
        __syncthreads();

        cf2 acc[OPT];
#pragma unroll
        for (int j = 0; j < OPT; j++) acc[j] = (cf2){ 0.f, 0.f };
        // tile-local sample of (output j, tap i+e) = 8t + u, u = (H - 7 - i) + (7 + D j - e), as in xlate_fir_kernel (D OPT = 8)
        const cf2 *zp = zs + 9 * t + 9 * ((H - 7) >> 3);
        for (int i = 0; i < ntp; i += 8, zp -= 9) {              // ascending tap order: the summation order of the spec
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float h = hs[i + e];
#pragma unroll
                for (int j = 0; j < OPT; j++)
                    acc[j] = __builtin_elementwise_fma(zp[xl_pad(7 + D * j - e)], (cf2){ h, h }, acc[j]);
            }
        }
        float2 *o = a.out + (uint64_t)c * a.ld_out;
#pragma unroll
        for (int j = 0; j < OPT; j++) {
            const uint32_t k = k0 + OPT * t + j;
            if (k < a.nout) o[k] = make_float2(acc[j].x, acc[j].y);
        }
        __syncthreads();                                         // the next channel overwrites the mixed window
    }
}

struct XlateSharedState {
    bool enabled = false;
    uint32_t C = 0, D = 0, ntaps = 0, ntp = 0, hist = 0, carry_cap = 0, carry_len = 0, max_out = 0;
    int cur = 0;
    uint64_t n_abs = 0;
    DevBuf<float> taps;
    DevBuf<uint64_t> steps;
    DevBuf<float2> carry[2];         // one shared row of hist + D samples, double-buffered
    DevBuf<float2> out;              // [C][max_out]
    HostStage stage;                 // host-resident blocks: one row of D * max_out samples
};

inline void xlate_shared_destroy(XlateSharedState &x) { x = XlateSharedState{}; }

inline int xlate_shared_reset(XlateSharedState &x, hipStream_t s)
{
    if (!x.enabled) return 0;
    if (hipMemsetAsync(x.carry[0].get(), 0, sizeof(float2) * x.carry_cap, s) != hipSuccess) return -EIO;
    if (hipMemsetAsync(x.carry[1].get(), 0, sizeof(float2) * x.carry_cap, s) != hipSuccess) return -EIO;
    x.cur = 0; x.carry_len = x.hist; x.n_abs = 0;
    return 0;
}

inline int xlate_shared_create(XlateSharedState &x, uint32_t C, uint32_t D, uint32_t max_out, double rate_hz, const double *center_hz,
                               const std::vector<float> &taps, hipStream_t s)
{
    xlate_shared_destroy(x);
    if (!(D == 1 || D == 2 || D == 4 || D == 8) || C == 0 || !center_hz || taps.empty() || !(rate_hz > 0.0)) return -EINVAL;
    std::vector<uint64_t> steps(C);
    for (uint32_t c = 0; c < C; c++) {
        if (!(std::fabs(center_hz[c]) <= rate_hz)) return -EINVAL;
        // fraction of a turn per input sample, two's complement for negative offsets: as xlate_create computes it
        const long double f = (long double)center_hz[c] / (long double)rate_hz;
        const long double fr = f - std::floor(f);
        steps[c] = (uint64_t)(fr * 18446744073709551616.0L);
    }
    const uint32_t ntp = (uint32_t)((taps.size() + 7) / 8 * 8);
    if (ntp > (uint32_t)XLS_MAX_TAPS) return -E2BIG;
    x.C = C; x.D = D; x.ntaps = (uint32_t)taps.size(); x.ntp = ntp; x.hist = ntp - 1; x.carry_cap = ntp + D; x.max_out = max_out;
    std::vector<float> padded(ntp, 0.0f);
    for (size_t i = 0; i < taps.size(); i++) padded[i] = taps[i];
    int rc = x.taps.alloc(ntp) | x.steps.alloc(C) | x.carry[0].alloc(x.carry_cap) | x.carry[1].alloc(x.carry_cap) | x.out.alloc((size_t)C * max_out);
    if (!rc && hipMemcpy(x.taps.get(), padded.data(), sizeof(float) * ntp, hipMemcpyHostToDevice) != hipSuccess) rc = -EIO;
    if (!rc && hipMemcpy(x.steps.get(), steps.data(), sizeof(uint64_t) * C, hipMemcpyHostToDevice) != hipSuccess) rc = -EIO;
    if (rc) { xlate_shared_destroy(x); return rc; }
    x.enabled = true;
    return xlate_shared_reset(x, s);
}

// channels per workgroup: as many groups of as few channels as it takes to reach WANT workgroups; one group (the raw tile read once)
// when the tiles alone are that many.  The output bits do not depend on it.
inline uint32_t xlate_shared_cpg(uint32_t C, uint64_t tiles)
{
    constexpr uint64_t WANT = 4096;                              // workgroups: sixteen per CU of a 256-CU device (measured: DESIGN.md 4.7b)
    const uint64_t groups = std::min<uint64_t>(C, std::max<uint64_t>(1, (WANT + tiles - 1) / tiles));
    return (uint32_t)((C + groups - 1) / groups);
}

// filter nsamp new samples of the one shared row (host or device); *out_iq is [C][*out_ld] device memory holding *nout samples per row
inline int xlate_shared_run(XlateSharedState &x, const float2 *iq, size_t nsamp, int mem, hipStream_t s,
                            const float2 **out_iq, uint64_t *out_ld, uint32_t *nout)
{
    *out_iq = x.out.get(); *out_ld = x.max_out; *nout = 0;
    if (!x.enabled) return -ENOSYS;
    if (nsamp == 0) return 0;
    if (nsamp > (size_t)x.D * x.max_out) return -E2BIG;
    const uint64_t avail = (uint64_t)(x.carry_len - x.hist) + nsamp;
    const uint64_t n_out = avail / x.D;
    if (n_out > x.max_out) return -E2BIG;
    const float2 *d = iq;
    if (mem == AMPS_MEM_HOST) {
        uint64_t ld = 0;
        if (int rc = x.stage.stage(iq, nsamp, nsamp, 1, (size_t)x.D * x.max_out, &d, &ld)) return rc;
    }
    XlateSharedArgs a{};
    a.block = d; a.carry = x.carry[x.cur].get(); a.taps = x.taps.get(); a.steps = x.steps.get(); a.out = x.out.get(); a.ld_out = x.max_out;
    a.n_abs0 = x.n_abs; a.carry_len = x.carry_len; a.hist = x.hist; a.nsamp = (uint32_t)nsamp; a.nout = (uint32_t)n_out; a.ntp = x.ntp; a.C = x.C;
    if (n_out) {
        const uint64_t tiles = (n_out * x.D + XL_TILE - 1) / XL_TILE;
        a.cpg = xlate_shared_cpg(x.C, tiles);
        const dim3 grid((uint32_t)tiles, (x.C + a.cpg - 1) / a.cpg);
        switch (x.D) {
        case 1: hipLaunchKernelGGL(xlate_shared_kernel<1>, grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL(xlate_shared_kernel<2>, grid, dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(xlate_shared_kernel<4>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(xlate_shared_kernel<8>, grid, dim3(256), 0, s, a); break;
        }
    }
    const uint32_t consumed = (uint32_t)(n_out * x.D);
    const uint32_t new_len = x.hist + (uint32_t)(avail - (uint64_t)consumed);
    hipLaunchKernelGGL(xlate_carry_kernel, dim3((new_len + 255) / 256, 1), dim3(256), 0, s, d, (uint64_t)nsamp, x.carry[x.cur].get(), x.carry[x.cur ^ 1].get(),
                       x.carry_cap, x.carry_len, consumed, new_len);
    if (hipGetLastError() != hipSuccess) return -EIO;
    if (mem == AMPS_MEM_HOST) { if (int rc = x.stage.arm(s)) return rc; }
    x.cur ^= 1; x.carry_len = new_len; x.n_abs += consumed;
    *nout = (uint32_t)n_out;
    return 0;
}

} // namespace amps
