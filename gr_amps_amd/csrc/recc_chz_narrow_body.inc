// recc_chz_narrow_body.inc -- the body of the narrow banks' kernel, included once per entry point by recc_chz_narrow.hip.h: text, not a
// header (no include guard, nothing that stands alone).  The entry points are chz_narrow_kernel (T = float2 or chz_sc16) and
// chz_narrow_b8_kernel (T = xl_sc8 or xl_cu8, a block of 8-bit I/Q read in place).  In scope: the template parameters M, DEC and T (the
// sample type of a.block), the argument `ChzNarrowArgs a`, and what recc_chz_narrow.hip.h defines in front of the entry points.  Only
// the staging loop knows T: it expands to fc32 (chz_cvt) into one LDS layout, and the fold, the passes and the store run on that
// whatever the block was.
// Why text and not a function: as for recc_chz12_body.hip.h.  Moved into a __device__ __forceinline__ function template -- nothing else
// changed -- all twelve chz_narrow_kernel instantiations came out as different code with the argument by reference (4 to 82 lines
// longer), and six of them with the argument by value.  As text they compile to the instruction stream they had before the 8-bit
// entry point existed.
// A third entry point, chz_narrow_mix_kernel (amps_recc_set_wideband_shift), defines CHZ_BODY_MIX as its ChzMixArgs around the include:
// the staging loop (recc_chz_stage.inc) then mixes what a thread loaded, and nothing else differs.  The other two do not define it
// and see the text they saw before.
    static_assert(chz_narrow_geometry(M, DEC), "M = 512, 256 or 128 at D = M / 2 or 3 M / 4");
    constexpr int FR = chz_narrow_fr(M, DEC), S = chz_narrow_stride(M), NST = chz_narrow_stage(M, DEC);
    constexpr int E = FR * M / 256;                              // (frame, branch) pairs, and later (bin, frame) pairs, per thread
    constexpr int BR = M > 256 ? M / 256 : 1;                    // branches whose taps a thread keeps
    static_assert(chz_narrow_lds_bytes(M, DEC) <= 80 * 1024, "two workgroups per CU");
    __shared__ cf2 xin[NST];
    __shared__ cf2 u[FR * S];
    const int t = threadIdx.x;
    const uint32_t frame0 = blockIdx.x * (uint32_t)FR;

    float h[BR][8];
#pragma unroll
    for (int b = 0; b < BR; b++)
#pragma unroll
        for (int p = 0; p < 8; p++) h[b][p] = a.taps[p * M + (t + 256 * b) % M];

    // stage the workgroup's input in LDS, expanded to fc32: recc_chz_stage.inc, the one text of both families' bodies
    {
#include "recc_chz_stage.inc"
    }
    __syncthreads();

    // fold
#pragma unroll
    for (int q = 0; q < E; q++) {
        const int idx = t + 256 * q, f = idx / M, j = idx % M;
        const float (&hb)[8] = h[M > 256 ? q % BR : 0];
        const cf2 *x = xin + f * DEC + j;
        cf2 acc = x[0] * hb[0];
#pragma unroll
        for (int p = 1; p < 8; p++) { const cf2 s = x[p * M]; acc = (cf2){ fmaf(hb[p], s.x, acc.x), fmaf(hb[p], s.y, acc.y) }; }
        // q and M fix f up to the thread's half at M = 128; the roll ((f + 1) D) mod M takes 2 or 4 values
        u[f * S + chz_narrow_pos((j + ((f + 1) * DEC) % M) & (M - 1))] = acc;
    }
    __syncthreads();

    if constexpr (M == 512) {
        chz_narrow_pass<M, 8, 1, FR>(u, a.twiddle, t);
        chz_narrow_pass<M, 8, 8, FR>(u, a.twiddle, t);
        chz_narrow_pass<M, 8, 64, FR>(u, a.twiddle, t);
    } else if constexpr (M == 256) {
        chz_narrow_pass<M, 16, 1, FR>(u, a.twiddle, t);
        chz_narrow_pass<M, 16, 16, FR>(u, a.twiddle, t);
    } else {
        chz_narrow_pass<M, 16, 1, FR>(u, a.twiddle, t);
        chz_narrow_pass<M, 8, 16, FR>(u, a.twiddle, t);
    }

    // store: the frame runs fastest across lanes
#pragma unroll
    for (int q = 0; q < E; q++) {
        const int idx = t + 256 * q, f = idx % FR, bin = idx / FR;
        const uint32_t row = a.bin2row[bin], frame = frame0 + (uint32_t)f;
        if (row < a.n_channels && frame < a.nframes) {
            const cf2 y = u[f * S + chz_narrow_pos(bin)];
            a.out[(uint64_t)row * a.ld + frame] = make_float2(y.x, y.y);
        }
    }
