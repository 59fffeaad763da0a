// recc_chz_grid10_body.inc -- the body of the 10 kHz-grid banks' kernel, included once per entry point by recc_chz_grid10.hip.h: text,
// not a header, for the reason recc_chz_narrow_body.inc gives.  The entry points are chz_grid10_kernel and its mixing twin
// chz_grid10_mix_kernel (amps_recc_set_wideband_shift), which defines CHZ_BODY_MIX as its ChzMixArgs around the include: what a thread
// loaded is then mixed by the sample's absolute index (chz_mix_staged) on its way into LDS, and nothing else differs.  In scope: the
// template parameters M and T (the sample type of a.block), the bank's arguments `ChzNarrowArgs a`, and what recc_chz_grid10.hip.h
// defines in front of the entry points.
    static_assert(chz_grid10_size(M), "M = 2500, 2000, 1000 or 500");
    constexpr int P = CHZ_GRID10_P, DEC = M / 4, FR = chz_grid10_fr(M), S = chz_grid10_stride(M), NST = chz_grid10_stage(M);
    constexpr int NBR = (M + 255) / 256;                         // branches a thread folds
    constexpr int E = (FR * M + 255) / 256;                      // (bin, frame) pairs a thread stores
    static_assert(FR % 4 == 0 && S >= M && chz_grid10_lds_bytes(M) <= 80 * 1024, "whole periods of the roll; two workgroups per CU");
    __shared__ cf2 lds[chz_grid10_lds_elems(M)];
    cf2 *const xin = lds, *const u = lds;                        // [NST] staged input until the fold has read it, [FR * S] frames from then on
    const int t = threadIdx.x;
    const uint32_t frame0 = blockIdx.x * (uint32_t)FR;

    float h[NBR][P];
#pragma unroll
    for (int b = 0; b < NBR; b++)
#pragma unroll
        for (int p = 0; p < P; p++) h[b][p] = a.taps[p * M + (t + 256 * b) % M];

    // stage the workgroup's input in LDS, expanded to fc32: recc_chz_stage.inc, the one text of both families' bodies
    {
#include "recc_chz_stage.inc"
    }
    __syncthreads();

    // fold: into registers, and into the input's place once every thread has read what it needs of it
    cf2 acc[NBR][FR];
#pragma unroll
    for (int b = 0; b < NBR; b++) {
        const int j = t + 256 * b;
        if (j < M) {
#pragma unroll
            for (int f = 0; f < FR; f++) {
                const cf2 *x = xin + f * DEC + j;
                acc[b][f] = x[0] * h[b][0];
#pragma unroll
                for (int p = 1; p < P; p++) { const cf2 s = x[p * M]; acc[b][f] = (cf2){ fmaf(h[b][p], s.x, acc[b][f].x), fmaf(h[b][p], s.y, acc[b][f].y) }; }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NBR; b++) {
        const int j = t + 256 * b;
        if (j < M) {
#pragma unroll
            for (int f = 0; f < FR; f++) {
                const int k = j + ((f + 1) & 3) * DEC;           // + ((f + 1) D) mod M
                u[f * S + (k >= M ? k - M : k)] = acc[b][f];
            }
        }
    }
    __syncthreads();

    chz_grid10_pass<M, 5, 1, FR>(u, a.twiddle, t);
    chz_grid10_pass<M, 5, 5, FR>(u, a.twiddle, t);
    chz_grid10_pass<M, 5, 25, FR>(u, a.twiddle, t);
    if constexpr (M == 2500) {
        chz_grid10_pass<M, 5, 125, FR>(u, a.twiddle, t);
        chz_grid10_pass<M, 4, 625, FR>(u, a.twiddle, t);
    } else {
        chz_grid10_pass<M, M / 125, 125, FR>(u, a.twiddle, t);
    }

    // store: the frame runs fastest across lanes
#pragma unroll
    for (int q = 0; q < E; q++) {
        const int idx = t + 256 * q, f = idx % FR, bin = idx / FR;
        if (bin < M) {
            const uint32_t row = a.bin2row[bin], frame = frame0 + (uint32_t)f;
            if (row < a.n_channels && frame < a.nframes) {
                const cf2 y = u[f * S + bin];
                a.out[(uint64_t)row * a.ld + frame] = make_float2(y.x, y.y);
            }
        }
    }
