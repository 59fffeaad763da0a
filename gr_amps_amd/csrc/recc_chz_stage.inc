// recc_chz_stage.inc -- the staging loop of the two-kernel banks' bodies (recc_chz_narrow_body.inc, recc_chz_grid10_body.inc), included
// once by each inside a block of its own: text, not a header, for the reason recc_chz_narrow_body.inc gives.  In scope: T (the sample
// type of a.block), the bank's arguments `ChzNarrowArgs a`, the constants NST (samples a workgroup stages) and DEC, frame0, the thread
// index t and the LDS array xin[NST].  Sample i of the workgroup is carry-relative sample frame0 D + i; behind the stream's end (frames
// this launch does not produce) zeros.
// Eight loads in flight per thread: every load is unconditional, from an address that is valid whatever the sample is (element 0 of the
// carry, which is never empty, or of the block, which has a sample whenever a launch produces a frame), and what it returned is kept
// or replaced by zero afterwards, so that a batch costs one memory latency and not eight.  An integer block is read a sample per load
// (4 bytes of sc16, 2 bytes of sc8 / cu8, at the sample's own alignment): a load lies inside one aligned dword that holds the sample
// it asks for, so nothing in front of the block's first or behind its last such dword is touched.
// A mixing twin (chz_narrow_mix_kernel, chz_grid10_mix_kernel) defines CHZ_BODY_MIX as its ChzMixArgs around the body's include: what a
// thread loaded is then mixed by the sample's absolute index (chz_mix_staged) on its way into LDS, and nothing else differs.
        constexpr int NLD = (NST + 255) / 256, BATCH = 8;
        const uint64_t c0 = (uint64_t)frame0 * DEC;
        const T *blk = (const T *)a.block;
#pragma unroll 1
        for (int i0 = 0; i0 < NLD; i0 += BATCH) {
            cf2 v[BATCH];
#pragma unroll
            for (int b = 0; b < BATCH; b++) {
                const uint64_t ci = c0 + (uint64_t)(t + 256 * (i0 + b));
                const bool in_carry = ci < a.carry_len;
                const uint64_t bi = ci - a.carry_len;
                const bool in_block = !in_carry && bi < a.nsamp;
                if constexpr (chz_is_short<T>::value) {
                    const float2 c = a.carry[in_carry ? ci : 0];
                    const cf2 s = chz_cvt(blk[in_block ? bi : 0]);
                    v[b] = in_carry ? (cf2){ c.x, c.y } : in_block ? s : (cf2){ 0.f, 0.f };
                } else {
                    const float2 c = *(in_carry ? a.carry + ci : in_block ? blk + bi : a.carry);
                    v[b] = (in_carry || in_block) ? (cf2){ c.x, c.y } : (cf2){ 0.f, 0.f };
                }
#ifdef CHZ_BODY_MIX                                              // the mixing twin: see above
                v[b] = chz_mix_staged(v[b], CHZ_BODY_MIX, ci);
#endif
            }
#pragma unroll
            for (int b = 0; b < BATCH; b++) {
                const int i = t + 256 * (i0 + b);
                if (i < NST) xin[i] = v[b];
            }
        }
