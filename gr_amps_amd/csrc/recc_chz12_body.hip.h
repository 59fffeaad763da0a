// recc_chz12_body.hip.h -- the body of the filter-bank kernel, included once per entry point by recc_channelizer.hip.h (no include
// guard): chz12_kernel (T = float2, an fc32 block) and chz12_short_kernel (T = chz_sc16, a block of 16-bit I/Q read in place).
// In scope: the template parameters P, MODE, DEC, the argument `ChzArgs a`, the sample type T of a.block, the macro
// CHZ12_BODY_SHORT (1 where T is chz_sc16), and what recc_channelizer.hip.h includes and defines in front of the entry points: the
// fold role's parts (recc_chz_fold.hip.h), the passes (recc_chz_fft.hip.h), the slicer (recc_chz_slicer.hip.h), chz_carry_sample and
// the CHZ_STAMP / CHZ_TL_* timeline macros.  The three ring waits that expand packed samples are chosen by the macro and not by
// `if constexpr`: a discarded branch that names the half-step's age was enough to move registers in the SLICER role of five of the
// ten fc32 kernels.
// Why text and not a function: moved into a __device__ __forceinline__ function -- nothing else changed -- the ten fc32 kernels came
// out as different code (the early return becomes a branch to a common exit, blocks are placed differently; up to 440 instructions
// fewer or more per kernel), and the fc32 kernel is the measured headline.  As text it compiles to the instruction stream it had.
    static_assert(DEC == CHZ_D || DEC == CHZ_D768, "input samples per frame");
    constexpr bool SHORT = chz_is_short<T>::value;
    static_assert(!SHORT || MODE != CHZ12_IQ, "the unfused form takes an sc16 block through chz_short_to_float_kernel");
    constexpr int M = CHZ_M, D = DEC, NB = CHZ_BATCH;
    constexpr int SPS = 1536 / DEC;                                   // frames per Manchester symbol (20 ksym/s at 30.72 Msps)
    constexpr bool IQ = MODE == CHZ12_IQ;
    constexpr int SL = IQ ? AMPS_SLICER_ATAN_BOXCAR : MODE;
    __shared__ cf2 buf[CHZ_SLOTS * NB * CHZ_FB];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    // Role of a wave.  The hardware arbitrates VALU issue between the waves of a SIMD by priority, then by age: the fold role is
    // pure VALU and would starve the two roles that alternate LDS round trips with short VALU bursts -- their latency chains
    // would then run AFTER the fold instead of beside it.  So the latency-bound roles get the oldest waves and a higher priority
    // (measured, ms per GiB, spec C / A: fold in the oldest waves and no priorities 0.440 / 0.592; priorities alone 0.390 /
    // 0.505; order alone 0.395 / 0.502; both 0.387 / 0.503; round 2's two-role kernel on the same box 0.387 / 0.532).
    const int role = 2 - (wave >> 2);                                   // 0 fold (waves 8..11), 1 pass 2 (4..7), 2 pass 3 + slicer (0..3)
    // (round 6, under the priorities below: the other wave orders of the three roles -- fold | pass 2 | slicer, fold | slicer | pass 2,
    // slicer | fold | pass 2, pass 2 | slicer | fold -- are within 1 % of this one: profiles/r06/prio_ab.txt)
    // Which role runs pass 3.  Behind the cheap slicers (specs B, C: 7 instructions per channel pair and frame) it shares the
    // slicer's waves; spec A's arctangent makes the slicer the longest chain of a time step (46 instructions per pair and
    // frame), so there pass 3 moves to the pass-2 waves (spec A 0.537 -> 0.517 ms, spec C 0.399 -> 0.414 if it moved too).
    // Spec D keeps pass 3 beside its slicer like specs B / C: either placement 0.413-0.421 ms, and its second channel pair sliced by
    // the pass-2 role's waves (which idle half a step) 0.425-0.428 against 0.420-0.428 -- the kernel is bound by VALU throughput, not
    // by one role's chain (profiles/EXPERIMENTS.md, round 4).
    constexpr bool P3_WITH_P2 = !IQ && SL == AMPS_SLICER_ATAN_BOXCAR;   // (handing one of the slicer's two channel pairs to the pass-2 role instead: 0.518 against 0.494)
    const int wf = wave & 3;                                            // frame of a half-batch this wave transforms (roles 1, 2)
    // Pass 3 produces the bins n = i (mod 64) from the points i + 64 r: a handle that decodes one channel group only needs the grp_w
    // residues of its group, so the four frames of a half-batch pack into 4 grp_w lanes: virtual lane v = 64 wf + lane transforms
    // residue i = grp_r grp_w + v % grp_w of frame v / grp_w (grp_w = 64: lane i of wave wf, frame wf, as ever)
    const uint32_t p3_v = 64u * (uint32_t)wf + (uint32_t)lane;
    const bool p3_on = p3_v < 4u * a.grp_w;
    const int p3_f = (int)(p3_v / a.grp_w) & 3, p3_i = (int)(a.grp_r * a.grp_w + p3_v % a.grp_w);
    // Priorities.  Rounds 3-5: pass 3 + slicer 2, pass 2 1, fold 0 (six other triples within the noise at D = 512 under specs A / C).  Round 6,
    // with the fold the longest chain of a step at either decimation (chz_timeline: 2575 of 3445 cycles at D = 768, the pass-2 role idle for
    // 1650): the FOLD ABOVE PASS 2 -- pass 3 + slicer 2, fold 1, pass 2 0 -- is 1.8-3.3 % faster under spec D at D = 768, 1.4-5 % under
    // B / C, 0.8-3.2 % at D = 512 (every triple with pass 2 lowest gains 2-3 %; profiles/r06/prio_ab.txt).  Spec A, whose pass-2 waves also
    // run pass 3, loses 4-8 % by it and keeps the old order, as does the unfused form.
    constexpr bool FOLD_OVER_P2 = !IQ && SL != AMPS_SLICER_ATAN_BOXCAR;
    constexpr int PRIO_PASS2 = FOLD_OVER_P2 ? 0 : 1, PRIO_FOLD = FOLD_OVER_P2 ? 1 : 0;
    if (role == 2) __builtin_amdgcn_s_setprio(2); else if (role == 1) __builtin_amdgcn_s_setprio(PRIO_PASS2); else __builtin_amdgcn_s_setprio(PRIO_FOLD);
    // The next launch's carry (the last L - D + 4 D samples and the leftover) is a ~80 KB copy: every workgroup moves its slice
    // here, a sample per thread of wave 0, instead of a kernel of its own behind this one (4.4 us + a launch gap per push).  Not
    // in the fold waves: their vmcnt windows count their own loads only.
    if (a.carry_out && wave == 0) {
        const uint32_t per = (a.carry_out_len + gridDim.x - 1) / gridDim.x;
        const uint32_t k0 = blockIdx.x * per;
        const uint32_t k1 = k0 + per < a.carry_out_len ? k0 + per : a.carry_out_len;
        for (uint32_t k = k0 + (uint32_t)lane; k < k1; k += 64)
            a.carry_out[k] = chz_carry_sample((const T *)a.block, a.carry, a.carry_len, a.nsamp, a.hist, a.consumed, k);
    }
    const int64_t f0 = (int64_t)blockIdx.x * a.frames_per_wg;   // multiple of 64
    if (f0 >= (int64_t)a.nframes) return;
    int64_t f1 = f0 + a.frames_per_wg; if (f1 > (int64_t)a.nframes) f1 = a.nframes;
    // the slicer state of every bin is rebuilt by two pre-roll half-batches; the first may reach behind the carry (zeros): it
    // only primes the delay lines for the second, which is exact (the carry holds L - D + 4 D samples)
    const int64_t fs = IQ ? f0 : f0 - CHZ_PREROLL;
    const int nh = (int)((f1 - fs + NB - 1) / NB);              // half-batches of this workgroup
    CHZ_TL_DECL;
    const int nsteps = nh + 3;                                    // time step i: fold h = i, pass 2 h = i - 1, pass 3 h = i - 2, slicer h = i - 3

    if (role == 0) {
        // ------------------------------------------------------------------ fold role
        const int t = tid & 255;
        const int64_t lead0 = (int64_t)a.carry_len - (int64_t)a.hist;
        const ChzIn<T> in{ (const T *)a.block, a.carry, (int64_t)a.hist, lead0, (int64_t)a.carry_len, (int64_t)a.nsamp };
        cf2 coef[4][P / 2];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int q = 0; q < P; q += 2) coef[j][q / 2] = (cf2){ a.taps[t + 256 * j + q * M], a.taps[t + 256 * j + (q + 1) * M] };
        cf2 tw1[3];                                               // pass 2's input twiddles of this thread's outputs k1 = 1..3
#pragma unroll
        for (int k1 = 1; k1 < 4; k1++) tw1[k1 - 1] = chz_twiddle((t >> 4) * k1, 64);
        if constexpr (DEC == CHZ_D768) {
        // ---- D = 768 (recc_chz_fold.hip.h, section "D = 768"): twelve ring slots per branch, three new samples per branch and half-step
        cf2 ring[4][CHZ768_R];
        {
            const int64_t vend = fs * D;                          // multiple of M (fs is a multiple of four)
#pragma unroll
            for (int jb = 0; jb < 4; jb++) {
                const int64_t vlast = vend - M + (t + 256 * jb);
#pragma unroll
                for (int q = 0; q < P; q++) ring[jb][q] = in.generic_nb(vlast - (int64_t)M * (P - 1 - q));
            }
        }
        chz768_prime(ring, in, fs, t);
        constexpr int PERIOD = 4;                                 // half-steps until the ring is back where it started (three slots per half-step, twelve slots)
        // half-step h loads frames of the half-steps h + 1 (from its third frame on) and h + 2: the fast loader is right once the
        // first frame of half-step h + 1 lies inside the new block
        // (The unfused form -- a checking mode -- runs every half-step as an edge step at this decimation: with its epilogue's row
        // addresses the kernel does not fit 168 registers, and what the compiler chose to spill were ring slots with a load in flight
        // -- it stores the stale value and reloads it behind the wait; tests/test_cpu_inflight_loads.py scans for exactly that.  One
        // drained batch of twelve loads per half-step is a third of the fast loader's speed, and the arithmetic is the same.)
        int h_edge = 0;
        if (IQ || in.nsamp < D) h_edge = nsteps;
        else if ((fs + NB) * D < in.lead) {
            const int64_t need = (in.lead + D - 1) / D - (fs + NB);
            h_edge = (int)((need + NB - 1) / NB);
            h_edge = (h_edge + PERIOD - 1) / PERIOD * PERIOD;
            if (h_edge > nsteps) h_edge = nsteps;
        }
        // the workgroup's descriptor starts at the first sample of its first FAST half-step (a few frames in front of the block, at the
        // most, for the workgroup that takes over from the carry: nothing down there is ever addressed); a range beyond 2^31 bytes -- a
        // 50 GB push -- keeps the bounds-checked loader
        const int64_t base_s = (fs + (int64_t)NB * h_edge) * D - in.lead;
        if ((int64_t)(nsteps - h_edge + 3) * NB * D * (int64_t)sizeof(T) >= (1ll << 31)) h_edge = nsteps;
        const chz_rsrc_t rsrc = chz_make_rsrc(in.block + base_s, (uint64_t)(in.nsamp - base_s) * sizeof(T));
        __syncthreads();                                          // all roles start together
        auto half_step = [&](auto basec, auto edgec, int h) {
            constexpr int BASE = decltype(basec)::value;
            constexpr bool EDGE = decltype(edgec)::value;
            CHZ_STAMP(h, 0);
            if (__builtin_expect(h < nh, 1)) {
                const int64_t F = fs + (int64_t)NB * h;
                cf2 *dst = buf + (h & (CHZ_SLOTS - 1)) * NB * CHZ_FB;
#if CHZ12_BODY_SHORT
                chz768_ring_wait<BASE, 0, !EDGE>(ring, h - h_edge);
#else
                chz768_ring_wait<BASE, 0>(ring);
#endif
                CHZ_STAMP(h, 1);
                if constexpr (EDGE) {
                    chz768_fold2_ring<P, BASE, 0>(ring, coef, tw1, dst, t, [] {});
                    chz768_fold2_ring<P, BASE, 2>(ring, coef, tw1, dst, t, [] {});
                    chz768_loads_generic<BASE>(ring, in, F, t);
                } else {
                    const uint32_t so = (uint32_t)(h - h_edge) * (uint32_t)(NB * D * sizeof(T));   // this half-step inside the workgroup's descriptor
                    chz768_fold2_ring<P, BASE, 0>(ring, coef, tw1, dst, t, [&] { chz768_loads_a<BASE>(ring, in, t, rsrc, so); });
#if CHZ12_BODY_SHORT
                    chz768_ring_wait<BASE, 2, true>(ring, h - h_edge);
#else
                    chz768_ring_wait<BASE, 2>(ring);
#endif
                    chz768_fold2_ring<P, BASE, 2>(ring, coef, tw1, dst, t, [&] { chz768_loads_b<BASE>(ring, in, t, rsrc, so); });
                }
                CHZ_STAMP(h, 2);
            }
            CHZ_STAMP(h, 3);
            __syncthreads();
            CHZ_STAMP(h, 4);
        };
        auto run_steps = [&](auto edgec, int hb, int he) __attribute__((always_inline)) {        // half-steps [hb, he); hb is a multiple of the ring's period
            for (int h = hb; h < he; h += PERIOD) {
                half_step(std::integral_constant<int, 0>{}, edgec, h);
                if (h + 1 >= he) break;
                half_step(std::integral_constant<int, 3>{}, edgec, h + 1);
                if (h + 2 >= he) break;
                half_step(std::integral_constant<int, 6>{}, edgec, h + 2);
                if (h + 3 >= he) break;
                half_step(std::integral_constant<int, 9>{}, edgec, h + 3);
            }
        };
        run_steps(std::true_type{}, 0, h_edge);
        if constexpr (!IQ) run_steps(std::false_type{}, h_edge, nsteps);
        } else {
        cf2 ring[4][P + 4];                                       // delay lines + the inputs of this and the next half-step
        {
            const int64_t vend = fs * D;                          // multiple of M (fs is even)
#pragma unroll
            for (int jb = 0; jb < 4; jb++) {
                const int64_t vlast = vend - M + (t + 256 * jb);
#pragma unroll
                for (int q = 0; q < P; q++) ring[jb][q] = in.generic_nb(vlast - (int64_t)M * (P - 1 - q));
            }
        }
        chz_load_half_ring<P, 0, P>(ring, in, fs, t);
        chz_load_half_ring<P, 0, P + 2>(ring, in, fs + NB, t);
        constexpr int PERIOD = (P + 4) / 2;                       // half-steps until the ring is back where it started (6)
        static_assert(PERIOD == 6, "the unrolled loop below is written for P = 8");
        // half-step h loads the frames of half-step h + 2: the fast loader is right once those lie inside the new block
        int h_edge = 0;
        if (in.nsamp < D) h_edge = nsteps;
        else if ((fs + 2 * NB) * D < in.lead) {
            const int64_t need = (in.lead + D - 1) / D - (fs + 2 * NB);           // frames from the first loaded one to the first inside the block
            h_edge = (int)((need + NB - 1) / NB);
            h_edge = (h_edge + PERIOD - 1) / PERIOD * PERIOD;
            if (h_edge > nsteps) h_edge = nsteps;
        }
        // the workgroup's descriptor (chz_make_rsrc) starts at the first sample of its first FAST half-step; a range beyond 2^31 bytes keeps the bounds-checked loader
        const int64_t base_s = (fs + (int64_t)NB * h_edge) * D - in.lead;
        if ((int64_t)(nsteps - h_edge + 3) * NB * D * (int64_t)sizeof(T) >= (1ll << 31)) h_edge = nsteps;
        const chz_rsrc_t rsrc = chz_make_rsrc(in.block + base_s, (uint64_t)(in.nsamp - base_s) * sizeof(T));
        __syncthreads();                                          // all roles start together 
        // one half-step = four frames: fold them, then load the frames of the half-step after next into the two slots that
        // just died.  A load has eight frames (~3 us) to arrive: with four frames of lead the fold waves were the critical path
        // (4 waves x 8 loads x 512 B = 16 KB in flight per CU do not cover the HBM latency under load).
        // One half-step = four frames.  EDGE half-steps (the head of a launch, where the inputs still come from the carry of the
        // previous push, and pushes shorter than a frame) load with ordinary, bounds-checked loads BEHIND the fold and drain them
        // at once; all others prefetch with untracked asm loads (chz_load1_ring) that go into the ring slots as they die, as early
        // in the step as possible: the oldest slot of branches 0, 1 is not read at all in this half-step; the oldest of branches
        // 2, 3 and the second-oldest of branches 0, 1 are last read by the first tap block of frames 0 / 1; the second-oldest of
        // branches 2, 3 by the first tap block of frame 2.  A load then has almost two time steps to land and is issued beside the
        // other roles' VALU work.  The two kinds never meet inside one loop body: a control-flow join behind an untracked load
        // invites the compiler to copy a register whose load is still in flight (it did; tests/test_cpu_inflight_loads.py scans
        // the assembly for that).
        auto half_step = [&](auto basec, auto edgec, int h) {
            constexpr int BASE = decltype(basec)::value;
            constexpr bool EDGE = decltype(edgec)::value;
            CHZ_STAMP(h, 0);
            if (__builtin_expect(h < nh, 1)) {
                const int64_t F = fs + (int64_t)NB * h;
                cf2 *dst = buf + (h & (CHZ_SLOTS - 1)) * NB * CHZ_FB;
#if CHZ12_BODY_SHORT
                chz_ring_wait<P, BASE, !EDGE>(ring, h >= h_edge + 2);
#else
                chz_ring_wait<P, BASE>(ring);
#endif
                CHZ_STAMP(h, 1);
                if constexpr (EDGE) {
                    chz_fold2_ring<P, BASE, 0>(ring, coef, tw1, dst, t, [] {});
                    chz_fold2_ring<P, BASE, 2>(ring, coef, tw1, dst, t, [] {});
                    chz_load_half_ring<P, BASE, P + 4>(ring, in, F + 2 * NB, t);
                } else {
                    const uint32_t so = (uint32_t)(h - h_edge) * (uint32_t)(NB * D * sizeof(T));   // this half-step inside the workgroup's descriptor
                    chz_load1_ring<P, BASE, P + 4, 0>(ring, in, t, rsrc, so);
                    chz_fold2_ring<P, BASE, 0>(ring, coef, tw1, dst, t, [&] {
                        chz_load1_ring<P, BASE, P + 4, 1>(ring, in, t, rsrc, so);
                        chz_load1_ring<P, BASE, P + 4, 2>(ring, in, t, rsrc, so);
                    });
                    chz_fold2_ring<P, BASE, 2>(ring, coef, tw1, dst, t, [&] { chz_load1_ring<P, BASE, P + 4, 3>(ring, in, t, rsrc, so); });
                }
                CHZ_STAMP(h, 2);
            }
            CHZ_STAMP(h, 3);
            __syncthreads();
            CHZ_STAMP(h, 4);
        };
        auto run_steps = [&](auto edgec, int hb, int he) __attribute__((always_inline)) {        // half-steps [hb, he); hb is a multiple of the ring's period
            for (int h = hb; h < he; h += PERIOD) {
                half_step(std::integral_constant<int, 0>{}, edgec, h);
                if (h + 1 >= he) break;
                half_step(std::integral_constant<int, 2>{}, edgec, h + 1);
                if (h + 2 >= he) break;
                half_step(std::integral_constant<int, 4>{}, edgec, h + 2);
                if (h + 3 >= he) break;
                half_step(std::integral_constant<int, 6>{}, edgec, h + 3);
                if (h + 4 >= he) break;
                half_step(std::integral_constant<int, 8>{}, edgec, h + 4);
                if (h + 5 >= he) break;
                half_step(std::integral_constant<int, 10>{}, edgec, h + 5);
            }
        };
        run_steps(std::true_type{}, 0, h_edge);
        run_steps(std::false_type{}, h_edge, nsteps);
        }
        CHZ_TL_FLUSH;
    } else if (role == 1) {
        // ------------------------------------------------------------------ pass-2 role (+ pass 3 when P3_WITH_P2)
        cf2 tw3[P3_WITH_P2 ? 15 : 1];                             // twiddles of the second radix-16 pass: W_1024^{r lane}
        if constexpr (P3_WITH_P2) {
#pragma unroll
            for (int r = 1; r < 16; r++) tw3[r - 1] = chz_twiddle(r * p3_i, 1024);
        }
        __syncthreads();                                          // all roles start together 
        {
            for (int i = 0; i < nh + 3; i++) {
                const int h = i - 1, h3 = i - 2;
                CHZ_STAMP(i, 0);
                if (h >= 0 && h < nh) chz_p2(buf + ((h & (CHZ_SLOTS - 1)) * NB + wf) * CHZ_FB, lane);
                CHZ_STAMP(i, 1);
                if constexpr (P3_WITH_P2) { if (h3 >= 0 && h3 < nh && p3_on) chz_p3(buf + ((h3 & (CHZ_SLOTS - 1)) * NB + p3_f) * CHZ_FB, tw3, p3_i); }
                CHZ_STAMP(i, 3);
                __syncthreads();
                CHZ_STAMP(i, 4);
            }
        }
        CHZ_TL_FLUSH;
    } else {
        // ------------------------------------------------------------------ pass-3 + slicer role
        cf2 tw3[P3_WITH_P2 ? 1 : 15];                             // twiddles of the second radix-16 pass: W_1024^{r lane}
        if constexpr (!P3_WITH_P2) {
#pragma unroll
            for (int r = 1; r < 16; r++) tw3[r - 1] = chz_twiddle(r * p3_i, 1024);
        }
        ChzSlicer<SL, IQ, SPS> slicer;
        slicer.init(a, wf, lane);
        __syncthreads();                                          // all roles start together 
        {
            // time step i slices half-batch hs = i - 3 and transforms h3 = i - 2.  STEADY steps -- 2 <= hs <= nh - 2: real frames, not
            // the range's last half-batch, h3 inside the range -- run without any of the rare-case tests (ChzSlicer::half<1 / 2>);
            // a 32-frame word completes when hs = 1 (mod 8), i.e. in the last step of every group of eight that starts at i = 5
            auto step = [&](auto kindc, auto parc, int i) __attribute__((always_inline)) {
                constexpr int KIND = decltype(kindc)::value, PAR = decltype(parc)::value;   // PAR = i & 1
                const int hs = i - 3, h3 = i - 2;
                CHZ_STAMP(i, 0);
                if (KIND != 0 || (hs >= 0 && hs < nh)) slicer.template half<KIND, PAR>(a, buf, fs, f0, f1, hs);
                CHZ_STAMP(i, 1);
                if constexpr (!P3_WITH_P2) { if ((KIND != 0 || (h3 >= 0 && h3 < nh)) && p3_on) chz_p3(buf + ((h3 & (CHZ_SLOTS - 1)) * NB + p3_f) * CHZ_FB, tw3, p3_i); }
                CHZ_STAMP(i, 3);
                __syncthreads();
                CHZ_STAMP(i, 4);
            };
            constexpr int I_FIRST = IQ ? 3 + 2 : 5;               // first steady step (hs = 2); ODD, and a group is eight steps: the parities below
            static_assert((I_FIRST & 1) == 1, "parity of the steady groups");
            const int i_last = nh + 1;                            // last steady step (hs = nh - 2, h3 = nh - 1)
            using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>; using K2 = std::integral_constant<int, 2>;
            using P0 = std::integral_constant<int, 0>; using P1 = std::integral_constant<int, 1>;
            // Every step's parity is a compile-time constant, the edge steps' too: a run-time parity at either end would keep BOTH
            // frame buffers of the slicer alive across the whole steady loop (24 VGPRs: measured as spills in the word step, +10 %).
            int i = 0;
            static_assert(I_FIRST == 5, "the five edge steps in front of the steady groups are written out");
            if (i < nsteps) { step(K0{}, P0{}, i); i++; }
            if (i < nsteps) { step(K0{}, P1{}, i); i++; }
            if (i < nsteps) { step(K0{}, P0{}, i); i++; }
            if (i < nsteps) { step(K0{}, P1{}, i); i++; }
            if (i < nsteps) { step(K0{}, P0{}, i); i++; }
            while (i + 7 <= i_last) {
                // seven plain steps and the one that completes a word; two steps per loop round so that the time step's parity -- which
                // of the slicer's two frame buffers is written -- is a compile-time constant (all eight as straight-line code: 15
                // spilled VGPRs)
#pragma unroll 1
                for (int k = 0; k < 6; k += 2) { step(K1{}, P1{}, i + k); step(K1{}, P0{}, i + k + 1); }
                step(K1{}, P1{}, i + 6);
                step(K2{}, P0{}, i + 7);
                i += 8;
            }
            // (i is odd here -- I_FIRST + 8 n -- or the range was shorter than the five edge steps and nothing is left)
            while (i < nsteps) {
                step(K0{}, P1{}, i); i++;
                if (i >= nsteps) break;
                step(K0{}, P0{}, i); i++;
            }
        }
        CHZ_TL_FLUSH;
    }
