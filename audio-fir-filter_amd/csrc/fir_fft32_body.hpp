// fir_fft32_body.hpp -- the body of fir_fft32_f64_kernel and of
// fir_fft32_items_parts_kernel (fir_fft32.hpp), included inside each kernel's
// braces: no include guard, nothing at namespace scope.  In scope: the
// kernel's parameters (p, pair, tw, task, B, gd, c8, items), kOut and kItem.
    extern __shared__ double2 flds[];
    double2 *twl = flds + kFftM; // the kFft32Tw twiddles, LDS-resident
    for (int i = threadIdx.x; i < kFft32Tw; i += kFftNT) twl[i] = tw[i];
    {
        const int u = fft_unit32(0, blockIdx.x, gridDim.x, gd.units);
        DirectParams iv;
        int c;
        int64_t n0;
        fft_unit_decode<kItem>(p, gd, items, u, B, iv, c, n0);
        fft32_stage_samples(kItem ? iv : p, c, n0, threadIdx.x, flds);
    }
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    __syncthreads();
    const uint32_t tkE = task[threadIdx.x], tkO = task[kFftNT + threadIdx.x];
    const double2 *pairO = pair + kFftPairTable;
    float pk_run = 0.0f;
    int pk_ch = -1;
    float *pk_lds = reinterpret_cast<float *>(twl + kFft32Tw);
    int pk_pending = -1;
    int rnd = 0;
    for (int u = fft_unit32(0, blockIdx.x, gridDim.x, gd.units); u < gd.units;
         u = fft_unit32(++rnd, blockIdx.x, gridDim.x, gd.units)) {
        int j = threadIdx.x;
        asm volatile("" : "+v"(j));
        const int w = j >> 6, lane = j & 63;
        DirectParams iv; // kItem: this unit's view of the launch
        int ch;
        int64_t n0;
        fft_unit_decode<kItem>(p, gd, items, u, B, iv, ch, n0);
        const DirectParams &pu = kItem ? iv : p;
        double2 park[16]; // the half that is not in LDS: O's stage-1 values, then E's outputs
        double2 *pb = p.park + (size_t)blockIdx.x * kParkSlab * kFftNT + j; // this thread's slab entries
        FFT32_STAMP(0);

        // ---- stage 1: the samples out of the LDS image (the previous unit's
        // final phase staged them), the radix-2 split, both halves' 16-point
        // DFTs (half E into LDS, half O to the slab)
        {
            // (the staging transfers retired before the previous unit's stores)
            const float2 *fz = reinterpret_cast<const float2 *>(flds);
            float2 v[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) v[r] = fz[fft32_zidx(r, w, lane)];
            double2 a[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                a[r] = make_double2((double)v[r].x + (double)v[r + 16].x, (double)v[r].y + (double)v[r + 16].y);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                park[r] = w32mul(make_double2((double)v[r].x - (double)v[r + 16].x,
                                              (double)v[r].y - (double)v[r + 16].y), r);
            dft16(a);
            twiddle16(a, twl[j]); // W_8192^(j c)
            // every lane of the wave has read its samples (same wave, issue order)
#pragma unroll
            for (int c = 0; c < 16; ++c) flds[512 * fft_slot(c) + j] = a[c];
            dft16(park);
            const double2 w1 = twl[kFft32TwOdd + j]; // W_16384^j
#pragma unroll
            for (int r = 0; r < 16; ++r) park[r] = cmul(park[r], w1);
            twiddle16(park, twl[j]); // W_8192^(j c)
#pragma unroll
            for (int r = kParkRegs; r < 16; ++r) pb[(r - kParkRegs) * kFftNT] = park[r];
        }
        FFT32_STAMP(1);
        __syncthreads();
        FFT32_STAMP(2);
        if (pk_pending >= 0) {
            if (threadIdx.x == 0) fft_peak_commit(pu, pk_pending, pk_lds);
            pk_pending = -1;
        }

        // ---- half E: the even bins (fresh indices: the column phase's
        // addresses die with it instead of living across both halves)
        {
            int jc = threadIdx.x;
            uint32_t tk = tkE;
            asm volatile("" : "+v"(jc), "+v"(tk));
            fft_columns<kOut, false>(flds, twl, pair, tk, c8, false, jc, rnd, [] {});
        }
        FFT32_STAMP(3);
        // the parked half O values back, in flight across the barrier wait
        // and the swap's first DFT
#pragma unroll
        for (int r = kParkRegs; r < 16; ++r) park[r] = pb[(r - kParkRegs) * kFftNT];
        __syncthreads();
        FFT32_STAMP(4);

        // ---- swap: half E's inverse columns out of LDS and through their
        // final 16-point DFTs, then half O's stage-1 values in (thread j's own
        // addresses: no barrier between the reads and the writes)
        {
            double2 a[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = flds[512 * fft_slot(c) + j];
            twiddle16(a, twl[j]); // W_8192^(j c)
            dft16(a);
#pragma unroll
            for (int c = 0; c < 16; ++c) flds[512 * fft32_slot_odd(c) + j] = park[c];
#pragma unroll
            for (int r = 0; r < 16; ++r) park[r] = a[r]; // E[j + 512 r]
#pragma unroll
            for (int r = kParkRegs; r < 16; ++r) pb[(r - kParkRegs) * kFftNT] = park[r];
        }
        FFT32_STAMP(5);
        __syncthreads();
        FFT32_STAMP(6);

        // ---- half O: the odd bins
        {
            int jc = threadIdx.x;
            uint32_t tk = tkO;
            asm volatile("" : "+v"(jc), "+v"(tk));
            fft_columns<kOut, false>(flds, twl, pairO, tk, c8, true, jc, rnd, [] {});
        }
        FFT32_STAMP(7);
        // half E's outputs back from the slab, in flight across the barrier wait
#pragma unroll
        for (int r = kParkRegs; r < 16; ++r) park[r] = pb[(r - kParkRegs) * kFftNT];
        __syncthreads();
        FFT32_STAMP(8);

        // ---- final: half O's columns out of LDS; the next unit's samples
        // into the freed blocks (unconditional -- the last unit restages
        // itself -- so the waits below count the same instructions on every
        // path); half O's 16-point DFTs, W_32^a, the radix-2 merge, stores
        double2 a[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) a[c] = flds[512 * fft32_slot_odd(c) + j];
        const double2 wj = twl[j], w1 = twl[kFft32TwOdd + j]; // W_8192^j, W_16384^j
        // vmcnt(0) lgkmcnt(0): the wave's reads of its blocks have retired, and
        // so have half E's slab reloads -- the compiler does not count LDS-DMA
        // in vmcnt, so a wait it placed for them after the transfers below
        // would also wait for the transfers
        __builtin_amdgcn_s_waitcnt(0x0070);
        {
            const int un1 = fft_unit32(rnd + 1, blockIdx.x, gridDim.x, gd.units);
            const int un = un1 < gd.units ? un1 : u;
            DirectParams nv; // kItem: the next unit's view (another row, file or group)
            int cn;
            int64_t nn;
            fft_unit_decode<kItem>(p, gd, items, un, B, nv, cn, nn);
            fft32_stage_samples(kItem ? nv : p, cn, nn, j, flds);
        }
        FFT32_STAMP(9);
        twiddle16(a, wj); // W_8192^(j c)
        dft16(a);
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = w32mul(cmul(a[r], w1), r);
        // the staging transfers have had the DFTs to land; waiting here, not
        // at the loop head, keeps the output stores out of the wait (the
        // compiler neither counts LDS-DMA in vmcnt nor orders it before LDS
        // reads: this explicit wait is what stage 1's reads rely on)
        __builtin_amdgcn_s_waitcnt(kVmcnt0);
        FFT32_STAMP(10);
        const float pk = fft32_store_unit<kOut>(pu, ch, n0, B, j, park, a);
        if (ch != pk_ch) {
            if (pu.peak && pk_ch >= 0) {
                fft_peak_stage(pk_lds, pk_run);
                pk_pending = pk_ch;
                asm volatile("" : "+v"(pk_pending));
            }
            pk_run = 0.0f;
            pk_ch = ch;
        }
        pk_run = fmaxf(pk_run, pk);
        FFT32_STAMP(11);
    }
    // the last unit's restaging transfer must land before the LDS is released
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    if (!kItem && p.peak && pk_ch >= 0) { // the item form has no fused peak (items_peak_kernel)
        __syncthreads();
        if (pk_pending >= 0 && threadIdx.x == 0) fft_peak_commit(p, pk_pending, pk_lds);
        __syncthreads();
        fft_peak_stage(pk_lds, pk_run);
        __syncthreads();
        if (threadIdx.x == 0) fft_peak_commit(p, pk_ch, pk_lds);
    }
