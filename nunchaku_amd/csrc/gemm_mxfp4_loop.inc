// The body gemm_mxfp4.hip's kernels share, from the staging plan to the low-rank-up MFMAs: behind it acc[ni][mi] holds the fp32 product plus the
// low-rank term of the wave's 64 x 128 outputs (element i of lane (r, h): row 64 wave + 32 mi + r, column 32 ni + 8 (i >> 2) + 4 h + (i & 3)).
// A fragment of a kernel body, not a function: moved into one, the plain kernel's register allocation is the compiler's to change.  It expects in
// scope DT, T, V8 and `p` (Mxfp4GemmParams or a struct derived from it); it leaves tid, wave, lane, r, h, TN, bm, bn, m0, n0 and acc behind.
// The weight-side row (of wgt, wscales, lora_up) behind tile column c is MX_WBASE + c + MX_WSKIP(c): n0 + c unless the including kernel defines
// the two macros (the rows of one 32-column accumulator tile must be consecutive).  Both are undefined again at the end of this file.
#ifndef MX_WBASE
#define MX_WBASE n0
#define MX_WSKIP(c) 0
#endif
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * MX_STAGE];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int TN = p.N / MX_TN;
    const int bm = blockIdx.x / TN, bn = blockIdx.x % TN;
    const int m0 = bm * MX_TM, n0 = bn * MX_TN;
    const int KB = p.K / 2, KS = p.K / 128;

    // ---- DMA plan: position pos = 64 i + lane of a tile holds row pos >> 2, slot pos & 3 = block (slot ^ ((row >> 2) & 3)); the A tile is 16
    //      wave instructions (4 a wave), the B tile 8 (2 a wave).  Offsets are range-checked 32-bit byte offsets (validated on the host).
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void *)p.act, 0, (int)((size_t)p.M_pad * KB), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void *)p.wgt, 0, (int)((size_t)p.N * KB), 0x00020000);
    unsigned va[4], vw[2];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned pos = (unsigned)(wave * 4 + j) * 64u + lane, row = pos >> 2, blk = (pos & 3u) ^ ((row >> 2) & 3u);
        va[j] = (unsigned)(m0 + row) * (unsigned)KB + blk * 16u;
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const unsigned pos = (unsigned)(wave * 2 + j) * 64u + lane, row = pos >> 2, blk = (pos & 3u) ^ ((row >> 2) & 3u);
        vw[j] = (unsigned)(MX_WBASE + row + MX_WSKIP(row)) * (unsigned)KB + blk * 16u;
    }
    auto stage_dma = [&](int ks, int buf) {
        mx_lds_u8 *S = (mx_lds_u8 *)lds + buf * MX_STAGE;
#pragma unroll
        for (int j = 0; j < 4; j++) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (mx_lds_void *)(S + (wave * 4 + j) * 1024), 16, va[j], ks * 64, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; j++) __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (mx_lds_void *)(S + MX_A_BYTES + (wave * 2 + j) * 1024), 16, vw[j], ks * 64, 0, 0);
    };
    // the scale dwords of K-step ks: lane (r, h) takes those of its own rows / columns; behind the step's wait it moves block h to byte 0 (block 2 + h to byte 2)
    const uint32_t *sa_ptr = p.ascales + m0 + wave * 64 + r, *sw_ptr = p.wscales + MX_WBASE + r;
    auto load_scales = [&](int ks, unsigned (&sa)[2], unsigned (&sw)[4]) {
#pragma unroll
        for (int mi = 0; mi < 2; mi++) sa[mi] = sa_ptr[(size_t)ks * p.M_pad + 32 * mi];
#pragma unroll
        for (int ni = 0; ni < 4; ni++) sw[ni] = sw_ptr[(size_t)ks * p.N + 32 * ni + MX_WSKIP(32 * ni)];
    };

    v16f acc[4][2];
#pragma unroll
    for (int ni = 0; ni < 4; ni++)
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[ni][mi][i] = 0.f;

    // fragment addresses inside a stage: rows 64 wave + 32 mi + r of A, 32 ni + r of B; (row >> 2) & 3 = (r >> 2) & 3 for both
    const unsigned sw3 = ((unsigned)r >> 2) & 3u;
    const unsigned fa = (unsigned)(wave * 64 + r) * 64u, fb = (unsigned)MX_A_BYTES + (unsigned)r * 64u;

    unsigned sa_n[2], sw_n[4];
    load_scales(0, sa_n, sw_n);
    stage_dma(0, 0);
    for (int ks = 0; ks < KS; ks++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's part of step ks has landed ...
        __syncthreads();                                 // ... and everybody's; every wave is done reading the other buffer
        unsigned sa[2], sw[4];
#pragma unroll
        for (int i = 0; i < 2; i++) { asm volatile("" : "+v"(sa_n[i])); sa[i] = sa_n[i] >> (8 * h); } // (pinned behind the wait: hoisted into the previous step, the
#pragma unroll
        for (int i = 0; i < 4; i++) { asm volatile("" : "+v"(sw_n[i])); sw[i] = sw_n[i] >> (8 * h); } //  shifts put an s_waitcnt vmcnt(6) between that step's MFMAs)
        if (ks + 1 < KS) { // block-uniform; the scale loads first, so that a wait for them leaves the six DMA instructions in flight: hipcc copies the loaded
                           // dwords into their loop-carried registers behind the step's 10th to 14th MFMA (s_waitcnt vmcnt(11) / (9) / (6))
            load_scales(ks + 1, sa_n, sw_n);
            stage_dma(ks + 1, (ks + 1) & 1);
        }
        const mx_lds_u8 *S = (const mx_lds_u8 *)lds + (ks & 1) * MX_STAGE;
        auto extent = [&](auto kk_c) { // one MFMA K-extent of 64 channels: the lane's block is 2 kk + h (kk is an immediate: op_sel)
            constexpr int kk = decltype(kk_c)::value;
            const unsigned slot = (((unsigned)(2 * kk + h)) ^ sw3) << 4;
            v8i a[2], b[4];
#pragma unroll
            for (int mi = 0; mi < 2; mi++) {
                const v4i t = *(const mx_lds_v4i *)(S + fa + mi * 2048 + slot);
                a[mi] = v8i{t[0], t[1], t[2], t[3], 0, 0, 0, 0};
            }
#pragma unroll
            for (int ni = 0; ni < 4; ni++) {
                const v4i t = *(const mx_lds_v4i *)(S + fb + ni * 2048 + slot);
                b[ni] = v8i{t[0], t[1], t[2], t[3], 0, 0, 0, 0};
            }
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int mi = 0; mi < 2; mi++) // D[n][m]: the weights are the first operand, so a lane ends up with 4 neighbouring columns of one row
                    acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[ni][mi], 4, 4, 2 * kk, (int)sw[ni], 2 * kk, (int)sa[mi]);
        };
        extent(std::integral_constant<int, 0>{});
        extent(std::integral_constant<int, 1>{});
    }

    // ---- epilogue.  Low rank on the 16-bit MFMA, 16 ranks at a time in ascending order, with gemm_w4a4's rounding point: round16(lora_act * scale)
    const int Rr = p.R;
    if (Rr > 0) {
        const float *la_base = p.lora_act + (size_t)(m0 + wave * 64 + r) * Rr + 8 * h;
        const T *lu_base = (const T *)p.lora_up + (size_t)(MX_WBASE + r) * Rr + 8 * h;
        for (int rc = 0; rc < Rr; rc += 16) {
            const float sc = p.lora_scales[rc >> 4];
            V8 la[2], lu[4];
#pragma unroll
            for (int mi = 0; mi < 2; mi++) {
                const v4f x0 = *reinterpret_cast<const v4f *>(la_base + (size_t)mi * 32 * Rr + rc);
                const v4f x1 = *reinterpret_cast<const v4f *>(la_base + (size_t)mi * 32 * Rr + rc + 4);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    la[mi][j] = f2h<T>(sc == 1.0f ? x0[j] : x0[j] * sc);
                    la[mi][4 + j] = f2h<T>(sc == 1.0f ? x1[j] : x1[j] * sc);
                }
            }
#pragma unroll
            for (int ni = 0; ni < 4; ni++) lu[ni] = *reinterpret_cast<const V8 *>(lu_base + (size_t)(ni * 32 + MX_WSKIP(32 * ni)) * Rr + rc);
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[ni][mi] = Half<DT>::mfma32(lu[ni], la[mi], acc[ni][mi]);
        }
    }
#undef MX_WBASE
#undef MX_WSKIP
