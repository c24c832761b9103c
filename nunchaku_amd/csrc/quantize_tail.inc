// A fragment of a tile quantiser's kernel body (quantize_tail.h says what it expects in scope).  #define QUANT_TAIL_PART 1 | 2 | 3 before each include.
#if QUANT_TAIL_PART == 1
    v2i xv[2][8]; // the lane's record: row r, channels 64 grp + 8 tc + 4 h + e
#pragma unroll
    for (int i = 0; i < 16; i++) xv[i >> 3][i & 7] = v2i{0, 0};
    unsigned ldo[4] = {0, 0, 0, 0}; // lora_down slab offsets of DMA instructions i = j, j + 4 (rank 4j + lane / 16 [+ 16]; the swizzle only depends on j)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned rank = 4 * j + (lane >> 4);
        ldo[j] = (rank * (unsigned)K + kp * 128 + (((lane & 15) ^ (rank & 15)) * 8)) * 2u;
    }
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void *)p.lora_down, 0, (int)((size_t)p.R * K * 2), 0x00020000);
    auto slab_dma = [&](int rank0) { // ranks rank0 .. rank0 + 31 of this chunk's channels -> the tile region; ranks >= R lie beyond the descriptor's range and read as zero
#pragma unroll
        for (int i = 0; i < 8; i++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rl, (lds_void *)(W + i * 1024), 16, ldo[i & 3] + ((i >> 2) * 16 + rank0) * K * 2, 0, 0, 0);
    };

#elif QUANT_TAIL_PART == 2
        // (one wave, in-order LDS: its reads below see its own writes; no workgroup barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- 3. back in record layout: 8 bytes (half h) of piece 8 grp + tc of row r
#pragma unroll
        for (int grp = 0; grp < 2; grp++)
#pragma unroll
            for (int tc = 0; tc < 8; tc++) xv[grp][tc] = *(const lds_v2i *)(W + r * 256 + (((grp * 8 + tc) ^ (r & 15)) << 4) + 8 * h);
        if (p.R > 0) { // the tile is in registers: its LDS takes the first slab of lora_down while the groups below are quantised
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            slab_dma(0);
        }

#ifndef QUANT_TAIL_READBACK_ONLY // (a kernel with a block quantiser of its own takes step 3 alone)
        // ---- 4. the two groups of the chunk: the quantiser of quantize.hip, expression for expression
        uint8_t *dst = p.act + ((size_t)rt * KP + kp) * F6_CHUNK + (size_t)lane * 16;
#pragma unroll
        for (int grp = 0; grp < 2; grp++) {
            v16f ev, od; // elements 0,2 / 1,3 of the lane's eight 4-channel pieces = the two sources of the FP6 pack
            float amax = 0.f;
#pragma unroll
            for (int tc = 0; tc < 8; tc++) {
                v4f rs = {};
                if constexpr (SMOOTH) rs = *(const lds_v4f *)(W + QG_TILE_BYTES + (grp * 64 + 8 * tc + 4 * h) * 4);
                float xf[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    xf[e] = h2f(hfrom<T>((unsigned short)((unsigned)xv[grp][tc][e >> 1] >> (16 * (e & 1)))));
                    if constexpr (SMOOTH) xf[e] = smooth_div16<T>(xf[e], rs[e]);
                    amax = fmaxf(amax, fabsf(xf[e]));
                }
                ev[2 * tc] = xf[0]; ev[2 * tc + 1] = xf[2];
                od[2 * tc] = xf[1]; od[2 * tc + 1] = xf[3];
            }
            amax = fmaxf(amax, __shfl_xor(amax, 32));
            const float scale = amax * (1.0f / 7.0f);
            const float rscale = scale == 0.f ? 0.f : 1.0f / scale;
#pragma unroll
            for (int i = 0; i < 16; i++) { // NaN (a NaN element, or inf * 0 in a group holding inf) -> code 0, as in quantize.hip
                ev[i] = nan_to_zero(ev[i] * rscale);
                od[i] = nan_to_zero(od[i] * rscale);
            }
            const v6i pk = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(ev, od, 8.0f);
            if (grp == 0) {
                *reinterpret_cast<uint4 *>(dst) = make_uint4((unsigned)pk[0], (unsigned)pk[1], (unsigned)pk[2], (unsigned)pk[3]);
                *reinterpret_cast<uint2 *>(dst + F6_PLANE) = make_uint2((unsigned)pk[4], (unsigned)pk[5]);
            } else {
                *reinterpret_cast<uint2 *>(dst + F6_PLANE + 8) = make_uint2((unsigned)pk[0], (unsigned)pk[1]);
                *reinterpret_cast<uint4 *>(dst + 2 * F6_PLANE) = make_uint4((unsigned)pk[2], (unsigned)pk[3], (unsigned)pk[4], (unsigned)pk[5]);
            }
            // S image: [rt][kp][grp][32]; lane (r, h) writes group h
            if (h == grp) ((T *)p.ascales)[(((size_t)rt * KP + kp) * 2 + grp) * 32 + r] = f2h<T>(scale);
        }
#endif

#elif QUANT_TAIL_PART == 3
    // ---- 5. low rank, one 32-rank slab at a time: 8 MFMAs per wave (pieces 2q, 2q + 1 of every lane are k-slots 8h .. 8h + 7), the four waves' tiles
    //         parked in their own regions and summed by wave 0 in a fixed order; atomics only between workgroups
    for (int rank0 = 0; rank0 < p.R; rank0 += 32) { // block-uniform
        v16f acc;
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 0.f;
        if (active) {
            if (rank0 > 0) slab_dma(rank0); // (the barrier that closed the previous round has freed the region)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int grp = 0; grp < 2; grp++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int piece = grp * 8 + 2 * q;
                    const v2i b0 = *(const lds_v2i *)(W + r * 256 + ((piece ^ (r & 15)) << 4) + 8 * h);
                    const v2i b1 = *(const lds_v2i *)(W + r * 256 + (((piece + 1) ^ (r & 15)) << 4) + 8 * h);
                    const V8 a = __builtin_bit_cast(V8, v4i{xv[grp][2 * q][0], xv[grp][2 * q][1], xv[grp][2 * q + 1][0], xv[grp][2 * q + 1][1]});
                    const V8 b = __builtin_bit_cast(V8, v4i{b0[0], b0[1], b1[0], b1[1]});
                    acc = Half<DT>::mfma32(a, b, acc);
                }
        }
        *(lds_v16f *)(W + lane * 64) = acc; // (behind this wave's own slab reads: in-order LDS)
        __syncthreads();
        if (wave == 0) {
            const lds_u8 *B = (const lds_u8 *)lds + lane * 64;
            const v16f s = ((*(const lds_v16f *)(B) + *(const lds_v16f *)(B + QG_WAVE_BYTES)) + *(const lds_v16f *)(B + 2 * QG_WAVE_BYTES)) +
                           *(const lds_v16f *)(B + 3 * QG_WAVE_BYTES);
            if (rank0 + r < p.R) { // C layout: col (rank) = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int m = rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    lora_act_add(p.lora_act, (size_t)m * p.R + rank0 + r, s[i], p.mode);
                }
            }
        }
        __syncthreads();
    }
#endif
#undef QUANT_TAIL_PART
