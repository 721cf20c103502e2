// patch_embed_body.inc — the statements of the patch embedding kernels (encoder.hip, K1), included once into each of them.
// The including kernel provides: the template argument CPT; `constexpr bool GRAY` (the pixel source: gray bytes [B,S,S], or
// fp32 planes [B,3,S,S]); the pointers img (fp32 source) and gray (byte source), of which it reads one; `NormConsts nc` (read
// when GRAY); and w_t, bias, gamma, beta, x, S, G, rpw. One text for both kernels, so that they cannot drift — and included,
// not called: wrapped into an inlined __device__ function the same statements are optimised once on their own and again after
// inlining, and patch_embed_kernel<CPT> came out with another schedule (the library is checked for byte-reproducibility).
    constexpr int C = 8 * CPT;
    constexpr int PW = 128 * PE_NP;             // pixels per staged line
    constexpr int WS = C + 4;                   // weight row stride in LDS
    constexpr bool SWZ = CPT == 16;             // parts 4..7 (channels 64..127) stored 4 floats later
    constexpr int NWQ = (12 * C + 255) / 256;   // weight quads per thread
    constexpr int NPQ = GRAY ? 1 : (12 * (PW / 4) + 255) / 256;
    constexpr int NGQ = GRAY ? (4 * (PW / 4) + 255) / 256 : 1;   // gray source: dwords (4 pixels of one line) per thread
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* wt = sm;             // [48][WS]
    float* pix = sm + 48 * WS;  // [3][4][PW]
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int p = tid >> 3, part = tid & 7;
    const int c0 = part * CPT;
    f32x4 wq[NWQ];
#pragma unroll
    for (int k = 0; k < NWQ; ++k) wq[k] = ((const f32x4*)w_t)[min(tid + 256 * k, 12 * C - 1)];
    // a workgroup takes `rpw` consecutive patch rows (round 6: two at G % 2 == 0 — the 24 KB of weights are staged once per
    // workgroup, a quarter of what a patch row moves into the CU) in chunks of 96 patches; per output nothing changes
    const int nchunk = (G + 32 * PE_NP - 1) / (32 * PE_NP);
    for (int ch = 0; ch < rpw * nchunk; ++ch) {
        const int py = blockIdx.x * rpw + ch / nchunk, px0 = (ch % nchunk) * 32 * PE_NP;
        f32x4 pq[NPQ];
        uint32_t gq[NGQ];
        if constexpr (GRAY) {
#pragma unroll
            for (int k = 0; k < NGQ; ++k) {
                const int i = min(tid + 256 * k, 4 * (PW / 4) - 1);
                const int ky = i / (PW / 4), xq = i % (PW / 4);
                const int gx = px0 * 4 + xq * 4;                    // S % 4 == 0: four pixels are inside the image or outside it
                gq[k] = *(const uint32_t*)(gray + ((size_t)b * S + (py * 4 + ky)) * S + min(gx, S - 4));
            }
        } else {
#pragma unroll
            for (int k = 0; k < NPQ; ++k) {
                const int i = min(tid + 256 * k, 12 * (PW / 4) - 1);
                const int line = i / (PW / 4), xq = i % (PW / 4);       // line = ci * 4 + ky
                const int gx = px0 * 4 + xq * 4;                        // S % 4 == 0: a quad is inside the image or outside it
                pq[k] = *(const f32x4*)(img + ((size_t)(b * 3 + (line >> 2)) * S + (py * 4 + (line & 3))) * S + min(gx, S - 4));
            }
        }
        f32x4 bq[CPT / 4];
#pragma unroll
        for (int j = 0; j < CPT / 4; ++j) bq[j] = *(const f32x4*)(bias + c0 + 4 * j);
        __builtin_amdgcn_sched_barrier(0);      // keep the requests together, ahead of the first wait
        if (ch > 0) __syncthreads();            // the previous chunk's pixels have been consumed
        else {
#pragma unroll
            for (int k = 0; k < NWQ; ++k) {
                const int i = tid + 256 * k;
                const int row = i / (C / 4), c = (i % (C / 4)) * 4;
                if (i < 12 * C) *(f32x4*)(wt + row * WS + c + (SWZ ? (c >> 6) * 4 : 0)) = wq[k];
            }
        }
        if constexpr (GRAY) {
#pragma unroll
            for (int k = 0; k < NGQ; ++k) {
                const int i = tid + 256 * k;
                const int ky = i / (PW / 4), xq = i % (PW / 4);
                const uint32_t u = gq[k];
                const float g[4] = {(float)(u & 255u), (float)((u >> 8) & 255u), (float)((u >> 16) & 255u), (float)(u >> 24)};
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (g[e] - nc.mean255[ci]) * nc.inv[ci];
                    if (px0 * 4 + xq * 4 >= S) v = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (i < 4 * (PW / 4)) *(f32x4*)(pix + (ci * 4 + ky) * PW + xq * 4) = v;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < NPQ; ++k) {
                const int i = tid + 256 * k;
                const int line = i / (PW / 4), xq = i % (PW / 4);
                f32x4 v = pq[k];
                if (px0 * 4 + xq * 4 >= S) v = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (i < 12 * (PW / 4)) *(f32x4*)(pix + line * PW + xq * 4) = v;
            }
        }
        __syncthreads();
        float acc[PE_NP][CPT];
#pragma unroll
        for (int j = 0; j < CPT; ++j)
#pragma unroll
            for (int q = 0; q < PE_NP; ++q) acc[q][j] = bq[j >> 2][j & 3];
        // tap loop, software-pipelined by hand: the weight quads of tap t + 1 (and, at kx = 3, the next line's pixels) are
        // requested before tap t's FMAs, the scheduling barrier keeps a tap's requests ahead of the previous tap's FMAs. (244
        // registers at C = 128: two workgroups per CU, where the LDS would allow three — capped at 168 registers the compiler
        // spills 70; two are enough to cover one workgroup's staging with the other's taps.)
        const float* wbase = wt + c0 + (SWZ ? (part >> 2) * 4 : 0);
        const float* pbase = pix + p * 4;
        f32x4 wc[CPT / 4], pv[PE_NP];
#pragma unroll
        for (int j = 0; j < CPT / 4; ++j) wc[j] = *(const f32x4*)(wbase + 4 * j);
#pragma unroll
        for (int q = 0; q < PE_NP; ++q) pv[q] = *(const f32x4*)(pbase + q * 128);
#pragma unroll 1
        for (int line = 0; line < 12; ++line) {
            f32x4 pn[PE_NP];
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                f32x4 wn[CPT / 4];
                const float* wr = wbase + min(line * 4 + kx + 1, 47) * WS;
#pragma unroll
                for (int j = 0; j < CPT / 4; ++j) wn[j] = *(const f32x4*)(wr + 4 * j);
                if (kx == 3) {
                    const float* pr = pbase + min(line + 1, 11) * PW;
#pragma unroll
                    for (int q = 0; q < PE_NP; ++q) pn[q] = *(const f32x4*)(pr + q * 128);
                }
#pragma unroll
                for (int j = 0; j < CPT; j += 4) {
                    const f32x4 w4 = wc[j >> 2];
#pragma unroll
                    for (int q = 0; q < PE_NP; ++q) {
                        const float v = pv[q][kx];
                        acc[q][j] = fmaf(v, w4[0], acc[q][j]); acc[q][j + 1] = fmaf(v, w4[1], acc[q][j + 1]);
                        acc[q][j + 2] = fmaf(v, w4[2], acc[q][j + 2]); acc[q][j + 3] = fmaf(v, w4[3], acc[q][j + 3]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < CPT / 4; ++j) wc[j] = wn[j];
            }
#pragma unroll
            for (int q = 0; q < PE_NP; ++q) pv[q] = pn[q];
        }
        __builtin_amdgcn_sched_barrier(0);      // gamma / beta requested here, not above the tap loop (32 registers)
        f32x4 g4[CPT / 4], b4[CPT / 4];
#pragma unroll
        for (int j = 0; j < CPT / 4; ++j) { g4[j] = *(const f32x4*)(gamma + c0 + 4 * j); b4[j] = *(const f32x4*)(beta + c0 + 4 * j); }
#pragma unroll
        for (int q = 0; q < PE_NP; ++q) {
            const int px = px0 + q * 32 + p;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < CPT; ++j) s += acc[q][j];
            s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
            const float mean = s / (float)C;
            float sq = 0.f;
#pragma unroll
            for (int j = 0; j < CPT; ++j) { acc[q][j] -= mean; sq = fmaf(acc[q][j], acc[q][j], sq); }
            sq += __shfl_xor(sq, 1, 64); sq += __shfl_xor(sq, 2, 64); sq += __shfl_xor(sq, 4, 64);
            const float rstd = rsqrtf(sq / (float)C + 1e-5f);
            if (px < G) {
                float* o = x + ((size_t)(b * G + py) * G + px) * C + c0;
#pragma unroll
                for (int j = 0; j < CPT; j += 4) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[q][j + e] * rstd, g4[j >> 2][e], b4[j >> 2][e]);
                    *(f32x4*)(o + j) = v;
                }
            }
        }
    }
