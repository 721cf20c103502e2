// Body of dec_head_kernel<BEAM> and dec_head_guided_kernel (decoder.hip): included once per kernel with MNX_HEAD_GUIDED 0 / 1,
// so that the unguided kernels compile from exactly the text they always had. Names from the including kernel: a (HeadArgs),
// BEAM, and — guided — g (GuideTab).
    __shared__ float hv[256];
    __shared__ float red[8];
    __shared__ int redi[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    const int4 rv = a.st->rowv[row];
    const int n_act = a.st->n_active;
    f32x4 xrow = *(const f32x4*)(a.x + (size_t)row * 256 + lane * 4);
    if (a.tree_bias) {
        const float* pp = a.part + (size_t)row * 256 + lane * 4;
        const size_t ps = (size_t)a.part_stride;
        f32x4 p[16];
#pragma unroll
        for (int z = 0; z < 16; ++z) p[z] = *(const f32x4*)(pp + z * ps);
#pragma unroll
        for (int w = 1; w < 16; w *= 2)
#pragma unroll
            for (int i = 0; i < 16; i += 2 * w) p[i] += p[i + w];
        xrow = xrow + (p[0] + *(const f32x4*)(a.tree_bias + lane * 4));
    } else if (a.part) {
        const float* pp = a.part + (size_t)row * 256 + lane * 4;
        const size_t ps = (size_t)a.part_stride;
        f32x4 sum = *(const f32x4*)pp;
        for (int z = 1; z < a.n_part; ++z) sum += *(const f32x4*)(pp + z * ps);
        xrow = sum + xrow;
    }
    if (row >= n_act) return;
    const int slot = rv.x, t = rv.y;
#if MNX_HEAD_GUIDED     // the row's next label id: requested here, consumed by thread 0 at the end
    const int* lab = g.lab + (size_t)slot * g.stride;
    const bool g_inside = t + 1 < lab[0];
    const int g_next = g_inside ? lab[t + 2] : GUIDE_MASK;
#endif
    if (wave == 0) {
        f32x4 v = xrow;
        const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
        v -= mean;
        const float var = wave_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]) * (1.0f / 256.0f);
        const f32x4 o = v * rsqrtf(var + 1e-6f) * *(const f32x4*)(a.gamma + lane * 4) + *(const f32x4*)(a.beta + lane * 4);
        *(f32x4*)(hv + lane * 4) = o;
        *(f32x4*)(a.hidden + ((size_t)slot * a.T + t) * 256 + lane * 4) = o;
    }
    __syncthreads();
    const bool valid = tid < a.V;
    float logit = -3.0e38f;
    if (valid) {
        float s = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 8
        for (int k = 0; k < 256; k += 4) {     // 32 independent coalesced loads in flight per unrolled body
            s = fmaf(hv[k], a.wout_t[k * a.VP + tid], s);
            s1 = fmaf(hv[k + 1], a.wout_t[(k + 1) * a.VP + tid], s1);
            s2 = fmaf(hv[k + 2], a.wout_t[(k + 2) * a.VP + tid], s2);
            s3 = fmaf(hv[k + 3], a.wout_t[(k + 3) * a.VP + tid], s3);
        }
        logit = (s + s1) + (s2 + s3) + a.bout[tid];
        if (a.logits_trace && slot < a.trace_rows) a.logits_trace[((size_t)t * a.trace_rows + slot) * a.V + tid] = logit;
    }
    // log_softmax
    float m = wave_max(logit);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float e = valid ? expf(logit - m) : 0.f;
    e = wave_sum(e);
    if (lane == 0) red[4 + wave] = e;
    __syncthreads();
    const float lse = m + logf(red[4] + red[5] + red[6] + red[7]);
    float lp = logit - lse;
    const int prev = rv.z;
    if (prev >= a.x0 && prev < a.y0) { if (tid < a.y0) lp = -10000.0f; }     // after an x-bin: only y-bins
    else if (prev >= a.y0)           { if (tid >= a.x0) lp = -10000.0f; }    // after a y-bin: no coordinate bins
    if (t == 0 && tid == a.eos) lp = -1e20f;                                  // min_length = 1
    if (BEAM) {
        if (valid) a.blp[(size_t)slot * BEAM_LP_STRIDE + tid] = lp;
        return;
    }
    if (!valid) lp = -3.0e38f;
    // argmax, lowest index wins ties (topk(1))
    float bv = lp;
    int bi = tid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) { red[wave] = bv; redi[wave] = bi; }
    __syncthreads();
#if MNX_HEAD_GUIDED
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (red[w] > bv || (red[w] == bv && redi[w] < bi)) { bv = red[w]; bi = redi[w]; }
        guided_advance(a, slot, t, g_next, g_inside, bi, bv);
    }
    return;
#endif
    const int ftok = (a.forced && slot < a.trace_rows) ? a.forced[(size_t)slot * a.T + t] : -1;
    if (ftok >= 0 && tid == ftok) a.token_logp[(size_t)slot * a.T + t] = lp;
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (red[w] > bv || (red[w] == bv && redi[w] < bi)) { bv = red[w]; bi = redi[w]; }
        a.tokens[(size_t)slot * a.T + t] = bi;
        if (ftok < 0) a.token_logp[(size_t)slot * a.T + t] = bv;
        const int adv = ftok >= 0 ? ftok : bi;
        a.st->prev_tok[slot] = adv;
        a.st->len[slot] = t + 1;
        a.st->t[slot] = t + 1;
        if ((a.st->stop_on_eos[slot] && adv == a.eos) || t + 1 >= a.st->max_len[slot]) a.st->alive[slot] = 0;
    }
