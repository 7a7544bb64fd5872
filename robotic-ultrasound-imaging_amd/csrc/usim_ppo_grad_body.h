// usim_ppo_grad_body.h -- the statements of the gradient kernel's body (usim_ppo.hip), included by the two kernel templates that run them: usim_ppo_grad_kernel
// (a lone call) and usim_ppo_grad_multi_kernel (a population: the member is blockIdx.z).  NOT a header of its own: it is the inside of a __global__ function that has
// declared, with these names,  N (N.w1[net] .. N.bh[net], N.log_std: the networks' fields),  b (PpoBatch),  work (the call's or the member's workspace),
// lay (PpoLay / PpoMultiLay: where the workspace holds what)  and the template parameters VF and LOSS.  The text is shared rather than a function because the lone
// instances have to be compiled from the statements they were compiled from: as an inlined function the same statements gave other register allocations (the
// clip_range_vf instance spilled; profiles/population_learner/resource_usage.txt), as the branch described in usim_ppo.hip once did.
    __shared__ __attribute__((aligned(16))) float xs[PP_TM][PP_XS];          // the tile's observations, column 19 zero
    __shared__ __attribute__((aligned(16))) float h1[PP_TM][PP_H1S];         // layer-1 activations; from the end of stage 6 the layer-1 deltas
    __shared__ __attribute__((aligned(16))) float h2[PP_TM][PP_H2S];         // layer-2 activations; from stage 5 the layer-2 deltas
    __shared__ __attribute__((aligned(16))) float whs[PP_MAXA][PP_H2];       // head weights, rows >= O zero
    __shared__ __attribute__((aligned(16))) float dout[PP_TM][PP_MAXA];      // d loss / d head output, columns >= O zero
    __shared__ float dls[PP_TM][PP_MAXA], acts[PP_TM][PP_MAXA];             // per-row d loss / d log_std; the tile's actions
    __shared__ float r_old[PP_TM], r_adv[PP_TM], r_ret[PP_TM], r_oldv[VF ? PP_TM : 1];      // r_oldv: the tile's old values (VF only)
    __shared__ double red[PP_WG / 64];
    if (pp_stopped(b.gate)) return;
    const int tid = threadIdx.x, net = blockIdx.y, A = b.adim, O = net ? 1 : A, B = b.batch;
    const PpoLayout L = ppo_layout(net, A);
    const int P = ppo_params(A);
    const float* __restrict__ W2R = work + lay.pack(A) + net * PP_W2;                     // [128][256]
    const float* __restrict__ W2T = work + lay.pack(A) + 2 * PP_W2 + net * PP_W2;         // [256][128]
    const double* adv_stat = reinterpret_cast<const double*>(work + lay.adv(A));
    const double adv_mean = adv_stat[0], adv_inv = adv_stat[1];
    const float* __restrict__ W1 = N.w1[net];
    const float* __restrict__ B1 = N.b1[net];
    const float* __restrict__ B2 = N.b2[net];
    for (int t = tid; t < PP_MAXA * PP_H2; t += PP_WG) whs[t / PP_H2][t % PP_H2] = (t / PP_H2 < O) ? N.wh[net][t] : 0.f;

    // this thread's places in the five products
    const int j1 = tid & 255, half = tid >> 8;                   // layer 1 and dW1: feature j1; rows 16 half .. (forward), inputs 10 half .. (dW1)
    const int cq = tid & 31, rg2 = tid >> 5;                     // layer 2: outputs 4 cq .. + 3 of rows 2 rg2, 2 rg2 + 1
    const int hk = tid & 127, hq = tid >> 7;                     // head gradient: input hk, outputs hq and hq + 4; layer-2 delta: column hk, rows 8 hq .. + 7
    const int cg = tid & 15, kg = tid >> 4;                      // dW2: outputs 8 cg .. + 7 x inputs 8 kg .. + 7
    const int kq = tid & 63, rg4 = tid >> 6;                     // d h1: inputs 4 kq .. + 3 of rows 4 rg4 .. + 3
    float aw2[8][8], aw1[10], awh0 = 0.f, awh1 = 0.f, ab1 = 0.f, ab2 = 0.f, asmall = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) aw2[i][j] = 0.f;
#pragma unroll
    for (int i = 0; i < 10; ++i) aw1[i] = 0.f;
    double s_pl = 0.0, s_kl = 0.0, s_cf = 0.0, s_vl = 0.0;        // loss sums of the rows this thread speaks for (tid < 256, tid % 8 == 0)

    const int ntiles = (LOSS != PP_PPO && net == 1 && !b.ret) ? 0 : (B + PP_TM - 1) / PP_TM;
    for (int tile = blockIdx.x; tile < ntiles; tile += PP_W) {
        const int row0 = tile * PP_TM;
        // ---- stage 0: the tile's samples (rows past the batch: zeros, and no gradient below) ----
        for (int t = tid; t < PP_TM * PP_XS; t += PP_WG) {
            const int r = t / PP_XS, i = t - r * PP_XS;
            xs[r][i] = (i < PP_OBS && row0 + r < B) ? b.obs[pp_row(b, row0 + r) * PP_OBS + i] : 0.f;
        }
        if (tid < 256) {
            const int r = tid >> 3, a = tid & 7;
            acts[r][a] = (a < A && row0 + r < B) ? b.act[pp_row(b, row0 + r) * A + a] : 0.f;
        } else if (tid < 256 + PP_TM) {
            const int r = tid - 256;
            const bool valid = row0 + r < B;
            const size_t src = valid ? pp_row(b, row0 + r) : 0;
            if constexpr (LOSS == PP_PPO) {
                r_old[r] = valid ? b.old_logp[src] : 0.f;
                r_adv[r] = valid ? (float)(((double)b.adv[src] - adv_mean) * adv_inv) : 0.f;
                r_ret[r] = valid ? b.ret[src] : 0.f;
                if constexpr (VF) r_oldv[r] = valid ? b.oldv[src] : 0.f;
            } else {
                r_ret[r] = (valid && b.ret) ? b.ret[src] : 0.f;   // the value target (read by the value network's workgroups only)
            }
        }
        __syncthreads();
        // ---- stage 1: layer 1 (19 -> 256, tanh) ----
        {
            float wv[PP_OBS];
#pragma unroll
            for (int i = 0; i < PP_OBS; ++i) wv[i] = W1[j1 * PP_OBS + i];
            const float bj = B1[j1];
#pragma unroll 4
            for (int rr = 0; rr < 16; ++rr) {
                const int r = 16 * half + rr;
                float acc = bj;
#pragma unroll
                for (int i = 0; i < PP_OBS; ++i) acc = fmaf(xs[r][i], wv[i], acc);
                h1[r][j1] = pp_tanh(acc);
            }
        }
        __syncthreads();
        // ---- stage 2: layer 2 (256 -> 128, tanh): 2 rows x 4 outputs per thread, the transposed copy read along its rows ----
        {
            const int r0 = 2 * rg2, c0 = 4 * cq;
            float a0[4], a1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a0[j] = a1[j] = B2[c0 + j];
#pragma unroll 2
            for (int k = 0; k < PP_H1; k += 4) {
                const float4 ha = *reinterpret_cast<const float4*>(&h1[r0][k]), hb = *reinterpret_cast<const float4*>(&h1[r0 + 1][k]);
                const float xa[4] = {ha.x, ha.y, ha.z, ha.w}, xb[4] = {hb.x, hb.y, hb.z, hb.w};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float4 w = *reinterpret_cast<const float4*>(&W2T[(k + s) * PP_H2 + c0]);
                    a0[0] = fmaf(xa[s], w.x, a0[0]); a0[1] = fmaf(xa[s], w.y, a0[1]); a0[2] = fmaf(xa[s], w.z, a0[2]); a0[3] = fmaf(xa[s], w.w, a0[3]);
                    a1[0] = fmaf(xb[s], w.x, a1[0]); a1[1] = fmaf(xb[s], w.y, a1[1]); a1[2] = fmaf(xb[s], w.z, a1[2]); a1[3] = fmaf(xb[s], w.w, a1[3]);
                }
            }
            *reinterpret_cast<float4*>(&h2[r0][c0]) = make_float4(pp_tanh(a0[0]), pp_tanh(a0[1]), pp_tanh(a0[2]), pp_tanh(a0[3]));
            *reinterpret_cast<float4*>(&h2[r0 + 1][c0]) = make_float4(pp_tanh(a1[0]), pp_tanh(a1[1]), pp_tanh(a1[2]), pp_tanh(a1[3]));
        }
        __syncthreads();
        // ---- stage 3: heads and the loss: eight lanes per row, lane a < O forms output a (waves 0 .. 3, whole) ----
        if (tid < 256) {
            const int r = tid >> 3, a = tid & 7;
            const bool valid = row0 + r < B;
            float out = 0.f;
            if (a < O) {
                out = N.bh[net][a];
#pragma unroll 8
                for (int k = 0; k < PP_H2; k += 4) {
                    const float4 h = *reinterpret_cast<const float4*>(&h2[r][k]);
                    const float4 w = *reinterpret_cast<const float4*>(&whs[a][k]);
                    out = fmaf(h.x, w.x, out); out = fmaf(h.y, w.y, out); out = fmaf(h.z, w.z, out); out = fmaf(h.w, w.w, out);
                }
            }
            if constexpr (LOSS != PP_PPO) {
                if (net == 0) {
                    // behaviour cloning: d = act - mean; log-prob as below; the row's squared action error sum_a d^2.  d loss / d log-prob = -1 / batch
                    // (PP_BC_NLL: the gradient reaches the mean, y / sigma, and log_std, y^2 - 1); d loss / d mean = -2 d / batch (PP_BC_MSE: the mean only)
                    const bool is_act = a < A;
                    const float ls = is_act ? N.log_std[a] : 0.f, inv_s = expf(-ls);
                    const float d = acts[r][a] - out, y = d * inv_s;
                    float lp = is_act ? fmaf(-0.5f * y, y, -ls - LOG_SQRT_2PI_F) : 0.f;
                    float sq = is_act ? d * d : 0.f;
                    lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4);
                    sq += __shfl_xor(sq, 1); sq += __shfl_xor(sq, 2); sq += __shfl_xor(sq, 4);
                    if constexpr (LOSS == PP_BC_NLL) {
                        const float g = valid ? -b.inv_b : 0.f;
                        dout[r][a] = is_act ? (g * y) * inv_s : 0.f;
                        dls[r][a] = is_act ? g * fmaf(y, y, -1.f) : 0.f;
                    } else {
                        dout[r][a] = (is_act && valid) ? (-2.f * b.inv_b) * d : 0.f;
                        dls[r][a] = 0.f;
                    }
                    if (a == 0 && valid) {
                        s_pl += LOSS == PP_BC_NLL ? -(double)lp : (double)sq;
                        s_kl += (double)sq;
                        s_cf += (double)lp;
                    }
                } else {
                    const float d = out - r_ret[r];
                    dout[r][a] = (a == 0 && valid) ? b.vf2 * d : 0.f;
                    dls[r][a] = 0.f;
                    if (a == 0 && valid) s_vl += (double)(d * d);
                }
            } else if (net == 0) {
                const bool is_act = a < A;
                const float ls = is_act ? N.log_std[a] : 0.f, inv_s = expf(-ls);
                const float y = (acts[r][a] - out) * inv_s;
                float lp = is_act ? fmaf(-0.5f * y, y, -ls - LOG_SQRT_2PI_F) : 0.f;      // DiagGaussianDistribution.log_prob, summed over the row's eight lanes
                lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4);
                const float lr = lp - r_old[r], ratio = expf(lr), ad = r_adv[r];
                const float lo = 1.f - b.clip, hi = 1.f + b.clip;
                const bool pass = !((ad > 0.f && ratio > hi) || (ad < 0.f && ratio < lo));  // min(A r, A clip(r)) has a gradient where the unclipped term is the smaller
                const float g = (valid && pass) ? -(ad * ratio) * b.inv_b : 0.f;          // d loss / d log-prob of the row
                dout[r][a] = is_act ? (g * y) * inv_s : 0.f;                              // d log-prob / d mean = y / sigma
                dls[r][a] = is_act ? g * fmaf(y, y, -1.f) : 0.f;                          // d log-prob / d log_std = y^2 - 1
                if (a == 0 && valid) {
                    const float rc = fminf(fmaxf(ratio, lo), hi);
                    s_pl -= (double)fminf(ad * ratio, ad * rc);
                    s_kl += (double)((ratio - 1.f) - lr);
                    s_cf += fabsf(ratio - 1.f) > b.clip ? 1.0 : 0.0;
                }
            } else if constexpr (VF) {
                // clip_range_vf: Vp = old + clamp(V - old, -c, c).  Inside the closed band Vp is V itself (not re-rounded through old) and the row is the
                // unclipped one; outside it the loss row takes old +- c formed in float32 and the gradient is exactly zero
                const float d = out - r_ret[r], old = r_oldv[r], dv = out - old;
                const bool inside = fabsf(dv) <= b.cvf;
                const float dc = inside ? d : (dv > 0.f ? old + b.cvf : old - b.cvf) - r_ret[r];
                dout[r][a] = (a == 0 && valid && inside) ? b.vf2 * d : 0.f;
                dls[r][a] = 0.f;
                if (a == 0 && valid) s_vl += (double)(dc * dc);
            } else {
                const float d = out - r_ret[r];
                dout[r][a] = (a == 0 && valid) ? b.vf2 * d : 0.f;
                dls[r][a] = 0.f;
                if (a == 0 && valid) s_vl += (double)(d * d);
            }
        }
        __syncthreads();
        // ---- stage 4: head gradients dWh += dout' h2, d bias, d log_std ----
        {
#pragma unroll 8
            for (int r = 0; r < PP_TM; ++r) {
                const float hv = h2[r][hk];
                awh0 = fmaf(dout[r][hq], hv, awh0); awh1 = fmaf(dout[r][hq + 4], hv, awh1);
            }
            if (tid < PP_MAXA) { for (int r = 0; r < PP_TM; ++r) asmall += dout[r][tid]; }
            else if (tid >= 64 && tid < 64 + PP_MAXA) { for (int r = 0; r < PP_TM; ++r) asmall += dls[r][tid - 64]; }
        }
        __syncthreads();
        // ---- stage 5: layer-2 deltas in place of h2: (dout Wh) (1 - h2^2); every word has one owner ----
        {
            float wc[PP_MAXA];
#pragma unroll
            for (int a = 0; a < PP_MAXA; ++a) wc[a] = whs[a][hk];
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const int r = 8 * hq + rr;
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < PP_MAXA; ++a) s = fmaf(dout[r][a], wc[a], s);        // (outputs >= O: zero times zero)
                const float hv = h2[r][hk];
                h2[r][hk] = s * fmaf(-hv, hv, 1.f);
            }
        }
        __syncthreads();
        // ---- stage 6: dW2 += delta2' h1 (8 x 8 per thread), d b2, and d h1 = delta2 W2 into registers ----
        float dh[4][4];
        {
#pragma unroll 2
            for (int r = 0; r < PP_TM; ++r) {
                const float4 d0 = *reinterpret_cast<const float4*>(&h2[r][8 * cg]), d1 = *reinterpret_cast<const float4*>(&h2[r][8 * cg + 4]);
                const float4 e0 = *reinterpret_cast<const float4*>(&h1[r][8 * kg]), e1 = *reinterpret_cast<const float4*>(&h1[r][8 * kg + 4]);
                const float dv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w}, ev[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) aw2[i][j] = fmaf(dv[i], ev[j], aw2[i][j]);
            }
            if (tid < PP_H2) { for (int r = 0; r < PP_TM; ++r) ab2 += h2[r][tid]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) dh[i][j] = 0.f;
#pragma unroll 2
            for (int c = 0; c < PP_H2; c += 4) {
                float dv[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 d = *reinterpret_cast<const float4*>(&h2[4 * rg4 + i][c]);
                    dv[i][0] = d.x; dv[i][1] = d.y; dv[i][2] = d.z; dv[i][3] = d.w;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float4 w = *reinterpret_cast<const float4*>(&W2R[(c + s) * PP_H1 + 4 * kq]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        dh[i][0] = fmaf(dv[i][s], w.x, dh[i][0]); dh[i][1] = fmaf(dv[i][s], w.y, dh[i][1]);
                        dh[i][2] = fmaf(dv[i][s], w.z, dh[i][2]); dh[i][3] = fmaf(dv[i][s], w.w, dh[i][3]);
                    }
                }
            }
        }
        __syncthreads();                                         // the last read of h1 as activations by another thread is behind
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4* p = reinterpret_cast<float4*>(&h1[4 * rg4 + i][4 * kq]);
            const float4 hv = *p;
            *p = make_float4(dh[i][0] * fmaf(-hv.x, hv.x, 1.f), dh[i][1] * fmaf(-hv.y, hv.y, 1.f), dh[i][2] * fmaf(-hv.z, hv.z, 1.f), dh[i][3] * fmaf(-hv.w, hv.w, 1.f));
        }
        __syncthreads();
        // ---- stage 7: dW1 += delta1' x, d b1 ----
#pragma unroll 4
        for (int r = 0; r < PP_TM; ++r) {
            const float dv = h1[r][j1];
#pragma unroll
            for (int i = 0; i < 10; ++i) aw1[i] = fmaf(dv, xs[r][10 * half + i], aw1[i]);
            if (half == 0) ab1 += dv;
        }
        __syncthreads();
    }

    // ---- this workgroup's block: every word of its network's share is written, zeros included ----
    float* __restrict__ part = work + (size_t)blockIdx.x * P;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) part[L.w2 + (8 * cg + i) * PP_H1 + 8 * kg + j] = aw2[i][j];
#pragma unroll
    for (int i = 0; i < 10; ++i)
        if (10 * half + i < PP_OBS) part[L.w1 + j1 * PP_OBS + 10 * half + i] = aw1[i];
    if (half == 0) part[L.b1 + j1] = ab1;
    if (tid < PP_H2) part[L.b2 + tid] = ab2;
    if (hq < O) part[L.wh + hq * PP_H2 + hk] = awh0;
    if (hq + 4 < O) part[L.wh + (hq + 4) * PP_H2 + hk] = awh1;
    if (tid < O) part[L.bh + tid] = asmall;
    if (net == 0 && tid >= 64 && tid < 64 + A) part[P - A + (tid - 64)] = asmall;
    double* sums = reinterpret_cast<double*>(work + lay.sums(A)) + (size_t)blockIdx.x * 8;
    const double t_pl = wg_sum(s_pl, red), t_kl = wg_sum(s_kl, red), t_cf = wg_sum(s_cf, red), t_vl = wg_sum(s_vl, red);
    if (tid == 0) {
        if (net == 0) { sums[0] = t_pl; sums[3] = t_kl; sums[4] = t_cf; }
        else sums[1] = t_vl;
    }
