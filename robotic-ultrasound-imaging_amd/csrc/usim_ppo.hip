// usim_ppo.hip -- usim_ppo_grad / usim_ppo_adam: the learner's side of a PPO minibatch step (ppo.py NativePPO) -- the loss of
// stable-baselines3's PPO.train on one minibatch of the rollout buffer with its gradient for every parameter of the shipped MlpPolicy (19 -> 256 -> 128, tanh,
// A <= 8), and clip_grad_norm_ + Adam.step on one flat parameter block.  A translation unit of its own: it takes no usim_handle and shares nothing with the other
// units but the public header and usim_devmath.h (DI).
//
// usim_ppo_grad is four launches on the caller's stream:
//   prep      workgroup 0: mean and 1 / (std + 1e-8) of the minibatch's advantages in float64 (two passes, unbiased std; identity when not asked for or batch == 1);
//             workgroups 1 .. 64: both layer-2 matrices copied into the workspace, 16-byte aligned, as they are ([128][256]: the backward product reads rows) and
//             transposed ([256][128]: the forward product reads rows of that) -- the caller's tensors may sit at any 4-byte offset of a flat block
//   grad      USIM_PPO_WORKGROUPS x 2 workgroups of 512 threads; workgroup (w, net) takes the tiles w, w + W, w + 2 W, ... of 32 minibatch rows through ONE network
//             (0: policy, 1: value): forward pass, loss terms, backward pass, everything between barriers in LDS (activations h1 / h2; the deltas overwrite them in
//             place once their last reader is through).  Its share of every weight gradient stays in accumulator registers across its tiles (dW2: 8 x 8 words per
//             thread, dW1: 10, heads: 2, biases: 1 each) and is written once, at the end, as block w of the workspace -- a workgroup without a tile writes zeros, so the
//             workspace needs no clearing between calls
//   reduce    one thread per parameter adds the W blocks in block order (and subtracts ent_coef from the log_std entries: d(-ent_coef entropy) / d log_std)
//   finish    one workgroup: the W rows of loss sums in row order, the gradient's 2-norm, the eight statistics
// usim_ppo_adam is two: a one-thread launch that advances the step count, and the update (every workgroup forms the same norm from the whole gradient itself).
//
// clip_range_vf (SB3's value clipping) is a second instance of the gradient kernel (template parameter VF): stage 3's value lanes clamp V around the row's old
// value, one more LDS row.  A call without it launches the instance without it, whose value path is the one above, instruction for instruction.
// Behaviour cloning (usim_bc_grad; imitation.py NativeBC) is two more instances (template parameter LOSS): the supervised loss of the `imitation` package's BC in
// stage 3, fewer loads in stage 0, everything else -- the workspace, prep, reduce, finish, usim_ppo_adam -- shared as it is.
// The gate (target_kl's early stop, taken on the device; include/usim.h states the words): every kernel of both calls reads the stop flag on entry -- one word, the
// same for every thread, in front of every barrier -- and returns when it is set.  Thread 0 of finish counts the call and, last thing, sets the flag from the
// float32 approx_kl it has just written; the one-thread count kernel counts the step.  Plain stores by single threads of single-workgroup kernels; no atomics.
//
// THE ORDER OF EVERY SUM IS FIXED: a thread adds its rows in ascending order inside a tile and its tiles in ascending order; blocks are added in block order; sums
// over a workgroup are a butterfly inside the wave and the waves in order (as usim_plan.hip).  No floating-point atomics, nothing ordered by arrival, no dependence
// on the device's CU count: the same inputs give the same bits on every call.
//
// Numerics: float32 fused multiply-adds (plain loops: the matrix cores are the next step), tanh as usim_policy.hip's tanh_, expf of the
// device library for the standard deviation and the ratio; the advantage normalisation, the loss sums and the whole of Adam's arithmetic in float64, rounded once.
// tests/ppo_ref.py states the float64 reference and derives the error bound per gradient entry from exactly these operations.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/usim.h"
#include "usim_devmath.h"

namespace usim {

constexpr int PP_OBS = 19, PP_XS = 20, PP_H1 = 256, PP_H2 = 128, PP_TM = 32, PP_MAXA = 8;
constexpr int PP_H1S = PP_H1 + 4, PP_H2S = PP_H2 + 4;            // LDS row strides (16-byte aligned, off the bank period)
constexpr int PP_WG = 512;                                       // threads of a gradient workgroup
constexpr int PP_W = USIM_PPO_WORKGROUPS;                        // gradient workgroups per network = partial blocks: a constant of the library
constexpr int PP_RED = 1024;                                     // threads of the one-workgroup reductions (prep, finish) and of an Adam workgroup
constexpr int PP_LOADS = 8;                                      // loads a thread of those reductions has in flight before it adds them in order
constexpr int PP_BODY = PP_H1 * PP_OBS + PP_H1 + PP_H2 * PP_H1 + PP_H2;      // w1 b1 w2 b2 of one network: 38016
constexpr int PP_W2 = PP_H2 * PP_H1;                             // one layer-2 matrix
constexpr float LOG_SQRT_2PI_F = 0.9189385332046727f;
constexpr int PP_PPO = 0, PP_BC_NLL = 1 + USIM_BC_NLL, PP_BC_MSE = 1 + USIM_BC_MSE;      // the loss of a gradient-kernel instance (stage 0 and stage 3)

// offsets of one network's fields in the flat block (include/usim.h: pi_w1 pi_b1 pi_w2 pi_b2 act_w act_b vf_w1 vf_b1 vf_w2 vf_b2 val_w val_b log_std)
struct PpoLayout { int w1, b1, w2, b2, wh, bh; };
__host__ __device__ constexpr PpoLayout ppo_layout(int net, int A) {
    const int base = net ? PP_BODY + 129 * A : 0;
    return {base, base + PP_H1 * PP_OBS, base + PP_H1 * PP_OBS + PP_H1, base + PP_BODY - PP_H2, base + PP_BODY, base + PP_BODY + PP_H2 * (net ? 1 : A)};
}
__host__ __device__ constexpr int ppo_params(int A) { return 2 * PP_BODY + 130 * A + 129; }
// the workspace, in floats: W partial blocks | both W2 as they are, both transposed (16-byte aligned) | W rows of 8 float64 loss sums | advantage mean, 1 / (std + 1e-8)
__host__ __device__ constexpr int64_t ppo_off_pack(int A) { return ((int64_t)PP_W * ppo_params(A) + 3) / 4 * 4; }
__host__ __device__ constexpr int64_t ppo_off_sums(int A) { return ppo_off_pack(A) + 4 * PP_W2; }
__host__ __device__ constexpr int64_t ppo_off_adv(int A) { return ppo_off_sums(A) + 16 * PP_W; }
__host__ __device__ constexpr int64_t ppo_work_floats(int A) { return ppo_off_adv(A) + 4; }

struct PpoNet { const float *w1[2], *b1[2], *w2[2], *b2[2], *wh[2], *bh[2]; const float* log_std; };      // [0] policy, [1] value
struct PpoBatch {
    const float *obs, *act, *old_logp, *adv, *ret;
    const int32_t* index;
    int rows, batch, adim, normalize;
    float clip, inv_b, vf2;                                       // clip_range, 1 / batch, 2 vf_coef / batch
    const float* oldv;                                            // RolloutBuffer.values, read only when cvf > 0
    float cvf;                                                    // clip_range_vf; 0: off
    const int32_t* gate;                                          // the gate words or NULL; [0] set: every kernel of the call returns on entry
};

// the stop flag of the gate, read by every thread on entry (the same word for all: the branch is uniform and in front of every barrier)
DI bool pp_stopped(const int32_t* gate) { return gate && gate[0] != 0; }

// tanh(x) = 1 - 2 / (exp(2x) + 1), as usim_policy.hip's tanh_ (v_exp_f32 + v_rcp_f32: 2^-22 absolute; saturates to +-1)
DI float pp_tanh(float x) { const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f); return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f); }
// the buffer row of minibatch sample i (an index outside the buffer is moved to its nearest row rather than read)
DI size_t pp_row(const PpoBatch& b, int i) { return b.index ? (size_t)min(max(b.index[i], 0), b.rows - 1) : (size_t)i; }

// sum over a workgroup of whole waves: butterfly inside the wave, then the waves in order; all threads arrive, all receive the same bits.  lds: blockDim.x / 64 words
DI double wg_sum(double x, double* lds) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    __syncthreads();                                              // (the words may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += lds[w];
    return s;
}

__global__ __launch_bounds__(PP_RED) void usim_ppo_prep_kernel(const float* __restrict__ pi_w2, const float* __restrict__ vf_w2, PpoBatch b, float* __restrict__ pack,
                                                               double* __restrict__ adv_out) {
    __shared__ double red[PP_RED / 64];
    const int tid = threadIdx.x;
    if (pp_stopped(b.gate)) return;
    if (blockIdx.x > 0) {                                         // one word of one matrix per thread: 2 x 128 x 256 = 64 workgroups
        const int idx = (blockIdx.x - 1) * PP_RED + tid, net = idx / PP_W2, c = (idx / PP_H1) % PP_H2, k = idx % PP_H1;
        const float v = (net ? vf_w2 : pi_w2)[c * PP_H1 + k];
        pack[idx] = v;
        pack[2 * PP_W2 + net * PP_W2 + k * PP_H2 + c] = v;
        return;
    }
    double mean = 0.0, inv = 1.0;
    if (b.normalize && b.batch > 1) {                             // (uniform over the workgroup: every thread passes the barriers of wg_sum)
        // a thread's samples tid, tid + 1024, ... in ascending order, eight gathers in flight at a time (a sample past the batch adds an exact zero)
        double s = 0.0;
        for (int i = tid; i < b.batch; i += PP_LOADS * PP_RED) {
            double x[PP_LOADS];
#pragma unroll
            for (int u = 0; u < PP_LOADS; ++u) { const int k = i + u * PP_RED; x[u] = k < b.batch ? (double)b.adv[pp_row(b, k)] : 0.0; }
#pragma unroll
            for (int u = 0; u < PP_LOADS; ++u) s += x[u];
        }
        mean = wg_sum(s, red) / b.batch;
        double q = 0.0;
        for (int i = tid; i < b.batch; i += PP_LOADS * PP_RED) {
            double d[PP_LOADS];
#pragma unroll
            for (int u = 0; u < PP_LOADS; ++u) { const int k = i + u * PP_RED; d[u] = k < b.batch ? (double)b.adv[pp_row(b, k)] - mean : 0.0; }
#pragma unroll
            for (int u = 0; u < PP_LOADS; ++u) q = fma(d[u], d[u], q);
        }
        inv = 1.0 / (sqrt(wg_sum(q, red) / (b.batch - 1)) + 1e-8);
    }
    if (tid == 0) { adv_out[0] = mean; adv_out[1] = inv; }
}

// VF: clip_range_vf > 0.  The value clip is compiled into an instance of its own, so that the kernel of a call without it is the one it was before the clip existed
// (the branch in the shared body changed the register allocation of the whole kernel: profiles/ppo/resource_usage_gate.txt)
//
// LOSS: PP_PPO, or one of the two behaviour-cloning forms of usim_bc_grad (imitation.py NativeBC): the row's policy term is -log-prob(act) (PP_BC_NLL) or
// sum_a (mean_a - act_a)^2 (PP_BC_MSE), the value term regresses V on the row's target, there is no old log-prob, advantage or clip.  Only what a tile loads
// (stage 0) and the heads' loss (stage 3) differ, each behind `if constexpr`, so the PPO instances are compiled from the statements they were compiled from.  A
// behaviour-cloning call without value targets gives the value network's workgroups no tile: they write zeros.  b.ret carries the value targets (NULL: none), the
// float64 sums of approx_kl and clip_fraction carry the rows' squared action error and log-prob.
template <bool VF, int LOSS = PP_PPO>
__global__ __launch_bounds__(PP_WG) void usim_ppo_grad_kernel(PpoNet N, PpoBatch b, float* __restrict__ work) {
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
    const float* __restrict__ W2R = work + ppo_off_pack(A) + net * PP_W2;                 // [128][256]
    const float* __restrict__ W2T = work + ppo_off_pack(A) + 2 * PP_W2 + net * PP_W2;     // [256][128]
    const double* adv_stat = reinterpret_cast<const double*>(work + ppo_off_adv(A));
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
    double* sums = reinterpret_cast<double*>(work + ppo_off_sums(A)) + (size_t)blockIdx.x * 8;
    const double t_pl = wg_sum(s_pl, red), t_kl = wg_sum(s_kl, red), t_cf = wg_sum(s_cf, red), t_vl = wg_sum(s_vl, red);
    if (tid == 0) {
        if (net == 0) { sums[0] = t_pl; sums[3] = t_kl; sums[4] = t_cf; }
        else sums[1] = t_vl;
    }
}

__global__ __launch_bounds__(256) void usim_ppo_reduce_kernel(const float* __restrict__ work, int P, int A, float ent_coef, float* __restrict__ grad,
                                                               const int32_t* gate) {
    if (pp_stopped(gate)) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float s = 0.f;
#pragma unroll 8
    for (int w = 0; w < PP_W; ++w) s += work[(size_t)w * P + p];
    if (p >= P - A) s -= ent_coef;
    grad[p] = s;
}

DI double sum_of_squares(const float* __restrict__ g, int P, double* lds) {
    double q = 0.0;
    for (int i = threadIdx.x; i < P; i += PP_LOADS * PP_RED) {   // ascending, eight loads in flight (a word past the end adds an exact zero)
        double x[PP_LOADS];
#pragma unroll
        for (int u = 0; u < PP_LOADS; ++u) { const int k = i + u * PP_RED; x[u] = k < P ? (double)g[k] : 0.0; }
#pragma unroll
        for (int u = 0; u < PP_LOADS; ++u) q = fma(x[u], x[u], q);
    }
    return wg_sum(q, lds);
}

__global__ __launch_bounds__(PP_RED) void usim_ppo_finish_kernel(const float* __restrict__ work, const float* __restrict__ grad, const float* __restrict__ log_std, int P,
                                                                 int A, int batch, float vf_coef, float ent_coef, float* __restrict__ stats, int32_t* gate,
                                                                 float target_kl) {
    __shared__ double red[PP_RED / 64];
    if (pp_stopped(gate)) return;                                 // (every thread has read the flag before the barriers below; thread 0 writes it behind them)
    const double norm = sqrt(sum_of_squares(grad, P, red));
    if (threadIdx.x != 0) return;
    const double* sums = reinterpret_cast<const double*>(work + ppo_off_sums(A));
    double pl = 0.0, vl = 0.0, kl = 0.0, cf = 0.0, ent = 0.0;
    for (int w = 0; w < PP_W; ++w) { pl += sums[8 * w]; vl += sums[8 * w + 1]; kl += sums[8 * w + 3]; cf += sums[8 * w + 4]; }
    for (int a = 0; a < A; ++a) ent += (double)log_std[a];
    ent += A * (0.5 + 0.9189385332046727);                       // A / 2 (1 + log 2 pi)
    pl /= batch; vl /= batch; kl /= batch; cf /= batch;
    const float kl32 = (float)kl;
    stats[0] = (float)pl; stats[1] = (float)vl; stats[2] = (float)-ent; stats[3] = kl32; stats[4] = (float)cf;
    stats[5] = (float)(pl + (double)vf_coef * vl - (double)ent_coef * ent); stats[6] = (float)norm; stats[7] = 0.f;
    if (gate) {                                                   // this thread alone writes the gate: the call's count, then -- last thing -- the stop flag
        gate[1] += 1;
        if (target_kl > 0.f && kl32 > 1.5f * target_kl) gate[0] = 1;      // SB3: approx_kl > 1.5 target_kl, on the float32 word just written
    }
}

// one thread: Adam's step count and, with a gate that is open, the gate's count of optimizer steps
__global__ void usim_ppo_count_kernel(int32_t* __restrict__ step, int32_t* gate) {
    if (gate) {
        if (gate[0] != 0) return;
        gate[2] += 1;
    }
    *step += 1;
}

__global__ __launch_bounds__(PP_RED) void usim_ppo_adam_kernel(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
                                                               const int32_t* __restrict__ step, int P, float lr, float beta1, float beta2, float eps, float max_norm,
                                                               float* __restrict__ stats, const int32_t* gate) {
    __shared__ double red[PP_RED / 64];
    __shared__ double corr[2];
    if (pp_stopped(gate)) return;
    const double norm = sqrt(sum_of_squares(grad, P, red));       // every workgroup: the same words in the same order
    if (threadIdx.x == 0) {
        const double t = (double)*step;
        corr[0] = 1.0 - pow((double)beta1, t); corr[1] = 1.0 - pow((double)beta2, t);
        if (stats && blockIdx.x == 0) stats[6] = (float)norm;
    }
    __syncthreads();
    const int i = blockIdx.x * PP_RED + threadIdx.x;
    if (i >= P) return;
    const double coef = max_norm > 0.f ? fmin(1.0, (double)max_norm / (norm + 1e-6)) : 1.0;
    const double b1 = beta1, b2 = beta2, g = (double)grad[i] * coef;
    const double mi = b1 * (double)m[i] + (1.0 - b1) * g, vi = b2 * (double)v[i] + (1.0 - b2) * g * g;
    const double denom = sqrt(vi) / sqrt(corr[1]) + (double)eps;
    m[i] = (float)mi; v[i] = (float)vi;
    theta[i] = (float)((double)theta[i] - ((double)lr / corr[0]) * (mi / denom));
}

}  // namespace usim

static bool nonneg_finite(float x) { return x >= 0.f && isfinite(x); }               // (a NaN fails the comparison)

extern "C" int usim_ppo_params(int act_dim) { return act_dim >= 1 && act_dim <= usim::PP_MAXA ? usim::ppo_params(act_dim) : USIM_ERR_INVALID; }

extern "C" int64_t usim_ppo_work_floats(int act_dim) { return act_dim >= 1 && act_dim <= usim::PP_MAXA ? usim::ppo_work_floats(act_dim) : (int64_t)USIM_ERR_INVALID; }

extern "C" int usim_ppo_grad(const usim_policy_net* net, const usim_ppo_batch* b, float* work_dev, float* grad_dev, float* stats_dev, void* stream) {
    using namespace usim;
    if (!net || !b || !work_dev || !grad_dev || !stats_dev || (reinterpret_cast<uintptr_t>(work_dev) & 15)) return USIM_ERR_INVALID;
    if (!net->pi_w1 || !net->pi_b1 || !net->pi_w2 || !net->pi_b2 || !net->act_w || !net->act_b || !net->vf_w1 || !net->vf_b1 || !net->vf_w2 || !net->vf_b2 ||
        !net->val_w || !net->val_b || !net->log_std) return USIM_ERR_INVALID;
    if (!b->obs_dev || !b->act_dev || !b->old_logp_dev || !b->adv_dev || !b->ret_dev) return USIM_ERR_INVALID;
    if (b->act_dim < 1 || b->act_dim > PP_MAXA || b->batch < 1 || b->rows < 1 || (!b->index_dev && b->rows < b->batch)) return USIM_ERR_INVALID;
    if (b->batch > INT32_MAX - PP_LOADS * PP_RED) return USIM_ERR_INVALID;                  // (sample numbers are ints, and the strided loops step past the end once)
    if (!nonneg_finite(b->clip_range) || !isfinite(b->ent_coef) || !isfinite(b->vf_coef)) return USIM_ERR_INVALID;
    if (!nonneg_finite(b->clip_range_vf) || !nonneg_finite(b->target_kl)) return USIM_ERR_INVALID;
    if ((b->clip_range_vf > 0.f && !b->old_value_dev) || (b->target_kl > 0.f && !b->gate_dev)) return USIM_ERR_INVALID;
    const int A = b->act_dim, P = ppo_params(A);
    const PpoNet N{{net->pi_w1, net->vf_w1}, {net->pi_b1, net->vf_b1}, {net->pi_w2, net->vf_w2}, {net->pi_b2, net->vf_b2}, {net->act_w, net->val_w},
                   {net->act_b, net->val_b}, net->log_std};
    const PpoBatch K{b->obs_dev, b->act_dev, b->old_logp_dev, b->adv_dev, b->ret_dev, b->index_dev, b->rows, b->batch, A, b->normalize_advantage,
                     b->clip_range, (float)(1.0 / b->batch), (float)(2.0 * (double)b->vf_coef / b->batch), b->old_value_dev, b->clip_range_vf, b->gate_dev};
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(usim_ppo_prep_kernel, dim3(1 + 2 * PP_W2 / PP_RED), dim3(PP_RED), 0, s, net->pi_w2, net->vf_w2, K, work_dev + ppo_off_pack(A),
                       reinterpret_cast<double*>(work_dev + ppo_off_adv(A)));
    if (K.cvf > 0.f) hipLaunchKernelGGL(usim_ppo_grad_kernel<true>, dim3(PP_W, 2), dim3(PP_WG), 0, s, N, K, work_dev);
    else hipLaunchKernelGGL(usim_ppo_grad_kernel<false>, dim3(PP_W, 2), dim3(PP_WG), 0, s, N, K, work_dev);
    hipLaunchKernelGGL(usim_ppo_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, s, work_dev, P, A, b->ent_coef, grad_dev, b->gate_dev);
    hipLaunchKernelGGL(usim_ppo_finish_kernel, dim3(1), dim3(PP_RED), 0, s, work_dev, grad_dev, net->log_std, P, A, b->batch, b->vf_coef, b->ent_coef, stats_dev,
                       b->gate_dev, b->target_kl);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

// usim_bc_grad: usim_ppo_grad's four launches with a behaviour-cloning instance of the gradient kernel in the second.  prep copies both W2 matrices and takes its
// identity path for the advantages (none are read); reduce and finish are the ones above without a gate: their sums 3 and 4 are the rows' action error and log-prob
extern "C" int usim_bc_grad(const usim_policy_net* net, const usim_bc_batch* b, float* work_dev, float* grad_dev, float* stats_dev, void* stream) {
    using namespace usim;
    if (!net || !b || !work_dev || !grad_dev || !stats_dev || (reinterpret_cast<uintptr_t>(work_dev) & 15)) return USIM_ERR_INVALID;
    if (!net->pi_w1 || !net->pi_b1 || !net->pi_w2 || !net->pi_b2 || !net->act_w || !net->act_b || !net->vf_w1 || !net->vf_b1 || !net->vf_w2 || !net->vf_b2 ||
        !net->val_w || !net->val_b || !net->log_std) return USIM_ERR_INVALID;
    if (!b->obs_dev || !b->act_dev) return USIM_ERR_INVALID;
    if (b->act_dim < 1 || b->act_dim > PP_MAXA || b->batch < 1 || b->rows < 1 || (!b->index_dev && b->rows < b->batch)) return USIM_ERR_INVALID;
    if (b->batch > INT32_MAX - PP_LOADS * PP_RED) return USIM_ERR_INVALID;
    if (b->loss != USIM_BC_NLL && b->loss != USIM_BC_MSE) return USIM_ERR_INVALID;
    if (!isfinite(b->ent_coef) || !isfinite(b->vf_coef)) return USIM_ERR_INVALID;
    const int A = b->act_dim, P = ppo_params(A);
    const bool valued = b->value_dev && b->vf_coef != 0.f;         // no value term: the value network is not evaluated, its gradient words are +0
    const float vf_coef = valued ? b->vf_coef : 0.f;
    const PpoNet N{{net->pi_w1, net->vf_w1}, {net->pi_b1, net->vf_b1}, {net->pi_w2, net->vf_w2}, {net->pi_b2, net->vf_b2}, {net->act_w, net->val_w},
                   {net->act_b, net->val_b}, net->log_std};
    const PpoBatch K{b->obs_dev, b->act_dev, nullptr, nullptr, valued ? b->value_dev : nullptr, b->index_dev, b->rows, b->batch, A, 0,
                     0.f, (float)(1.0 / b->batch), (float)(2.0 * (double)vf_coef / b->batch), nullptr, 0.f, nullptr};
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(usim_ppo_prep_kernel, dim3(1 + 2 * PP_W2 / PP_RED), dim3(PP_RED), 0, s, net->pi_w2, net->vf_w2, K, work_dev + ppo_off_pack(A),
                       reinterpret_cast<double*>(work_dev + ppo_off_adv(A)));
    if (b->loss == USIM_BC_NLL) hipLaunchKernelGGL((usim_ppo_grad_kernel<false, PP_BC_NLL>), dim3(PP_W, 2), dim3(PP_WG), 0, s, N, K, work_dev);
    else hipLaunchKernelGGL((usim_ppo_grad_kernel<false, PP_BC_MSE>), dim3(PP_W, 2), dim3(PP_WG), 0, s, N, K, work_dev);
    hipLaunchKernelGGL(usim_ppo_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, s, work_dev, P, A, b->ent_coef, grad_dev, nullptr);
    hipLaunchKernelGGL(usim_ppo_finish_kernel, dim3(1), dim3(PP_RED), 0, s, work_dev, grad_dev, net->log_std, P, A, b->batch, vf_coef, b->ent_coef, stats_dev,
                       nullptr, 0.f);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_ppo_adam_gated(float* theta_dev, const float* grad_dev, float* m_dev, float* v_dev, int32_t* step_dev, int params, float lr, float beta1,
                                   float beta2, float eps, float max_grad_norm, float* stats_dev, int32_t* gate_dev, void* stream) {
    using namespace usim;
    if (!theta_dev || !grad_dev || !m_dev || !v_dev || !step_dev || params < 1) return USIM_ERR_INVALID;
    if (!nonneg_finite(lr) || !nonneg_finite(eps) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || isnan(max_grad_norm)) return USIM_ERR_INVALID;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(usim_ppo_count_kernel, dim3(1), dim3(1), 0, s, step_dev, gate_dev);
    hipLaunchKernelGGL(usim_ppo_adam_kernel, dim3((params + PP_RED - 1) / PP_RED), dim3(PP_RED), 0, s, theta_dev, grad_dev, m_dev, v_dev, step_dev, params, lr, beta1, beta2,
                       eps, max_grad_norm, stats_dev, gate_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_ppo_adam(float* theta_dev, const float* grad_dev, float* m_dev, float* v_dev, int32_t* step_dev, int params, float lr, float beta1, float beta2,
                             float eps, float max_grad_norm, float* stats_dev, void* stream) {
    return usim_ppo_adam_gated(theta_dev, grad_dev, m_dev, v_dev, step_dev, params, lr, beta1, beta2, eps, max_grad_norm, stats_dev, nullptr, stream);
}
