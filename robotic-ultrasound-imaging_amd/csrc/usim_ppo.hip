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
// Populations (usim_ppo_grad_multi / usim_ppo_adam_multi; population.py PopulationPPO(concurrent=True)): the same six launches for K members at once, the member
// being the last grid axis of every kernel and its hyper-parameters a row of a table on the device.  Each population kernel states its member's pointers and runs
// the body of its lone counterpart, so a member's words are the bits of a lone call; the kernels and the workspace layout stand at the end of the namespace.
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

// prep's body, shared by the lone kernel and the population's (usim_ppo_prep_multi_kernel), which hands it one member's matrices, batch and workspace
DI void ppo_prep(const float* __restrict__ pi_w2, const float* __restrict__ vf_w2, const PpoBatch& b, float* __restrict__ pack, double* __restrict__ adv_out) {
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

__global__ __launch_bounds__(PP_RED) void usim_ppo_prep_kernel(const float* __restrict__ pi_w2, const float* __restrict__ vf_w2, PpoBatch b, float* __restrict__ pack,
                                                               double* __restrict__ adv_out) {
    ppo_prep(pi_w2, vf_w2, b, pack, adv_out);
}

// VF: clip_range_vf > 0.  The value clip is compiled into an instance of its own, so that the kernel of a call without it is the one it was before the clip existed
// (the branch in the shared body changed the register allocation of the whole kernel: profiles/ppo/resource_usage_gate.txt)
//
// LOSS: PP_PPO, or one of the two behaviour-cloning forms of usim_bc_grad (imitation.py NativeBC): the row's policy term is -log-prob(act) (PP_BC_NLL) or
// sum_a (mean_a - act_a)^2 (PP_BC_MSE), the value term regresses V on the row's target, there is no old log-prob, advantage or clip.  Only what a tile loads
// (stage 0) and the heads' loss (stage 3) differ, each behind `if constexpr`, so the PPO instances are compiled from the statements they were compiled from.  A
// behaviour-cloning call without value targets gives the value network's workgroups no tile: they write zeros.  b.ret carries the value targets (NULL: none), the
// float64 sums of approx_kl and clip_fraction carry the rows' squared action error and log-prob.
//
// The body's statements stand in usim_ppo_grad_body.h, which this kernel and the population's (usim_ppo_grad_multi_kernel, the member being blockIdx.z) include:
// `N` gives each field's pointer per network (N.w1[net]: PpoNet, or the population's PpoNetRow), `work` is the workspace of the call or of the member, `lay` says
// where it holds what (PpoLay: the fixed layout of W blocks; PpoMultiLay: nb blocks).  The lone instances are compiled from the statements they were compiled from.
struct PpoLay {                                                   // the workspace of a lone call
    DI int64_t pack(int A) const { return ppo_off_pack(A); }
    DI int64_t sums(int A) const { return ppo_off_sums(A); }
    DI int64_t adv(int A) const { return ppo_off_adv(A); }
    DI int blocks() const { return PP_W; }
};
template <bool VF, int LOSS = PP_PPO>
__global__ __launch_bounds__(PP_WG) void usim_ppo_grad_kernel(PpoNet N, PpoBatch b, float* __restrict__ work) {
    const PpoLay lay;
#include "usim_ppo_grad_body.h"
}

// one parameter per thread: the `blocks` partial blocks in block order
template <class Lay>
DI void ppo_reduce(const float* __restrict__ work, const Lay lay, int P, int A, float ent_coef, float* __restrict__ grad, const int32_t* gate) {
    if (pp_stopped(gate)) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float s = 0.f;
#pragma unroll 8
    for (int w = 0; w < lay.blocks(); ++w) s += work[(size_t)w * P + p];
    if (p >= P - A) s -= ent_coef;
    grad[p] = s;
}

__global__ __launch_bounds__(256) void usim_ppo_reduce_kernel(const float* __restrict__ work, int P, int A, float ent_coef, float* __restrict__ grad,
                                                               const int32_t* gate) {
    ppo_reduce(work, PpoLay{}, P, A, ent_coef, grad, gate);
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

// one workgroup: the `rows` rows of loss sums in row order, the gradient's norm, the statistics, the gate
template <class Lay>
DI void ppo_finish(const float* __restrict__ work, const Lay lay, const float* __restrict__ grad, const float* __restrict__ log_std, int P, int A, int batch, float vf_coef,
                   float ent_coef, float* __restrict__ stats, int32_t* gate, float target_kl) {
    __shared__ double red[PP_RED / 64];
    if (pp_stopped(gate)) return;                                 // (every thread has read the flag before the barriers below; thread 0 writes it behind them)
    const double norm = sqrt(sum_of_squares(grad, P, red));
    if (threadIdx.x != 0) return;
    const double* sums = reinterpret_cast<const double*>(work + lay.sums(A));
    double pl = 0.0, vl = 0.0, kl = 0.0, cf = 0.0, ent = 0.0;
    for (int w = 0; w < lay.blocks(); ++w) { pl += sums[8 * w]; vl += sums[8 * w + 1]; kl += sums[8 * w + 3]; cf += sums[8 * w + 4]; }
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

__global__ __launch_bounds__(PP_RED) void usim_ppo_finish_kernel(const float* __restrict__ work, const float* __restrict__ grad, const float* __restrict__ log_std, int P,
                                                                 int A, int batch, float vf_coef, float ent_coef, float* __restrict__ stats, int32_t* gate,
                                                                 float target_kl) {
    ppo_finish(work, PpoLay{}, grad, log_std, P, A, batch, vf_coef, ent_coef, stats, gate, target_kl);
}

// Adam's step count and, with a gate that is open, the gate's count of optimizer steps
DI void ppo_count(int32_t* __restrict__ step, int32_t* gate) {
    if (gate) {
        if (gate[0] != 0) return;
        gate[2] += 1;
    }
    *step += 1;
}

// one thread
__global__ void usim_ppo_count_kernel(int32_t* __restrict__ step, int32_t* gate) { ppo_count(step, gate); }

DI void ppo_adam(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v, const int32_t* __restrict__ step, int P, float lr,
                 float beta1, float beta2, float eps, float max_norm, float* __restrict__ stats, const int32_t* gate) {
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

__global__ __launch_bounds__(PP_RED) void usim_ppo_adam_kernel(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
                                                               const int32_t* __restrict__ step, int P, float lr, float beta1, float beta2, float eps, float max_norm,
                                                               float* __restrict__ stats, const int32_t* gate) {
    ppo_adam(theta, grad, m, v, step, P, lr, beta1, beta2, eps, max_norm, stats, gate);
}

// ---- the population's forms (usim_ppo_grad_multi / usim_ppo_adam_multi): the member is one more grid axis (the last).  Every kernel states its member's pointers --
// row k of the K-major tensors, rows [k rows, (k + 1) rows) of the data, region k of the workspace, row k of the hyper-parameter table -- and runs the body above,
// so member k's words are the bits of a lone call.  The gradient launch has nb = min(W, tiles) workgroups per network and member instead of W: a lone workgroup
// without a tile writes +0.0f into every word of its block and +0.0 into its loss sums, both reductions start from +0 and adding +0 to a sum that started from +0
// never changes a bit (such a sum is never -0), so blocks nb .. W - 1 are left out of the launch, the workspace and both reductions.
// A member's workspace region, in floats: nb partial blocks | the four packed matrices (16-byte aligned) | nb rows of 8 float64 sums | the two advantage words
__host__ __device__ constexpr int ppo_multi_blocks(int batch) { return batch > (PP_W - 1) * PP_TM ? PP_W : (batch + PP_TM - 1) / PP_TM; }
__host__ __device__ constexpr int64_t ppo_multi_off_pack(int A, int nb) { return ((int64_t)nb * ppo_params(A) + 3) / 4 * 4; }
__host__ __device__ constexpr int64_t ppo_multi_off_sums(int A, int nb) { return ppo_multi_off_pack(A, nb) + 4 * PP_W2; }
__host__ __device__ constexpr int64_t ppo_multi_off_adv(int A, int nb) { return ppo_multi_off_sums(A, nb) + 16 * nb; }
__host__ __device__ constexpr int64_t ppo_multi_member_floats(int A, int nb) { return ppo_multi_off_adv(A, nb) + 4; }      // a multiple of 4

// the table's row of a member (include/usim.h USIM_PPO_HYPER_WORDS)
enum { HY_LR = 0, HY_CLIP = 1, HY_ENT = 2, HY_VF = 3, HY_MAXNORM = 4, HY_CVF = 5, HY_KL = 6 };

struct PpoMulti {
    const float* theta;                                           // [K][stride]
    const float *obs, *act, *old_logp, *adv, *ret, *oldv;        // [K rows]...
    const int32_t* index;                                         // [K][index_stride] or NULL
    const float* hyper;                                           // [K][USIM_PPO_HYPER_WORDS]
    int32_t* gate;                                                // [K][USIM_PPO_GATE_WORDS] or NULL
    float *work, *grad, *stats;                                   // K regions; [K][stride]; [K][USIM_PPO_STATS]
    int64_t region;                                               // floats of a member's workspace region
    int stride, index_stride, rows, batch, adim, normalize, nb;
    float inv_b;
};

// a member's workspace region and its row of theta as the gradient body reads them
struct PpoMultiLay {
    int nb;
    DI int64_t pack(int A) const { return ppo_multi_off_pack(A, nb); }
    DI int64_t sums(int A) const { return ppo_multi_off_sums(A, nb); }
    DI int64_t adv(int A) const { return ppo_multi_off_adv(A, nb); }
    DI int blocks() const { return nb; }
};
struct PpoField {                                                 // N.w1[net] of a flat row: the field's place in either network
    const float* row; int at[2];
    DI const float* operator[](int net) const { return row + (net ? at[1] : at[0]); }
};
struct PpoNetRow { PpoField w1, b1, b2, wh, bh; const float* log_std; };
DI PpoNetRow pm_net(const float* th, int A) {
    const PpoLayout p = ppo_layout(0, A), v = ppo_layout(1, A);
    return {{th, {p.w1, v.w1}}, {th, {p.b1, v.b1}}, {th, {p.b2, v.b2}}, {th, {p.wh, v.wh}}, {th, {p.bh, v.bh}}, th + ppo_params(A) - A};
}
DI const float* pm_hyper(const PpoMulti& M, int k) { return M.hyper + (size_t)k * USIM_PPO_HYPER_WORDS; }
DI int32_t* pm_gate(const PpoMulti& M, int k) { return M.gate ? M.gate + (size_t)k * USIM_PPO_GATE_WORDS : nullptr; }
DI float* pm_work(const PpoMulti& M, int k) { return M.work + (size_t)k * M.region; }
// member k's batch as a lone call states it (vf2 formed as the host forms it: float64, rounded once)
template <bool VF>
DI PpoBatch pm_batch(const PpoMulti& M, int k) {
    const size_t r0 = (size_t)k * M.rows;
    const float* h = pm_hyper(M, k);
    return PpoBatch{M.obs + r0 * PP_OBS, M.act + r0 * M.adim, M.old_logp + r0, M.adv + r0, M.ret + r0, M.index ? M.index + (size_t)k * M.index_stride : nullptr,
                    M.rows, M.batch, M.adim, M.normalize, h[HY_CLIP], M.inv_b, (float)(2.0 * (double)h[HY_VF] / M.batch), VF ? M.oldv + r0 : nullptr,
                    VF ? h[HY_CVF] : 0.f, pm_gate(M, k)};
}

// grid (65, K)
__global__ __launch_bounds__(PP_RED) void usim_ppo_prep_multi_kernel(PpoMulti M) {
    const int k = blockIdx.y, A = M.adim;
    const float* th = M.theta + (size_t)k * M.stride;
    const PpoBatch b = pm_batch<false>(M, k);                     // (prep reads neither the old values nor clip_range_vf)
    float* work = pm_work(M, k);
    ppo_prep(th + ppo_layout(0, A).w2, th + ppo_layout(1, A).w2, b, work + ppo_multi_off_pack(A, M.nb), reinterpret_cast<double*>(work + ppo_multi_off_adv(A, M.nb)));
}

// grid (nb, 2, K)
template <bool VF>
__global__ __launch_bounds__(PP_WG) void usim_ppo_grad_multi_kernel(PpoMulti M) {
    const int k = blockIdx.z;
    constexpr int LOSS = PP_PPO;
    const PpoNetRow N = pm_net(M.theta + (size_t)k * M.stride, M.adim);
    const PpoBatch b = pm_batch<VF>(M, k);
    float* __restrict__ work = pm_work(M, k);
    const PpoMultiLay lay{M.nb};
#include "usim_ppo_grad_body.h"
}

// grid (ceil(P / 256), K)
__global__ __launch_bounds__(256) void usim_ppo_reduce_multi_kernel(PpoMulti M) {
    const int k = blockIdx.y, A = M.adim;
    ppo_reduce(pm_work(M, k), PpoMultiLay{M.nb}, ppo_params(A), A, pm_hyper(M, k)[HY_ENT], M.grad + (size_t)k * M.stride, pm_gate(M, k));
}

// grid (1, K)
__global__ __launch_bounds__(PP_RED) void usim_ppo_finish_multi_kernel(PpoMulti M) {
    const int k = blockIdx.y, A = M.adim;
    const float* h = pm_hyper(M, k);
    ppo_finish(pm_work(M, k), PpoMultiLay{M.nb}, M.grad + (size_t)k * M.stride,
               M.theta + (size_t)k * M.stride + ppo_params(A) - A, ppo_params(A), A, M.batch, h[HY_VF], h[HY_ENT], M.stats + (size_t)k * USIM_PPO_STATS, pm_gate(M, k),
               h[HY_KL]);
}

// one thread per member
__global__ __launch_bounds__(256) void usim_ppo_count_multi_kernel(int32_t* __restrict__ step, int32_t* gate, int members) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < members) ppo_count(step + k, gate ? gate + (size_t)k * USIM_PPO_GATE_WORDS : nullptr);
}

// grid (ceil(P / 1024), K)
__global__ __launch_bounds__(PP_RED) void usim_ppo_adam_multi_kernel(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
                                                                     const int32_t* __restrict__ step, int stride, int P, const float* __restrict__ hyper, float beta1,
                                                                     float beta2, float eps, float* __restrict__ stats, const int32_t* gate) {
    const int k = blockIdx.y;
    const size_t o = (size_t)k * stride;
    const float* h = hyper + (size_t)k * USIM_PPO_HYPER_WORDS;
    ppo_adam(theta + o, grad + o, m + o, v + o, step + k, P, h[HY_LR], beta1, beta2, eps, h[HY_MAXNORM], stats ? stats + (size_t)k * USIM_PPO_STATS : nullptr,
             gate ? gate + (size_t)k * USIM_PPO_GATE_WORDS : nullptr);
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

// ---- the population's calls ----
static bool multi_sizes_ok(int stride, int members, int params) {
    return members >= 1 && members <= USIM_POLICY_MAX_MEMBERS && params >= 1 && stride >= params && stride % 4 == 0;
}

extern "C" int64_t usim_ppo_work_floats_multi(int act_dim, int members, int batch) {
    using namespace usim;
    if (act_dim < 1 || act_dim > PP_MAXA || members < 1 || members > USIM_POLICY_MAX_MEMBERS || batch < 1) return (int64_t)USIM_ERR_INVALID;
    return (int64_t)members * ppo_multi_member_floats(act_dim, ppo_multi_blocks(batch));
}

extern "C" int usim_ppo_grad_multi(const float* theta_dev, int stride, int members, const usim_ppo_batch_multi* b, float* work_dev, float* grad_dev, float* stats_dev,
                                   void* stream) {
    using namespace usim;
    if (!theta_dev || !b || !work_dev || !grad_dev || !stats_dev || (reinterpret_cast<uintptr_t>(work_dev) & 15)) return USIM_ERR_INVALID;
    if (!b->obs_dev || !b->act_dev || !b->old_logp_dev || !b->adv_dev || !b->ret_dev || !b->hyper_dev) return USIM_ERR_INVALID;
    if (b->act_dim < 1 || b->act_dim > PP_MAXA || b->batch < 1 || b->rows < 1 || (!b->index_dev && b->rows < b->batch)) return USIM_ERR_INVALID;
    if (b->batch > INT32_MAX - PP_LOADS * PP_RED) return USIM_ERR_INVALID;                  // (as usim_ppo_grad)
    const int A = b->act_dim, P = ppo_params(A);
    if (!multi_sizes_ok(stride, members, P) || (int64_t)members * b->rows > INT32_MAX) return USIM_ERR_INVALID;
    if (b->index_dev && b->index_stride < b->batch) return USIM_ERR_INVALID;
    if (b->value_clip && !b->old_value_dev) return USIM_ERR_INVALID;
    const int nb = ppo_multi_blocks(b->batch);
    const PpoMulti M{theta_dev, b->obs_dev, b->act_dev, b->old_logp_dev, b->adv_dev, b->ret_dev, b->old_value_dev, b->index_dev, b->hyper_dev, b->gate_dev,
                     work_dev, grad_dev, stats_dev, ppo_multi_member_floats(A, nb), stride, b->index_stride, b->rows, b->batch, A, b->normalize_advantage, nb,
                     (float)(1.0 / b->batch)};
    const hipStream_t s = (hipStream_t)stream;
    const unsigned K = (unsigned)members;
    hipLaunchKernelGGL(usim_ppo_prep_multi_kernel, dim3(1 + 2 * PP_W2 / PP_RED, K), dim3(PP_RED), 0, s, M);
    if (b->value_clip) hipLaunchKernelGGL(usim_ppo_grad_multi_kernel<true>, dim3(nb, 2, K), dim3(PP_WG), 0, s, M);
    else hipLaunchKernelGGL(usim_ppo_grad_multi_kernel<false>, dim3(nb, 2, K), dim3(PP_WG), 0, s, M);
    hipLaunchKernelGGL(usim_ppo_reduce_multi_kernel, dim3((P + 255) / 256, K), dim3(256), 0, s, M);
    hipLaunchKernelGGL(usim_ppo_finish_multi_kernel, dim3(1, K), dim3(PP_RED), 0, s, M);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_ppo_adam_multi(float* theta_dev, const float* grad_dev, float* m_dev, float* v_dev, int32_t* step_dev, int stride, int members, int params,
                                   const float* hyper_dev, float beta1, float beta2, float eps, float* stats_dev, int32_t* gate_dev, void* stream) {
    using namespace usim;
    if (!theta_dev || !grad_dev || !m_dev || !v_dev || !step_dev || !hyper_dev || !multi_sizes_ok(stride, members, params)) return USIM_ERR_INVALID;
    if (!nonneg_finite(eps) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return USIM_ERR_INVALID;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(usim_ppo_count_multi_kernel, dim3((members + 255) / 256), dim3(256), 0, s, step_dev, gate_dev, members);
    hipLaunchKernelGGL(usim_ppo_adam_multi_kernel, dim3((params + PP_RED - 1) / PP_RED, (unsigned)members), dim3(PP_RED), 0, s, theta_dev, grad_dev, m_dev, v_dev, step_dev,
                       stride, params, hyper_dev, beta1, beta2, eps, stats_dev, gate_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}
