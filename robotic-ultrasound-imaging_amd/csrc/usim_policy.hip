// usim_policy.hip -- the CALLER's side of env.step() on the device: SB3's VecNormalize + MlpPolicy forward + action sampling + rollout-buffer
// writes + GAE as four kernels per rollout step (src/rl.py:140 VecNormalize, :143 PPO("MlpPolicy"), :157 / :177-184
// checkpoints).  A translation unit of its own: it takes no usim_handle and shares nothing with the step kernels but usim_devmath.h (DI, philox, u4, PI_F).
//
// Why: with a policy in the loop a rollout step in PyTorch is ~100 launches of a few microseconds (float64 running statistics, two 3-layer MLPs,
// sampling, clipping, buffer copies) around a 15 us simulator kernel -- 300 us per step even when replayed as a graph.  Here:
//   usim_policy_obs_stats   RunningMeanStd.update on the observation batch (float64 batch moments, parallel-variance merge), one workgroup per channel
//   usim_policy_act         normalise + clip the observation, both MLPs on the matrix cores (v_mfma_f32_16x16x4_f32, fp32 in / fp32 accumulate),
//                           Gaussian sample from a counter-based stream, log-probability, clip to the action box; writes the rollout-buffer
//                           slices (normalised observation, unclipped action, value, log-prob, episode start) and the env's action
//   [usim_step]
//   usim_policy_reward      discounted-return statistics (RunningMeanStd on the returns), reward normalisation + clip, buffer write
//   usim_policy_gae         RolloutBuffer.compute_returns_and_advantage, one thread per environment, once per rollout
// or, up to 8192 environments, two launches per step:
//   usim_policy_step_fused  the policy launch with both VecNormalize updates inside: its workgroups exchange partial sums through device-scope stores /
//                           loads and arrival flags (no fences: see the kernel), then normalise and run the MLPs as above
//   [usim_step]
// and, where the caller asks for it, one more small launch per step:
//   usim_policy_bootstrap   += gamma V(terminal observation) on the rewards of the environments that ended at the time limit (see the kernel)
// and for K networks over K G environments (population.py) the same workgroups with the member on one more grid axis:
//   usim_policy_pack_multi / usim_policy_step_multi / usim_policy_reward_multi   K single-network calls on the members' slices in one launch each, bit for bit
// The weights are read from the caller's tensors (torch parameters: an optimiser step is seen by the next call); nothing is copied.
// Numerics: same formulas as policy.DeviceVecNormalize / MlpActorCritic; sums are ordered differently from PyTorch's kernels, so results agree to
// rounding (tests/test_gpu_policy_replay.py: 1e-5 on means / values / log-probs, 1e-12 relative on the float64 statistics), not bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#include "../../include/usim.h"
#include "usim_devmath.h"

using namespace usim;

namespace usim {

constexpr int PL_OBS = 19, PL_KPAD = 20, PL_H1 = 256, PL_H2 = 128, PL_TM = 32;          // MlpPolicy of the shipped checkpoints: 19 -> 256 -> 128 -> A / 1
constexpr int PL_H1S = PL_H1 + 4, PL_H2S = PL_H2 + 4;                                    // LDS row strides (260, 132: 16-byte aligned, off the 32-bank period)

struct PolicyNet {                                       // torch.nn.Linear layouts: weight [out][in], bias [out]
    const float *pi_w1, *pi_b1, *pi_w2, *pi_b2, *act_w, *act_b;      // policy_net (19 -> 256 -> 128, tanh), action_net (128 -> A)
    const float *vf_w1, *vf_b1, *vf_w2, *vf_b2, *val_w, *val_b;      // value_net_body, value_net (128 -> 1)
    const float* log_std;                                             // [A]
    const float4* w2_packed;                                          // layer-2 weights of both networks in operand order (usim_policy_pack), or nullptr
};
struct NormStats {                                       // policy.DeviceVecNormalize: float64 tensors, updated in place
    double *obs_mean, *obs_var, *obs_count;              // [19], [19], scalar
    double *ret_mean, *ret_var, *ret_count, *returns;    // scalars, [n]
    double clip_obs, clip_reward, gamma, epsilon;
};

DI double ld_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DI void st_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// RunningMeanStd.update_from_moments: merges a batch of n samples (sum x, sum x^2) into a running mean / variance over `count` samples (parallel-variance
// update); returns the new count.  (-ffp-contract=on fuses per statement: the statements are part of the result)
DI double merge_moments(double& mean, double& var, double count, double sum, double sum_sq, int n) {
    const double bm = sum / n, bv = fmax(sum_sq / n - bm * bm, 0.0);
    const double tot = count + n, delta = bm - mean;
    const double m2 = var * count + bv * n + delta * delta * count * n / tot;
    mean += delta * n / tot; var = m2 / tot;
    return tot;
}

// RunningMeanStd.update(obs).  PL_SB workgroups read their slice of the [n][19] batch once, coalesced (thread t takes words t, t + 128, ...: the
// channel of a word is its index mod 19, and since 128 * 19 words form a block, slot j of a thread always holds channel (first + t + 128 j) mod 19 --
// nineteen slots, nineteen different channels), and leave per-channel partial sums (sum x, sum x^2 in float64) in `part`.  The workgroup that
// finishes last adds the partials in a fixed order -- the result does not depend on which one that is -- and merges the batch moments into the
// running statistics (parallel-variance update of RunningMeanStd.update_from_moments).
constexpr int PL_SB = 32, PL_ST = 128;                           // workgroups, threads per workgroup
struct ObsStatsLds { double tabx[PL_OBS][PL_ST], tabq[PL_OBS][PL_ST]; bool last; };
DI void obs_stats_body(ObsStatsLds& L, const float* __restrict__ obs, int n, const NormStats& S, double* __restrict__ part, unsigned int* __restrict__ arrived) {
    // (executed by the first PL_ST threads of workgroups 0 .. PL_SB - 1; every barrier below is passed by all of them)
    double (&tabx)[PL_OBS][PL_ST] = L.tabx; double (&tabq)[PL_OBS][PL_ST] = L.tabq; bool& last = L.last;
    const int t = threadIdx.x, total = n * PL_OBS;
    const int per = ((total + PL_SB - 1) / PL_SB + PL_OBS - 1) / PL_OBS * PL_OBS;      // a multiple of 19: every slice starts at channel 0
    const int lo = blockIdx.x * per, hi = min(total, lo + per);
    const bool act = t < PL_ST;                                    // (a workgroup may bring more threads than the PL_ST that work here)
    double sx[PL_OBS], sq[PL_OBS];
#pragma unroll
    for (int j = 0; j < PL_OBS; ++j) { sx[j] = 0.0; sq[j] = 0.0; }
    if (act) {
        for (int b = lo; b < hi; b += PL_ST * PL_OBS) {
#pragma unroll
            for (int j = 0; j < PL_OBS; ++j) {
                const int w = b + t + PL_ST * j;
                const double x = (w < hi) ? (double)obs[w] : 0.0;
                sx[j] += x; sq[j] += x * x;
            }
        }
#pragma unroll
        for (int j = 0; j < PL_OBS; ++j) { const int ch = (t + PL_ST * j) % PL_OBS; tabx[ch][t] = sx[j]; tabq[ch][t] = sq[j]; }
    }
    __syncthreads();
    if (t < PL_OBS * 4) {                                          // four lanes per channel, 32 table entries each, combined in a fixed order
        const int c = t >> 2, seg = t & 3;
        double a = 0.0, b = 0.0;
#pragma unroll 8
        for (int k = seg * (PL_ST / 4); k < (seg + 1) * (PL_ST / 4); ++k) { a += tabx[c][k]; b += tabq[c][k]; }
        a += __shfl_xor(a, 1); b += __shfl_xor(b, 1); a += __shfl_xor(a, 2); b += __shfl_xor(b, 2);
        if (seg == 0) { st_agent(&part[(blockIdx.x * PL_OBS + c) * 2], a); st_agent(&part[(blockIdx.x * PL_OBS + c) * 2 + 1], b); }
    }
    // (no __threadfence: a device-scope fence writes back / invalidates the XCD's L2 once per wave; the partial sums travel as device-scope accesses and the
    //  arrival count follows them in program order -- see the fused policy kernel below)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) last = __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(PL_SB - 1);
    __syncthreads();
    if (!last) return;
    if (t < PL_OBS) {
        double2 pp[PL_SB];                                        // all loads first (independent), then the sums in a fixed order
#pragma unroll
        for (int k = 0; k < PL_SB; ++k) pp[k] = make_double2(ld_agent(&part[(k * PL_OBS + t) * 2]), ld_agent(&part[(k * PL_OBS + t) * 2 + 1]));
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int k = 0; k < PL_SB; ++k) { a += pp[k].x; b += pp[k].y; }
        merge_moments(S.obs_mean[t], S.obs_var[t], *S.obs_count, a, b, n);
    }
    __syncthreads();
    if (t == 0) { *S.obs_count += n; *arrived = 0u; }
}
__global__ __launch_bounds__(PL_ST) void usim_policy_obs_stats_kernel(const float* __restrict__ obs, int n, NormStats S, double* __restrict__ part,
                                                                      unsigned int* __restrict__ arrived) {
    __shared__ ObsStatsLds L;
    obs_stats_body(L, obs, n, S, part, arrived);
}

typedef float v4f_ __attribute__((ext_vector_type(4)));
typedef _Float16 v4h_ __attribute__((ext_vector_type(4)));
// float32 as the sum of two float16 words (hi = round(x), lo = round(x - hi)): x = hi + lo to 2^-22 |x| (down to the float16 subnormal step, 6e-8, for small x)
DI void split_h(const float x, _Float16& hi, _Float16& lo) { hi = (_Float16)x; lo = (_Float16)(x - (float)hi); }
// tanh(x) = 1 - 2 / (exp(2x) + 1): v_exp_f32 + v_rcp_f32 (absolute error ~1e-7; saturates to +-1 through exp -> inf / 0), a tenth of the library routine
DI float tanh_(float x) { const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f); return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f); }

// One workgroup = 32 environments through ONE of the two networks (blockIdx.y: 0 policy, 1 value): 256 workgroups at 4096 environments.
// Measured at 4096 environments (rocprofv3, by early exits): weight prefetch + observation normalisation 5.0 us, layer 1 +1.5, layer 2 +7.2, heads
// + sampling +2.7 = 16 us -- of which the 9.5 k matrix-core cycles of a wave are 4 us; replacing the layer-2 instructions by plain multiply-adds,
// halving the weight traffic (32 rows x one network instead of 16 rows x both: 78 -> 39 MB of L2 reads), rotating the order in which the
// workgroups walk the weights, prefetching them into registers at the top: none of them moved the total -- what is left is the per-CU rate at
// which a wave's 16-row x 64-byte operand reads go through the texture cache.
// Matrix-core layout (v_mfma_f32_16x16x4_f32): lane l supplies A[row l % 16][k l / 16] and B[k l / 16][col l % 16], receives
// D[row 4 (l / 16) + r][col l % 16] in accumulator register r.  The k order inside a group of 16 is free as long as A and B agree: group g = l / 16
// takes k = 16 s + 4 g + j in the j-th of four instructions, so that both operands are 16-byte reads.
//
// FUSED: both halves of VecNormalize.step_wait move into this kernel, so that a rollout step is two launches (policy, simulator) instead of three.
// The statistics need sums over ALL environments before any can be normalised: the policy workgroups (blockIdx.y = 0) leave the float64 moments of
// their own 32 environments (19 channels: sum x, sum x^2; discounted returns of the step before: sum r, sum r^2; sum of raw rewards) in a workspace row,
// raise a flag each, and every workgroup waits until all flags are up, adds them in row order (all arrive at the same
// bits), merges them into the running statistics it read BEFORE the wait and normalises its environments; workgroup (0, 0) stores the merged statistics
// AFTER the wait, so nobody can read them half-updated.  The grid is at most 2 x 256 workgroups of which two fit a CU (LDS 76 KB, 4 waves): all are
// resident, which the wait relies on; it is bounded all the same (a status word is raised and the kernel carries on with whatever rows it sees rather than
// hang).  Measured alternative: every workgroup reducing the whole batch by itself (no wait) -- 256 x 311 KB through L2 cost 20-27 us per launch.
// Layer-2 weights in operand order.  torch.nn.Linear stores weight[out][in]: the sixteen columns of a matrix-core operand are sixteen rows 1 KB apart, so a wave's
// 16-byte operand reads touch sixteen cache lines per instruction (3 of the kernel's 16 us at 4096 environments: rocprofv3 with the reads cut out).  usim_policy_pack
// rewrites the two matrices once per weight update as [network][wave][column tile][k step][lane] float4 -- the word lane (lr, lg) of wave w consumes at step s --
// and the policy kernel then reads 1 KB contiguous per instruction.  The words are stored SPLIT, each float32 as two float16 (split_h): layer 2 then runs as three
// float16 matrix-core products per tile -- hi hi + hi lo + lo hi, float32 accumulate, 2^-22 relative per product against 2^-24 -- at 8 cycles per 16 x 16 x 16
// instead of four float32 instructions of 32 cycles each: 3.7 us of the launch become 0.8.
DI int pl_packed_index(int net, int wave, int tile, int s, int lane) { return (((net * 4 + wave) * 2 + tile) * (PL_H1 / 16) + s) * 64 + lane; }
DI void pack_body(const float* __restrict__ pi_w2, const float* __restrict__ vf_w2, float4* __restrict__ packed) {
    const int idx = blockIdx.x * 256 + threadIdx.x;                    // one float4 per thread: 2 * 4 * 2 * 16 * 64 = 16384
    if (idx >= 2 * 4 * 2 * (PL_H1 / 16) * 64) return;
    const int lane = idx & 63, s = (idx >> 6) & 15, tile = (idx >> 10) & 1, wave = (idx >> 11) & 3, net = idx >> 13;
    const int lr = lane & 15, lg = lane >> 4, col = (wave * 2 + tile) * 16 + lr, k = 16 * s + 4 * lg;
    const float4 w = *reinterpret_cast<const float4*>(&(net ? vf_w2 : pi_w2)[col * PL_H1 + k]);
    union { struct { v4h_ hi, lo; } h; float4 f; } u;                  // the four words' high parts, then their low parts: 16 bytes, as before
    _Float16 a, b;
    split_h(w.x, a, b); u.h.hi[0] = a; u.h.lo[0] = b; split_h(w.y, a, b); u.h.hi[1] = a; u.h.lo[1] = b;
    split_h(w.z, a, b); u.h.hi[2] = a; u.h.lo[2] = b; split_h(w.w, a, b); u.h.hi[3] = a; u.h.lo[3] = b;
    packed[idx] = u.f;
}
__global__ __launch_bounds__(256) void usim_policy_pack_kernel(const float* __restrict__ pi_w2, const float* __restrict__ vf_w2, float4* __restrict__ packed) {
    pack_body(pi_w2, vf_w2, packed);
}

constexpr int PL_ROW = 48, PL_SG = 13;                          // doubles per workspace row (38 observation moments, 3 reward moments); segments of the final sum
constexpr unsigned PL_SPIN = 1u << 17;                             // polls before a wait gives up (~0.1 s; a wait that succeeds takes 5-10 us)
struct FusedArgs {
    const float* rew_prev; const uint8_t* done_prev; float* nrew_prev; double* raw_sum;
    double* work;                                                // [gridDim.x][PL_ROW] rows, then 2 gridDim.x arrival flags + a status word (32-bit words)
    int update_obs, have_prev, norm_reward;
};
struct FusedLds { double mean[PL_OBS], var[PL_OBS], inv[PL_OBS]; double scale; };             // (the raw observations sit where their normalised values go; the partial sums borrow h2)
struct FusedTab { double tab[2][PL_SG][PL_OBS]; double red[3][4]; };
static_assert(sizeof(FusedTab) <= PL_TM * PL_H2S * sizeof(float), "partial sums fit the layer-2 output buffer");

// Diagnostics (never in the shipped library): -DUSIM_POLICY_CUT=1 / 2 / 3 ends the kernel before layer 1 / before layer 2 / before the heads, -DUSIM_POLICY_NOLOAD replaces the
// layer-2 weight reads by constants -- the kernel's time by phase under rocprofv3.
// The workgroup's work is a device function: the single-network kernels below call it with their arguments as they are, the population kernel
// (usim_policy_act_multi_kernel) with the pointers of the member its blockIdx.z names.  It reads blockIdx.x (the 32 environments), blockIdx.y (the network)
// and, FUSED only, gridDim.x; everything else comes through its arguments.
template <bool FUSED>
DI void policy_act_body(PolicyNet P, NormStats S, const float* __restrict__ obs,
                        const uint8_t* __restrict__ prev_done, int n, int adim, const float* __restrict__ act_low,
                        const float* __restrict__ act_high, uint32_t key0, uint32_t key1, uint32_t ctr0, const uint32_t* __restrict__ ctr_base, int env_offset,
                        int deterministic, float* __restrict__ nobs_out, float* __restrict__ act_out,
                        float* __restrict__ act_env, float* __restrict__ value_out, float* __restrict__ logp_out,
                        float* __restrict__ start_out, FusedArgs F) {
    __shared__ FusedLds FL;
    __shared__ __attribute__((aligned(16))) float xs[PL_TM][PL_KPAD];
    __shared__ __attribute__((aligned(16))) _Float16 h1h[PL_TM][PL_H1 + 8], h1l[PL_TM][PL_H1 + 8];      // layer-1 activations, split (split_h); row stride 528 bytes
    __shared__ __attribute__((aligned(16))) float h2[PL_TM][PL_H2S];
    __shared__ __attribute__((aligned(16))) float w1s[PL_H1 * PL_OBS];        // layer-1 weights [256][19] of this workgroup's network
    __shared__ __attribute__((aligned(16))) float whs[8 * PL_H2];             // head weights: action_net [A][128] or value_net [1][128]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, net = blockIdx.y, row0 = blockIdx.x * PL_TM;
    const int lr = lane & 15, lg = lane >> 4;
    const uint32_t ctr = ctr0 + (ctr_base ? *ctr_base : 0u);                  // call counter: host part + a device word (a recorded graph advances the latter)
    // ---- every weight read is issued up front: this lane's layer-2 operands into registers (2 column tiles x 256 k = 32 x 16 bytes; they are
    //      consumed two barriers later, so their L2 latency is covered by the normalisation and layer 1), layer-1 and head weights into LDS with
    //      coalesced loads ----
    const int c0 = (wave * 2) * 16 + lr, c1 = c0 + 16;
    float4 wb0[PL_H1 / 16], wb1[PL_H1 / 16];
    // ... and every small parameter a later phase needs (biases, log-std, action box): read where they are used, each of them exposes an L2 round trip behind a barrier
    float4 pb1[4], pb2[2];
    float ph[4] = {0.f, 0.f, 0.f, 0.f};
    auto prefetch = [&]() {
        {
            const float* B1 = net ? P.vf_b1 : P.pi_b1; const float* B2 = net ? P.vf_b2 : P.pi_b2;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) pb1[tt] = *reinterpret_cast<const float4*>(&B1[(wave * 4 + tt) * 16 + 4 * lg]);      // (this lane's four output features of the tile)
            pb2[0] = *reinterpret_cast<const float4*>(&B2[(wave * 2) * 16 + 4 * lg]); pb2[1] = *reinterpret_cast<const float4*>(&B2[(wave * 2 + 1) * 16 + 4 * lg]);
            const int o = tid & 7;
            if (net == 0) { if (o < adim) { ph[0] = P.act_b[o]; ph[1] = P.log_std[o]; ph[2] = act_low[o]; ph[3] = act_high[o]; } }
            else ph[0] = P.val_b[0];
        }
#pragma unroll
        for (int s = 0; s < PL_H1 / 16; ++s) {
            const int k = 16 * s + 4 * lg;
#if defined(USIM_POLICY_NOLOAD)
            wb0[s] = make_float4(0.001f * k, 0.f, 0.002f, 0.f); wb1[s] = make_float4(0.f, 0.001f * lr, 0.f, 0.003f);
#else
            wb0[s] = P.w2_packed[pl_packed_index(net, wave, 0, s, lane)]; wb1[s] = P.w2_packed[pl_packed_index(net, wave, 1, s, lane)];
#endif
        }
        const float4* W1 = reinterpret_cast<const float4*>(net ? P.vf_w1 : P.pi_w1);
#pragma unroll
        for (int i = 0; i < (PL_H1 * PL_OBS / 4 + 255) / 256; ++i) { const int v = tid + 256 * i; if (v < PL_H1 * PL_OBS / 4) reinterpret_cast<float4*>(w1s)[v] = W1[v]; }
        const int nh = (net ? 1 : adim) * PL_H2 / 4;
        const float4* WH = reinterpret_cast<const float4*>(net ? P.val_w : P.act_w);
        if (tid < nh) reinterpret_cast<float4*>(whs)[tid] = WH[tid];
    };
    if constexpr (!FUSED) prefetch();
    if constexpr (FUSED) {
        const int nrow = gridDim.x;
        FusedTab& FT = *reinterpret_cast<FusedTab*>(&h2[0][0]);
        unsigned int* flags = reinterpret_cast<unsigned int*>(F.work + (size_t)nrow * PL_ROW);        // [2 nrow] arrival flags (one per workgroup), then a status word
        const unsigned epoch = 2u * ctr + 1u;                                                          // this call's flag value (never 0, new for every counter)
        const bool writer = blockIdx.x == 0 && net == 0;
        // the running statistics as they are before this call (read before the wait; stored only after it)
        double om = 0.0, ov = 0.0;
        if (tid < PL_OBS) { om = S.obs_mean[tid]; ov = S.obs_var[tid]; }
        const double ocnt = *S.obs_count, rmean0 = *S.ret_mean, rvar0 = *S.ret_var, rcnt0 = *S.ret_count;
        // this workgroup's raw observations
        for (int t = tid; t < PL_TM * PL_KPAD; t += 256) {
            const int r = t / PL_KPAD, c = t - r * PL_KPAD, env = row0 + r;
            xs[r][c] = (c < PL_OBS && env < n) ? obs[(size_t)env * PL_OBS + c] : 0.f;
        }
        __syncthreads();
        if (net == 0) {
            double* row = F.work + (size_t)blockIdx.x * PL_ROW;
            if (tid < 4 * PL_OBS) {                                // four lanes per channel, eight environments each
                const int c = tid >> 2, seg = tid & 3;
                double a = 0.0, b = 0.0;
                if (F.update_obs) {
#pragma unroll
                    for (int r = 8 * seg; r < 8 * seg + 8; ++r) { const double x = (double)xs[r][c]; a += x; b = fma(x, x, b); }
                }
                a += __shfl_xor(a, 1); b += __shfl_xor(b, 1); a += __shfl_xor(a, 2); b += __shfl_xor(b, 2);
                if (seg == 0) { st_agent(&row[2 * c], a); st_agent(&row[2 * c + 1], b); }
            } else if (tid >= 128 && tid < 128 + PL_TM) {          // (a wave of its own) the reward side of the step before, this workgroup's environments
                const int i = row0 + (tid - 128);
                double rw = 0.0, r = 0.0;
                if (F.have_prev && i < n) {
                    rw = (double)F.rew_prev[i]; r = fma(S.returns[i], S.gamma, rw);
                    S.returns[i] = F.done_prev[i] ? 0.0 : r;
                }
                double a = rw, b = r, c = r * r;
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
                if (tid == 128) { st_agent(&row[2 * PL_OBS], a); st_agent(&row[2 * PL_OBS + 1], b); st_agent(&row[2 * PL_OBS + 2], c); }
            }
        }
        // every workgroup of both networks announces itself: its rows are written and its reads of the old statistics have returned
        // No agent-scope fences: a release writes the XCD's L2 back and an acquire invalidates it, per wave (128 of each per XCD: 25 us per launch).  The rows
        // and flags are written and read with device-scope accesses instead (they go to the memory side directly); the flag follows the rows by program order:
        // every wave's stores (and its reads of the old statistics) have returned before it reaches the workgroup barrier.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&flags[net * nrow + blockIdx.x], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        prefetch();                                                 // (after the flag: the wait above would have had to drain these loads too; they fly during the wait below)
        // ---- wait for all of them (bounded): thread t watches flag t -- a counter that 2 x 128 workgroups on 8 XCDs add to costs ~50 us per launch ----
        int gave_up = 0;
        if (wave == 3) {                                            // one wave watches: lane l takes flags 2 l, 2 l + 1 (+ 128 j) as one 8-byte word
            const unsigned long long want = ((unsigned long long)epoch << 32) | epoch;
            const unsigned long long* f2 = reinterpret_cast<const unsigned long long*>(flags);
            for (int k = lane; k < nrow; k += 64) {                 // (2 nrow flags = nrow words)
                unsigned spins = 0;
                while (__hip_atomic_load(&f2[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {     // (relaxed: an acquire per poll invalidates the caches per poll)
                    __builtin_amdgcn_s_sleep(8);
                    if (++spins > PL_SPIN) { flags[2 * nrow] = 1u; gave_up = 1; break; }
                }
            }
        }
        // a workgroup whose own wait ran out has partial sums: it goes on (its launch must end) but, if it is the writer, leaves the caller's running statistics
        // untouched -- FusedRollout.collect() raises on the status word, and VecNormalize is then still the one of the rollout before
        const bool stats_ok = __syncthreads_or(gave_up) == 0;
        // ---- all rows in row order: thread (g, c) takes rows g, g + 13, ... of channel c -- every load issued before the first sum (a load that has to
        //      leave the XCD takes ~2 us; 128 of them one after the other was 50 us) --; then the 13 partial sums in order ----
        constexpr int JMAX = (USIM_POLICY_FUSED_MAX_ENVS / PL_TM + PL_SG - 1) / PL_SG;
        if (tid < PL_SG * PL_OBS) {
            const int g = tid / PL_OBS, c = tid - g * PL_OBS;
            double a = 0.0, b = 0.0;
            if (F.update_obs) {
                double2 v[JMAX];
#pragma unroll
                for (int j = 0; j < JMAX; ++j) {
                    const int k = g + PL_SG * j;
                    v[j] = (k < nrow) ? make_double2(ld_agent(&F.work[(size_t)k * PL_ROW + 2 * c]), ld_agent(&F.work[(size_t)k * PL_ROW + 2 * c + 1])) : make_double2(0.0, 0.0);
                }
#pragma unroll
                for (int j = 0; j < JMAX; ++j) { a += v[j].x; b += v[j].y; }
            }
            FT.tab[0][g][c] = a; FT.tab[1][g][c] = b;
        }
        if (F.have_prev) {                                          // the three reward sums: row t in thread t, then wave butterflies and the four wave sums in order
            double a = 0.0, b = 0.0, c = 0.0;
            if (tid < nrow) { const double* row = F.work + (size_t)tid * PL_ROW + 2 * PL_OBS; a = ld_agent(&row[0]); b = ld_agent(&row[1]); c = ld_agent(&row[2]); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
            if (lane == 0) { FT.red[0][wave] = a; FT.red[1][wave] = b; FT.red[2][wave] = c; }
        }
        __syncthreads();
        if (tid < PL_OBS) {
            if (F.update_obs) {
                double a = 0.0, b = 0.0;
#pragma unroll
                for (int g = 0; g < PL_SG; ++g) { a += FT.tab[0][g][tid]; b += FT.tab[1][g][tid]; }
                const double tot = merge_moments(om, ov, ocnt, a, b, n);
                if (writer && stats_ok) { S.obs_mean[tid] = om; S.obs_var[tid] = ov; if (tid == 0) *S.obs_count = tot; }
            }
            FL.mean[tid] = om; FL.var[tid] = ov; FL.inv[tid] = 1.0 / sqrt(ov + S.epsilon);
        } else if (tid == 64) {
            double rmean = rmean0, rvar = rvar0, rcnt = rcnt0;
            if (F.have_prev) {
                const double a = (FT.red[0][0] + FT.red[0][1]) + (FT.red[0][2] + FT.red[0][3]), b = (FT.red[1][0] + FT.red[1][1]) + (FT.red[1][2] + FT.red[1][3]),
                             c = (FT.red[2][0] + FT.red[2][1]) + (FT.red[2][2] + FT.red[2][3]);
                rcnt = merge_moments(rmean, rvar, rcnt, b, c, n);
                if (writer && stats_ok) { *S.ret_mean = rmean; *S.ret_var = rvar; *S.ret_count = rcnt; if (F.raw_sum) *F.raw_sum += a; }
            }
            FL.scale = 1.0 / sqrt(rvar + S.epsilon);
        }
        __syncthreads();
        if (F.have_prev && net == 0 && tid < PL_TM && row0 + tid < n) {
            double v = (double)F.rew_prev[row0 + tid];
            if (F.norm_reward) { v *= FL.scale; v = v < -S.clip_reward ? -S.clip_reward : (v > S.clip_reward ? S.clip_reward : v); }
            F.nrew_prev[row0 + tid] = (float)v;
        }
    }
    // ---- VecNormalize.normalize_obs: clip((obs - mean) / sqrt(var + eps)) in float64, stored as float32 (the nineteen reciprocal deviations once per workgroup:
    //      a float64 square root and a division per word were a microsecond of the launch) ----
    constexpr int NX = (PL_TM * PL_KPAD + 255) / 256;
    float xraw[NX];
    if constexpr (!FUSED) {
        // (the observation words are requested before the statistics are waited for: one round trip to L2, not two)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int t = tid + 256 * j, r = t / PL_KPAD, c = t - r * PL_KPAD, env = row0 + r;
            xraw[j] = (t < PL_TM * PL_KPAD && c < PL_OBS && env < n) ? obs[(size_t)env * PL_OBS + c] : 0.f;
        }
        if (tid < PL_OBS) { FL.mean[tid] = S.obs_mean[tid]; FL.inv[tid] = 1.0 / sqrt(S.obs_var[tid] + S.epsilon); }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        const int t = tid + 256 * j;
        if (t >= PL_TM * PL_KPAD) break;
        const int r = t / PL_KPAD, c = t - r * PL_KPAD, env = row0 + r;
        float v = 0.f;
        if (c < PL_OBS && env < n) {
            double x = ((double)(FUSED ? xs[r][c] : xraw[j]) - FL.mean[c]) * FL.inv[c];
            x = x < -S.clip_obs ? -S.clip_obs : (x > S.clip_obs ? S.clip_obs : x);
            v = (float)x;
            if (nobs_out && net == 0) nobs_out[(size_t)env * PL_OBS + c] = v;
        }
        xs[r][c] = v;
    }
    __syncthreads();
#if defined(USIM_POLICY_CUT) && USIM_POLICY_CUT == 1
    if (value_out) { if (tid == 0) value_out[row0] = xs[0][0] + wb0[0].x + wb1[3].y; return; }
#endif
    // ---- layer 1 (19 -> 256, tanh): wave w owns feature tiles 4 w .. 4 w + 3, both environment tiles.  Transposed product (features x environments = W1 X'): the
    //      four accumulator words of a lane are four CONSECUTIVE features of one environment -- one 8-byte store per split half instead of eight 2-byte ones ----
    {
        const float* W = w1s;
        const float* B = net ? P.vf_b1 : P.pi_b1;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int col = (wave * 4 + tt) * 16 + lr;
            v4f_ acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < PL_KPAD / 4; ++s) {
                const int k = 4 * s + lg;
                const float b = (k < PL_OBS) ? W[col * PL_OBS + k] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(b, xs[lr][k], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b, xs[16 + lr][k], acc1, 0, 0, 0);
            }
            const float bias[4] = {pb1[tt].x, pb1[tt].y, pb1[tt].z, pb1[tt].w};
            const int f0 = (wave * 4 + tt) * 16 + 4 * lg;
            v4h_ h0, l0, h1v, l1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                _Float16 a, b2;
                split_h(tanh_(acc0[r] + bias[r]), a, b2); h0[r] = a; l0[r] = b2;
                split_h(tanh_(acc1[r] + bias[r]), a, b2); h1v[r] = a; l1[r] = b2;
            }
            *reinterpret_cast<v4h_*>(&h1h[lr][f0]) = h0; *reinterpret_cast<v4h_*>(&h1l[lr][f0]) = l0;
            *reinterpret_cast<v4h_*>(&h1h[16 + lr][f0]) = h1v; *reinterpret_cast<v4h_*>(&h1l[16 + lr][f0]) = l1;
        }
    }
    __syncthreads();
#if defined(USIM_POLICY_CUT) && USIM_POLICY_CUT == 2
    if (value_out) { if (tid == 0) value_out[row0] = (float)h1h[0][0] + wb0[0].x + wb1[3].y; return; }
#endif
    // ---- layer 2 (256 -> 128, tanh): wave w owns column tiles 2 w, 2 w + 1 for both row tiles; 16 k values per pass (one 16-byte read per operand,
    //      four instructions per accumulator): a weight word read once serves 32 environments ----
    {
        const float* B = net ? P.vf_b2 : P.pi_b2;
        v4f_ a00 = {0.f, 0.f, 0.f, 0.f}, a01 = {0.f, 0.f, 0.f, 0.f}, a10 = {0.f, 0.f, 0.f, 0.f}, a11 = {0.f, 0.f, 0.f, 0.f};     // [row tile][column tile]
#pragma unroll
        for (int s = 0; s < PL_H1 / 16; ++s) {
            const int k = 16 * s + 4 * lg;
            const v4h_ x0h = *reinterpret_cast<const v4h_*>(&h1h[lr][k]), x0l = *reinterpret_cast<const v4h_*>(&h1l[lr][k]);
            const v4h_ x1h = *reinterpret_cast<const v4h_*>(&h1h[16 + lr][k]), x1l = *reinterpret_cast<const v4h_*>(&h1l[16 + lr][k]);
            union W { float4 f; struct { v4h_ hi, lo; } h; };
            W b0, b1; b0.f = wb0[s]; b1.f = wb1[s];
            // three products per tile, the small ones first
#define USIM_MM3(ACC, XH, XL, BB) ACC = __builtin_amdgcn_mfma_f32_16x16x16f16(BB.h.hi, XL, ACC, 0, 0, 0); ACC = __builtin_amdgcn_mfma_f32_16x16x16f16(BB.h.lo, XH, ACC, 0, 0, 0); \
                                  ACC = __builtin_amdgcn_mfma_f32_16x16x16f16(BB.h.hi, XH, ACC, 0, 0, 0);          /* (outputs x environments: W2 H1') */
            USIM_MM3(a00, x0h, x0l, b0) USIM_MM3(a01, x0h, x0l, b1) USIM_MM3(a10, x1h, x1l, b0) USIM_MM3(a11, x1h, x1l, b1)
#undef USIM_MM3
        }
        // (transposed as layer 1: a lane holds four consecutive outputs of one environment -- one 16-byte store per tile)
        const int n0 = (wave * 2) * 16 + 4 * lg, n1 = n0 + 16;
        const float4 bz0 = pb2[0], bz1 = pb2[1];
        *reinterpret_cast<float4*>(&h2[lr][n0]) = make_float4(tanh_(a00[0] + bz0.x), tanh_(a00[1] + bz0.y), tanh_(a00[2] + bz0.z), tanh_(a00[3] + bz0.w));
        *reinterpret_cast<float4*>(&h2[lr][n1]) = make_float4(tanh_(a01[0] + bz1.x), tanh_(a01[1] + bz1.y), tanh_(a01[2] + bz1.z), tanh_(a01[3] + bz1.w));
        *reinterpret_cast<float4*>(&h2[16 + lr][n0]) = make_float4(tanh_(a10[0] + bz0.x), tanh_(a10[1] + bz0.y), tanh_(a10[2] + bz0.z), tanh_(a10[3] + bz0.w));
        *reinterpret_cast<float4*>(&h2[16 + lr][n1]) = make_float4(tanh_(a11[0] + bz1.x), tanh_(a11[1] + bz1.y), tanh_(a11[2] + bz1.z), tanh_(a11[3] + bz1.w));
    }
    __syncthreads();
#if defined(USIM_POLICY_CUT) && USIM_POLICY_CUT == 3
    if (value_out) { if (tid == 0) value_out[row0] = h2[0][0]; return; }
#endif
    // ---- head: eight lanes per environment.  Policy network: lane o < A forms the mean of action component o (128 -> A), then sampling and the
    //      log-probability; value network: the eight lanes split the 128 -> 1 dot product ----
    const int r = tid >> 3, o = tid & 7, env = row0 + r;
    if (net == 0) {
        const bool is_act = o < adim;
        const float* Wr = whs + (is_act ? o : 0) * PL_H2;
        float acc = 0.f, bcc = 0.f;
#pragma unroll 8
        for (int k = 0; k < PL_H2; k += 4) {
            const float4 h = *reinterpret_cast<const float4*>(&h2[r][k]);
            const float4 w = *reinterpret_cast<const float4*>(&Wr[k]);
            acc = fmaf(h.x, w.x, acc); bcc = fmaf(h.y, w.y, bcc); acc = fmaf(h.z, w.z, acc); bcc = fmaf(h.w, w.w, bcc);
        }
        const float mean = acc + bcc + ph[0];
        // N(0, 1) for (environment, component): Box-Muller on one Philox block per pair of components
        float noise = 0.f;
        if (!deterministic && is_act) {
            const u4 rr = philox((uint32_t)(env_offset + env), ctr, (uint32_t)(o >> 1), 0x504f4c59u, key0, key1);
            const float u1 = ((float)(rr.a >> 8) + 1.0f) * (1.0f / 16777216.0f), u2 = (float)(rr.b >> 8) * (1.0f / 16777216.0f);
            const float rad = sqrtf(-2.f * __logf(u1)), ang = 2.f * PI_F * u2;        // (hardware log / sine / cosine: the draw is a sample, not a result to reproduce)
            noise = (o & 1) ? rad * __sinf(ang) : rad * __cosf(ang);
        }
        const float ls = is_act ? ph[1] : 0.f;
        const float a = mean + __expf(ls) * noise;
        // DiagGaussianDistribution.log_prob of the sample: sum over the components (the eight lanes of this environment)
        float lp = is_act ? (-0.5f * noise * noise - ls - 0.9189385332046727f) : 0.f;
        lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4);
        if (env < n) {
            if (is_act) {
                if (act_out) act_out[(size_t)env * adim + o] = a;
                act_env[(size_t)env * adim + o] = fminf(fmaxf(a, ph[2]), ph[3]);
            }
            if (o == 0) {
                if (logp_out) logp_out[env] = lp;
                if (start_out) start_out[env] = prev_done ? (prev_done[env] ? 1.f : 0.f) : 1.f;
            }
        }
    } else {
        float acc = 0.f;
#pragma unroll
        for (int k = 16 * o; k < 16 * o + 16; k += 4) {
            const float4 h = *reinterpret_cast<const float4*>(&h2[r][k]);
            const float4 w = *reinterpret_cast<const float4*>(&whs[k]);
            acc = fmaf(h.x, w.x, acc); acc = fmaf(h.y, w.y, acc); acc = fmaf(h.z, w.z, acc); acc = fmaf(h.w, w.w, acc);
        }
        acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4);
        if (env < n && o == 0 && value_out) value_out[env] = acc + ph[0];
    }
}
template <bool FUSED>
__global__ __launch_bounds__(256, 2) void usim_policy_act_kernel(PolicyNet P, NormStats S, const float* __restrict__ obs,
                                                              const uint8_t* __restrict__ prev_done, int n, int adim, const float* __restrict__ act_low,
                                                              const float* __restrict__ act_high, uint32_t key0, uint32_t key1, uint32_t ctr0, const uint32_t* __restrict__ ctr_base, int env_offset,
                                                              int deterministic, float* __restrict__ nobs_out, float* __restrict__ act_out,
                                                              float* __restrict__ act_env, float* __restrict__ value_out, float* __restrict__ logp_out,
                                                              float* __restrict__ start_out, FusedArgs F) {
    policy_act_body<FUSED>(P, S, obs, prev_done, n, adim, act_low, act_high, key0, key1, ctr0, ctr_base, env_offset, deterministic, nobs_out, act_out, act_env, value_out,
                           logp_out, start_out, F);
}

// ---- policy populations: K networks over n = K G environments, member k owning environments [k G, (k + 1) G).  The unit of work above is already 32 environments x
//      one network, and a workgroup reads its weights once whichever network they are: the member is one more grid axis (blockIdx.z for the policy launch, blockIdx.y
//      for the statistics and reward launches), and a workgroup forms its member's pointers from the bases -- scalar additions, uniform over the workgroup -- and runs the
//      single-network body on them with n = G.  A member's last workgroup therefore handles its tail as the single-network launch handles n % 32, and a call computes
//      the bits of K single-network calls on the slices (tests/test_gpu_population_kernels.py). ----
// the flat parameter block of include/usim.h (usim_ppo_params: the field order of usim_policy_net) as a PolicyNet
DI PolicyNet member_net(const float* t, int adim, const float4* packed) {
    PolicyNet P;
    P.pi_w1 = t; t += PL_H1 * PL_OBS; P.pi_b1 = t; t += PL_H1; P.pi_w2 = t; t += PL_H2 * PL_H1; P.pi_b2 = t; t += PL_H2;
    P.act_w = t; t += adim * PL_H2; P.act_b = t; t += adim;
    P.vf_w1 = t; t += PL_H1 * PL_OBS; P.vf_b1 = t; t += PL_H1; P.vf_w2 = t; t += PL_H2 * PL_H1; P.vf_b2 = t; t += PL_H2;
    P.val_w = t; t += PL_H2; P.val_b = t; t += 1; P.log_std = t;
    P.w2_packed = packed;
    return P;
}
// the statistics of member k out of K-major ones: [K][19] moments, [K] counts and return moments, returns [K G]; the four constants are shared
DI NormStats member_stats(NormStats S, int k, int G) {
    S.obs_mean += k * PL_OBS; S.obs_var += k * PL_OBS; S.obs_count += k;
    S.ret_mean += k; S.ret_var += k; S.ret_count += k;
    if (S.returns) S.returns += (size_t)k * G;
    return S;
}
template <class T> DI T* member_rows(T* p, int k, int G, int width) { return p ? p + (size_t)k * G * width : nullptr; }     // rows [k G, (k + 1) G) of a [K G][width] buffer (NULL stays NULL)

constexpr int PL_PACKED4 = 2 * 4 * 2 * (PL_H1 / 16) * 64;            // float4 words of one network pair's packed layer-2 weights (USIM_POLICY_PACKED / 4)
__global__ __launch_bounds__(256) void usim_policy_pack_multi_kernel(const float* __restrict__ theta, int stride, int adim, float4* __restrict__ packed) {
    const PolicyNet P = member_net(theta + (size_t)blockIdx.y * stride, adim, nullptr);
    pack_body(P.pi_w2, P.vf_w2, packed + (size_t)blockIdx.y * PL_PACKED4);
}
__global__ __launch_bounds__(PL_ST) void usim_policy_obs_stats_multi_kernel(const float* __restrict__ obs, int G, NormStats S, double* __restrict__ scratch) {
    __shared__ ObsStatsLds L;
    const int k = blockIdx.y;
    double* part = scratch + (size_t)k * USIM_POLICY_SCRATCH;
    obs_stats_body(L, member_rows(obs, k, G, PL_OBS), G, member_stats(S, k, G), part, reinterpret_cast<unsigned int*>(part + PL_SB * PL_OBS * 2));
}
__global__ __launch_bounds__(256, 2) void usim_policy_act_multi_kernel(const float* __restrict__ theta, int stride, const float4* __restrict__ packed, NormStats S,
                                                                    const float* __restrict__ obs, const uint8_t* __restrict__ prev_done, int G, int adim,
                                                                    const float* __restrict__ act_low, const float* __restrict__ act_high, uint32_t key0, uint32_t key1,
                                                                    uint32_t ctr0, const uint32_t* __restrict__ ctr_base, int env_offset, int deterministic,
                                                                    float* __restrict__ nobs_out, float* __restrict__ act_out, float* __restrict__ act_env,
                                                                    float* __restrict__ value_out, float* __restrict__ logp_out, float* __restrict__ start_out) {
    const int k = blockIdx.z;
    const PolicyNet P = member_net(theta + (size_t)k * stride, adim, packed + (size_t)k * PL_PACKED4);
    policy_act_body<false>(P, member_stats(S, k, G), member_rows(obs, k, G, PL_OBS), member_rows(prev_done, k, G, 1), G, adim, act_low, act_high, key0, key1, ctr0, ctr_base,
                           env_offset + k * G, deterministic, member_rows(nobs_out, k, G, PL_OBS), member_rows(act_out, k, G, adim), member_rows(act_env, k, G, adim),
                           member_rows(value_out, k, G, 1), member_rows(logp_out, k, G, 1), member_rows(start_out, k, G, 1), FusedArgs{});
}

// VecNormalize.step_wait after the env step: returns = gamma returns + reward; RunningMeanStd.update(returns); normalised, clipped reward; returns
// reset where an episode ended.  One workgroup, one pass over the batch (sum r, sum r^2, sum of the raw rewards reduced together).
struct RewardLds { double red[3][16]; double scale; };
DI void reward_body(RewardLds& L, const float* __restrict__ rew, const uint8_t* __restrict__ done, int n, const NormStats& S, int training,
                    int norm_reward, float* __restrict__ nrew_out, double* __restrict__ raw_sum) {
    double (&red)[3][16] = L.red; double& scale = L.scale;
    double raw = 0.0, s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double rw = (double)rew[i];
        raw += rw;
        if (training) { const double r = S.returns[i] * S.gamma + rw; s += r; q += r * r; S.returns[i] = done[i] ? 0.0 : r; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { raw += __shfl_xor(raw, o); s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = raw; red[1][threadIdx.x >> 6] = s; red[2][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { a += red[0][i]; b += red[1][i]; c += red[2][i]; }
        if (raw_sum) *raw_sum += a;
        if (training) *S.ret_count = merge_moments(*S.ret_mean, *S.ret_var, *S.ret_count, b, c, n);
        scale = 1.0 / sqrt(*S.ret_var + S.epsilon);
    }
    __syncthreads();
    const double sc = scale;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        double v = (double)rew[i];
        if (norm_reward) { v *= sc; v = v < -S.clip_reward ? -S.clip_reward : (v > S.clip_reward ? S.clip_reward : v); }
        nrew_out[i] = (float)v;
    }
}
__global__ __launch_bounds__(1024) void usim_policy_reward_kernel(const float* __restrict__ rew, const uint8_t* __restrict__ done, int n, NormStats S, int training,
                                                                  int norm_reward, float* __restrict__ nrew_out, double* __restrict__ raw_sum) {
    __shared__ RewardLds L;
    reward_body(L, rew, done, n, S, training, norm_reward, nrew_out, raw_sum);
}
// Both halves of VecNormalize.step_wait in ONE launch: workgroups 0 .. PL_SB - 1 update the observation statistics with the observation the step just
// produced (the policy kernel of the next step then only normalises: usim_policy_step training = 2), workgroup PL_SB does the reward side.  Two tiny,
// latency-bound kernels (11 + 7 us) become one.
__global__ __launch_bounds__(1024) void usim_policy_post_kernel(const float* __restrict__ rew, const uint8_t* __restrict__ done, int n, NormStats S, int training,
                                                                int norm_reward, float* __restrict__ nrew_out, double* __restrict__ raw_sum,
                                                                const float* __restrict__ next_obs, double* __restrict__ part, unsigned int* __restrict__ arrived) {
    __shared__ union { ObsStatsLds a; RewardLds b; } L;
    if (blockIdx.x < PL_SB) obs_stats_body(L.a, next_obs, n, S, part, arrived);
    else reward_body(L.b, rew, done, n, S, training, norm_reward, nrew_out, raw_sum);
}
// The population's reward launch, with the member on blockIdx.y.  with_obs: the grid of usim_policy_post_kernel per member (PL_SB statistics workgroups, then the
// reward workgroup); without: one reward workgroup per member, as usim_policy_reward_kernel.  raw_sum [K] (or NULL).
__global__ __launch_bounds__(1024) void usim_policy_post_multi_kernel(const float* __restrict__ rew, const uint8_t* __restrict__ done, int G, NormStats S, int training,
                                                                      int norm_reward, float* __restrict__ nrew_out, double* __restrict__ raw_sum,
                                                                      const float* __restrict__ next_obs, double* __restrict__ scratch, int with_obs) {
    __shared__ union { ObsStatsLds a; RewardLds b; } L;
    const int k = blockIdx.y;
    const NormStats M = member_stats(S, k, G);
    if (with_obs && blockIdx.x < PL_SB) {
        double* part = scratch + (size_t)k * USIM_POLICY_SCRATCH;
        obs_stats_body(L.a, member_rows(next_obs, k, G, PL_OBS), G, M, part, reinterpret_cast<unsigned int*>(part + PL_SB * PL_OBS * 2));
    } else
        reward_body(L.b, member_rows(rew, k, G, 1), member_rows(done, k, G, 1), G, M, training, norm_reward, member_rows(nrew_out, k, G, 1), raw_sum ? raw_sum + k : nullptr);
}

// RolloutBuffer.compute_returns_and_advantage: one thread per environment walks its column of the [T][n] buffers backwards
__global__ void usim_policy_gae_kernel(const float* __restrict__ rewards, const float* __restrict__ values, const float* __restrict__ starts,
                                       const float* __restrict__ last_values, const uint8_t* __restrict__ last_done, int T, int n, float gamma, float lam,
                                       float* __restrict__ adv, float* __restrict__ ret) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gae = 0.f, next_v = last_values[i], next_nt = 1.f - (last_done[i] ? 1.f : 0.f);
    for (int t = T - 1; t >= 0; --t) {
        const size_t ix = (size_t)t * n + i;
        const float v = values[ix];
        const float delta = rewards[ix] + gamma * next_v * next_nt - v;
        gae = delta + gamma * lam * next_nt * gae;
        adv[ix] = gae; ret[ix] = gae + v;
        next_v = v; next_nt = 1.f - starts[ix];
    }
}

// Time-limit bootstrap (SB3 OnPolicyAlgorithm.collect_rollouts: `if done and infos[idx].get("TimeLimit.truncated"): rewards[idx] += gamma * V(terminal_observation)`):
// environment i is truncated iff done[i] != 0 && ep_length[i] >= horizon (vec_env.py step_wait's rule; ep_length is stale where not done, hence both halves).
// One workgroup = BT_TM consecutive environments.  Truncations are rare per step, so the common workgroup sees none: it reads its 32 flag pairs, passes one barrier
// and returns -- no weight or statistics read is issued before that.  A workgroup that has some runs the value network for exactly those, one after the other,
// on plain float32 multiply-adds (~38 k per environment: no matrix cores, no packed weights): it lists them in environment order (slot j of the list), and every
// sum below runs over the inputs of ONE environment in an order that is fixed in the code -- not a function of j, of the other slots, of n or of the grid -- so an
// environment's result has the same bits wherever and with whomever it is computed.
//   normalise   float64 ((x - mean) * (1 / sqrt(var + eps))), clipped to +-clip_obs, rounded to float32: usim_policy_act_kernel's arithmetic; statistics read only
//   layer 1     thread f holds row f of vf_w1 [256][19]: fmaf chain k = 0 .. 18 from 0, + bias, tanh_
//   layer 2     the eight lanes of group g hold rows 4 g .. 4 g + 3 of vf_w2 [128][256] in registers (lane l the words k = 32 c + 4 l .. + 3 of chunk c = 0 .. 7,
//               loaded once per workgroup; an activation word read from LDS serves four rows): per row one fmaf chain over the lane's 32 words, k ascending,
//               then the xor-shuffle sums 1, 2, 4 (every lane arrives at the same bits), + bias, tanh_
//   head        eight lanes per slot as in the policy kernel: sixteen terms each, xor-shuffle sums 1, 2, 4, + bias
//   reward      rew[i] = fmaf(gamma, V, rew[i]); no other word of rew is touched, and rows of term_obs that are not truncated are never read
// count (may be null) += the workgroup's number of truncated environments: an integer atomic, exact in any order.
constexpr int BT_TM = 32;
__global__ __launch_bounds__(256) void usim_policy_bootstrap_kernel(PolicyNet P, NormStats S, const float* __restrict__ term_obs, const uint8_t* __restrict__ done,
                                                                    const int32_t* __restrict__ ep_length, int n, int horizon, float gamma, float* __restrict__ rew,
                                                                    int32_t* __restrict__ count) {
    __shared__ int list[BT_TM], m_s;
    __shared__ double mean[PL_OBS], inv[PL_OBS];
    __shared__ __attribute__((aligned(16))) float xs[BT_TM][PL_KPAD];
    __shared__ __attribute__((aligned(16))) float h1[BT_TM][PL_H1S];
    __shared__ __attribute__((aligned(16))) float h2[BT_TM][PL_H2S];
    const int tid = threadIdx.x, row0 = blockIdx.x * BT_TM;
    if (tid < 64) {                                                    // wave 0: the flags of this workgroup's environments, and the list of the truncated ones in order
        const int env = row0 + tid;
        const bool trunc = tid < BT_TM && env < n && done[env] != 0 && ep_length[env] >= horizon;
        const unsigned long long mask = __ballot(trunc);
        if (trunc) list[__popcll(mask & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) m_s = __popcll(mask);
    }
    __syncthreads();
    const int m = m_s;
    if (m == 0) return;                                                // the common case ends here
    // ---- every weight read is issued up front, in whole cache lines: the eight lanes of group g read 128 contiguous bytes of a row of vf_w2 per instruction (rows
    //      4 g .. 4 g + 3 stay in registers for all slots: 32 float4 per thread), vf_w1 goes through LDS (h1's space, free until layer 1 writes it) ----
    const int g = tid >> 3, l = tid & 7;
    float4 w2[4][PL_H1 / 32];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < PL_H1 / 32; ++c) w2[r][c] = *reinterpret_cast<const float4*>(P.vf_w2 + (size_t)(4 * g + r) * PL_H1 + 32 * c + 4 * l);
    float* w1s = &h1[0][0];
    static_assert(PL_H1 * PL_OBS <= BT_TM * PL_H1S, "vf_w1 fits the layer-1 output buffer");
#pragma unroll
    for (int i = 0; i < PL_OBS; ++i) w1s[tid + 256 * i] = P.vf_w1[tid + 256 * i];
    const float b1 = P.vf_b1[tid], b2 = P.vf_b2[4 * g + (l & 3)], vb = P.val_b[0];
    const int hs = tid >> 3, ho = tid & 7;                              // head: slot, lane of the slot
    float4 wh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wh[q] = *reinterpret_cast<const float4*>(&P.val_w[16 * ho + 4 * q]);
    if (tid < PL_OBS) { mean[tid] = S.obs_mean[tid]; inv[tid] = 1.0 / sqrt(S.obs_var[tid] + S.epsilon); }
    __syncthreads();
    float w1[PL_OBS];
#pragma unroll
    for (int k = 0; k < PL_OBS; ++k) w1[k] = w1s[tid * PL_OBS + k];    // (row stride 19 words: no bank is hit twice by 32 lanes)
    for (int e = tid; e < m * PL_KPAD; e += 256) {
        const int j = e / PL_KPAD, c = e - j * PL_KPAD;
        float v = 0.f;
        if (c < PL_OBS) {
            double x = ((double)term_obs[(size_t)(row0 + list[j]) * PL_OBS + c] - mean[c]) * inv[c];
            x = x < -S.clip_obs ? -S.clip_obs : (x > S.clip_obs ? S.clip_obs : x);
            v = (float)x;
        }
        xs[j][c] = v;
    }
    __syncthreads();                                                   // (every thread holds its row of vf_w1: h1 may be written)
    for (int j = 0; j < m; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < PL_OBS; ++k) acc = fmaf(w1[k], xs[j][k], acc);
        h1[j][tid] = tanh_(acc + b1);
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
        float4 h[PL_H1 / 32];
#pragma unroll
        for (int c = 0; c < PL_H1 / 32; ++c) h[c] = *reinterpret_cast<const float4*>(&h1[j][32 * c + 4 * l]);
        float s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < PL_H1 / 32; ++c) { a = fmaf(w2[r][c].x, h[c].x, a); a = fmaf(w2[r][c].y, h[c].y, a); a = fmaf(w2[r][c].z, h[c].z, a); a = fmaf(w2[r][c].w, h[c].w, a); }
            a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4);
            s[r] = a;
        }
        const float sl = (l & 2) ? ((l & 1) ? s[3] : s[2]) : ((l & 1) ? s[1] : s[0]);
        if (l < 4) h2[j][4 * g + l] = tanh_(sl + b2);
    }
    __syncthreads();
    float acc = 0.f;
    if (hs < m) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 h = *reinterpret_cast<const float4*>(&h2[hs][16 * ho + 4 * q]);
            acc = fmaf(h.x, wh[q].x, acc); acc = fmaf(h.y, wh[q].y, acc); acc = fmaf(h.z, wh[q].z, acc); acc = fmaf(h.w, wh[q].w, acc);
        }
    }
    acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4);
    if (hs < m && ho == 0) { const int env = row0 + list[hs]; rew[env] = fmaf(gamma, acc + vb, rew[env]); }
    if (tid == 0 && count) atomicAdd(count, m);
}

// the C ABI's structs as kernel arguments, and the arguments usim_policy_step and usim_policy_step_fused both require
static PolicyNet policy_net(const usim_policy_net& n) { return {n.pi_w1, n.pi_b1, n.pi_w2, n.pi_b2, n.act_w, n.act_b, n.vf_w1, n.vf_b1, n.vf_w2, n.vf_b2, n.val_w, n.val_b, n.log_std, reinterpret_cast<const float4*>(n.w2_packed)}; }
static NormStats norm_stats(const usim_norm_stats& s) { return {s.obs_mean, s.obs_var, s.obs_count, s.ret_mean, s.ret_var, s.ret_count, s.returns, s.clip_obs, s.clip_reward, s.gamma, s.epsilon}; }
static bool step_args_ok(const usim_policy_net* net, const usim_norm_stats* st, const float* obs_dev, int n, int act_dim, const float* lo, const float* hi, const usim_policy_out* out) {
    return net && st && obs_dev && out && out->act_env_dev && n > 0 && act_dim >= 1 && act_dim <= 7 && lo && hi && net->w2_packed;
}
// the policy launch of usim_policy_step (FUSED = false, F unused) and usim_policy_step_fused
template <bool FUSED>
static int launch_act(const usim_policy_net* net, const usim_norm_stats* st, const FusedArgs& F, const float* obs_dev, const uint8_t* prev_done_dev, int n, int act_dim,
                      const float* act_low_dev, const float* act_high_dev, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev, int env_offset,
                      int deterministic, const usim_policy_out* out, void* stream) {
    hipLaunchKernelGGL(usim_policy_act_kernel<FUSED>, dim3((n + PL_TM - 1) / PL_TM, 2), dim3(256), 0, (hipStream_t)stream, policy_net(*net), norm_stats(*st), obs_dev, prev_done_dev, n,
                       act_dim, act_low_dev, act_high_dev, (uint32_t)seed, (uint32_t)(seed >> 32), counter, counter_base_dev, env_offset, deterministic, out->nobs_dev, out->act_dev,
                       out->act_env_dev, out->value_dev, out->logp_dev, out->episode_start_dev, F);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

}  // namespace usim

extern "C" {

int usim_policy_pack(const usim_policy_net* net, float* packed_dev, void* stream) {
    if (!net || !net->pi_w2 || !net->vf_w2 || !packed_dev || (reinterpret_cast<uintptr_t>(packed_dev) & 15)) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_policy_pack_kernel, dim3(USIM_POLICY_PACKED / 4 / 256), dim3(256), 0, (hipStream_t)stream, net->pi_w2, net->vf_w2, reinterpret_cast<float4*>(packed_dev));
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

int usim_policy_step(const usim_policy_net* net, const usim_norm_stats* st, const float* obs_dev, const uint8_t* prev_done_dev, int n, int act_dim,
                     const float* act_low_dev, const float* act_high_dev, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev, int env_offset,
                     int training, int deterministic, const usim_policy_out* out, void* stream) {
    if (!step_args_ok(net, st, obs_dev, n, act_dim, act_low_dev, act_high_dev, out)) return USIM_ERR_INVALID;
    if (training == 1) {
        if (!st->scratch) return USIM_ERR_INVALID;
        // scratch: PL_SB x 19 x 2 partial sums, then the arrival counter (zero on entry, left zero)
        hipLaunchKernelGGL(usim_policy_obs_stats_kernel, dim3(PL_SB), dim3(PL_ST), 0, (hipStream_t)stream, obs_dev, n, norm_stats(*st), st->scratch,
                           reinterpret_cast<unsigned int*>(st->scratch + PL_SB * PL_OBS * 2));
    }
    return launch_act<false>(net, st, FusedArgs{}, obs_dev, prev_done_dev, n, act_dim, act_low_dev, act_high_dev, seed, counter, counter_base_dev, env_offset, deterministic, out, stream);
}

int usim_policy_step_fused(const usim_policy_net* net, const usim_norm_stats* st, const usim_policy_fused* f, const float* obs_dev, const uint8_t* prev_done_dev, int n,
                           int act_dim, const float* act_low_dev, const float* act_high_dev, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev,
                           int env_offset, int deterministic, const usim_policy_out* out, void* stream) {
    if (!f || !step_args_ok(net, st, obs_dev, n, act_dim, act_low_dev, act_high_dev, out)) return USIM_ERR_INVALID;
    if (!f->work_dev || (f->have_prev && (!f->rew_prev_dev || !f->done_prev_dev || !f->nrew_prev_dev))) return USIM_ERR_INVALID;
    if (n > USIM_POLICY_FUSED_MAX_ENVS) return USIM_ERR_UNSUPPORTED;          // every workgroup must be resident (see the kernel)
    {
        // The workgroups wait for one another inside an ordinary launch: that is only correct while the whole grid is resident at once.  Ask the
        // runtime what this device (in its current partition mode / CU mask) holds instead of trusting the constant above; cached per device.
        static std::atomic<int> capacity[64];                                 // (0: not asked yet; two threads asking at once store the same number)
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return USIM_ERR_HIP;
        int cap = capacity[dev].load(std::memory_order_relaxed);
        if (cap == 0) {
            int per_cu = 0, cus = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, usim_policy_act_kernel<true>, 256, 0) != hipSuccess ||
                hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return USIM_ERR_HIP;
            cap = per_cu * cus > 0 ? per_cu * cus : -1;
            capacity[dev].store(cap, std::memory_order_relaxed);
        }
        if (2 * ((n + PL_TM - 1) / PL_TM) > cap) return USIM_ERR_UNSUPPORTED;
    }
    const FusedArgs F{f->rew_prev_dev, f->done_prev_dev, f->nrew_prev_dev, f->raw_sum_dev, f->work_dev, f->update_obs, f->have_prev, f->norm_reward};
    return launch_act<true>(net, st, F, obs_dev, prev_done_dev, n, act_dim, act_low_dev, act_high_dev, seed, counter, counter_base_dev, env_offset, deterministic, out, stream);
}

int usim_policy_reward(const usim_norm_stats* st, const float* rew_dev, const uint8_t* done_dev, int n, int training, int norm_reward, float* nrew_dev,
                       double* raw_sum_dev, const float* next_obs_dev, void* stream) {
    if (!st || !rew_dev || !done_dev || !nrew_dev || n <= 0) return USIM_ERR_INVALID;
    const NormStats S = norm_stats(*st);
    if (next_obs_dev && training) {
        if (!st->scratch) return USIM_ERR_INVALID;
        hipLaunchKernelGGL(usim_policy_post_kernel, dim3(PL_SB + 1), dim3(1024), 0, (hipStream_t)stream, rew_dev, done_dev, n, S, training, norm_reward, nrew_dev, raw_sum_dev,
                           next_obs_dev, st->scratch, reinterpret_cast<unsigned int*>(st->scratch + PL_SB * PL_OBS * 2));
    } else
    hipLaunchKernelGGL(usim_policy_reward_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rew_dev, done_dev, n, S, training, norm_reward, nrew_dev, raw_sum_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

// ---- populations (the contracts are include/usim.h's): every argument is checked before the first launch ----
static bool members_ok(int members, int envs_per_member) {            // K, G >= 1, K G within int, K within a grid axis
    return members > 0 && envs_per_member > 0 && (int64_t)members * envs_per_member <= INT32_MAX && members <= USIM_POLICY_MAX_MEMBERS;
}
static bool theta_ok(const float* theta_dev, int stride, int act_dim) {
    return theta_dev && act_dim >= 1 && act_dim <= 8 && stride >= usim_ppo_params(act_dim) && stride % 4 == 0;
}

int usim_policy_pack_multi(const float* theta_dev, int stride, int members, int act_dim, float* packed_dev, void* stream) {
    if (!theta_ok(theta_dev, stride, act_dim) || !members_ok(members, 1) || !packed_dev || (reinterpret_cast<uintptr_t>(packed_dev) & 15)) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_policy_pack_multi_kernel, dim3(USIM_POLICY_PACKED / 4 / 256, members), dim3(256), 0, (hipStream_t)stream, theta_dev, stride, act_dim,
                       reinterpret_cast<float4*>(packed_dev));
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

int usim_policy_step_multi(const float* theta_dev, int stride, const float* packed_dev, const usim_norm_stats* st, const float* obs_dev, const uint8_t* prev_done_dev,
                           int members, int envs_per_member, int act_dim, const float* act_low_dev, const float* act_high_dev, uint64_t seed, uint32_t counter,
                           const uint32_t* counter_base_dev, int env_offset, int training, int deterministic, const usim_policy_out* out, void* stream) {
    if (!theta_ok(theta_dev, stride, act_dim) || !members_ok(members, envs_per_member) || !packed_dev || (reinterpret_cast<uintptr_t>(packed_dev) & 15)) return USIM_ERR_INVALID;
    if (!st || !st->obs_mean || !st->obs_var || !obs_dev || !act_low_dev || !act_high_dev || !out || !out->act_env_dev) return USIM_ERR_INVALID;
    const NormStats S = norm_stats(*st);
    const int G = envs_per_member;
    if (training == 1) {
        if (!st->scratch || !st->obs_count) return USIM_ERR_INVALID;
        hipLaunchKernelGGL(usim_policy_obs_stats_multi_kernel, dim3(PL_SB, members), dim3(PL_ST), 0, (hipStream_t)stream, obs_dev, G, S, st->scratch);
    }
    hipLaunchKernelGGL(usim_policy_act_multi_kernel, dim3((G + PL_TM - 1) / PL_TM, 2, members), dim3(256), 0, (hipStream_t)stream, theta_dev, stride,
                       reinterpret_cast<const float4*>(packed_dev), S, obs_dev, prev_done_dev, G, act_dim, act_low_dev, act_high_dev, (uint32_t)seed, (uint32_t)(seed >> 32), counter,
                       counter_base_dev, env_offset, deterministic, out->nobs_dev, out->act_dev, out->act_env_dev, out->value_dev, out->logp_dev, out->episode_start_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

int usim_policy_reward_multi(const usim_norm_stats* st, const float* rew_dev, const uint8_t* done_dev, int members, int envs_per_member, int training, int norm_reward,
                             float* nrew_dev, double* raw_sum_dev, const float* next_obs_dev, void* stream) {
    if (!st || !rew_dev || !done_dev || !nrew_dev || !members_ok(members, envs_per_member)) return USIM_ERR_INVALID;
    if (!st->ret_var || (training && (!st->ret_mean || !st->ret_count || !st->returns))) return USIM_ERR_INVALID;
    const int with_obs = next_obs_dev && training;
    if (with_obs && (!st->scratch || !st->obs_mean || !st->obs_var || !st->obs_count)) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_policy_post_multi_kernel, dim3(with_obs ? PL_SB + 1 : 1, members), dim3(1024), 0, (hipStream_t)stream, rew_dev, done_dev, envs_per_member,
                       norm_stats(*st), training, norm_reward, nrew_dev, raw_sum_dev, next_obs_dev, st->scratch, with_obs);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

int usim_policy_bootstrap(const usim_policy_net* net, const usim_norm_stats* st, const float* term_obs_dev, const uint8_t* done_dev, const int32_t* ep_length_dev,
                          int n, int horizon, float gamma, float* rew_dev, int32_t* count_dev, void* stream) {
    if (!net || !st || !term_obs_dev || !done_dev || !ep_length_dev || !rew_dev) return USIM_ERR_INVALID;
    if (!net->vf_w1 || !net->vf_b1 || !net->vf_w2 || !net->vf_b2 || !net->val_w || !net->val_b || !st->obs_mean || !st->obs_var) return USIM_ERR_INVALID;
    if (n <= 0 || horizon <= 0 || !(gamma >= 0.f && gamma <= 1.f)) return USIM_ERR_INVALID;           // (a NaN fails both comparisons)
    hipLaunchKernelGGL(usim_policy_bootstrap_kernel, dim3((n + BT_TM - 1) / BT_TM), dim3(256), 0, (hipStream_t)stream, policy_net(*net), norm_stats(*st), term_obs_dev,
                       done_dev, ep_length_dev, n, horizon, gamma, rew_dev, count_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

int usim_policy_gae(const float* rewards_dev, const float* values_dev, const float* episode_starts_dev, const float* last_values_dev, const uint8_t* last_done_dev,
                    int T, int n, float gamma, float gae_lambda, float* advantages_dev, float* returns_dev, void* stream) {
    if (!rewards_dev || !values_dev || !episode_starts_dev || !last_values_dev || !last_done_dev || !advantages_dev || !returns_dev || T <= 0 || n <= 0) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_policy_gae_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards_dev, values_dev, episode_starts_dev, last_values_dev,
                       last_done_dev, T, n, gamma, gae_lambda, advantages_dev, returns_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

}  // extern "C"
