// usim_score.hip -- usim_score_block: the discounted return of every environment's FIRST episode inside a rollout block [T][n] (rew, done), and that episode's
// length, in ONE launch -- the scoring pass of a shooting planner after usim_rollout_actions, instead of 2 T small torch kernels
// (ret += rew * alive; alive &= ~done).  A translation unit of its own: it shares nothing with the step kernels but the public header.
//
// For environment i:  L = 1 + the first k with done[k][i] != 0 (any non-zero byte), or T if there is none;
//                     return[i] = sum over k < L of gamma^k rew[k][i];  length[i] = L.
// Past its first done an environment of an auto-reset rollout plays an episode of its own: those words are not read into the sum (a NaN there does not reach it).
//
// The arithmetic is fixed, so the result is a function of the inputs alone: float32, in step order,  ret = fmaf(disc, r, ret); disc *= gamma;  from ret = 0, disc = 1.
// One thread per environment, 256 per workgroup, a loop over the steps: consecutive lanes read consecutive environments, so the loads of a step coalesce (256 B of
// rewards, 64 B of flags per wave).  A lane stops accumulating at its first done; a wave leaves the loop when all its lanes have.  No LDS, no atomics, nothing ordered
// by arrival.  4096 environments x 256 steps move 5 MB: not a hot spot -- it exists so that scoring is one node of the stream or graph.
//
// usim_score_block_tail: the same loop, then a bootstrap for the environments that met no done inside the block -- a critic's value of the state behind the last
// step, so that a candidate's return does not stop at step T as if nothing came after (planner.py MPPIPlanner(critic=...)):
//                     return[i] = fmaf(disc_T, s * tail[i], return[i])      disc_T: the loop's own running discount after its T steps, ((1 gamma) gamma) ... in float32
//                     s = (float)sqrt(*ret_var + epsilon), the square root in float64: a critic trained under VecNormalize's norm_reward speaks in normalised-return
//                     units, s takes it back to raw reward; s = 1 without ret_var
// The tail word of an environment that ended inside the block is not loaded.  A kernel of its own, the loop restated: usim_score_block_kernel stays as it is.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/usim.h"

namespace usim {

constexpr int SC_WG = 256;                                       // threads = environments per workgroup

__global__ __launch_bounds__(SC_WG) void usim_score_block_kernel(const float* __restrict__ rew, const uint8_t* __restrict__ done, int nsteps, int n, float gamma,
                                                                 float* __restrict__ ret_out, int32_t* __restrict__ len_out) {
    const size_t env = (size_t)blockIdx.x * SC_WG + threadIdx.x;
    bool alive = env < (size_t)n;                                // a lane beyond the last environment reads nothing
    const bool mine = alive;
    float ret = 0.f, disc = 1.f;
    int len = nsteps;
    for (int k = 0; k < nsteps; ++k) {
        if (!__any(alive)) break;                                // wave-uniform: every lane of the wave has met its first done
        if (alive) {
            const size_t w = (size_t)k * (size_t)n + env;
            ret = fmaf(disc, rew[w], ret);
            disc *= gamma;
            if (done[w] != 0) { len = k + 1; alive = false; }
        }
    }
    if (mine) {
        ret_out[env] = ret;
        if (len_out) len_out[env] = len;
    }
}

// the loop of usim_score_block_kernel and, for a lane that is still alive behind it, the bootstrap (file header)
__global__ __launch_bounds__(SC_WG) void usim_score_block_tail_kernel(const float* __restrict__ rew, const uint8_t* __restrict__ done, int nsteps, int n, float gamma,
                                                                      const float* __restrict__ tail, const double* __restrict__ ret_var, double epsilon,
                                                                      float* __restrict__ ret_out, int32_t* __restrict__ len_out) {
    const size_t env = (size_t)blockIdx.x * SC_WG + threadIdx.x;
    bool alive = env < (size_t)n;
    const bool mine = alive;
    float ret = 0.f, disc = 1.f;
    int len = nsteps;
    for (int k = 0; k < nsteps; ++k) {
        if (!__any(alive)) break;
        if (alive) {
            const size_t w = (size_t)k * (size_t)n + env;
            ret = fmaf(disc, rew[w], ret);
            disc *= gamma;
            if (done[w] != 0) { len = k + 1; alive = false; }
        }
    }
    if (tail && alive) {                                         // no done inside the block: disc is the discount after all nsteps steps
        const float s = ret_var ? (float)sqrt(*ret_var + epsilon) : 1.f;
        ret = fmaf(disc, s * tail[env], ret);
    }
    if (mine) {
        ret_out[env] = ret;
        if (len_out) len_out[env] = len;
    }
}

}  // namespace usim

extern "C" int usim_score_block(const float* rew_block_dev, const uint8_t* done_block_dev, int nsteps, int n, float gamma, float* return_dev, int32_t* length_dev,
                                void* stream) {
    using namespace usim;
    if (!rew_block_dev || !done_block_dev || !return_dev || n <= 0 || nsteps <= 0) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_score_block_kernel, dim3((unsigned)(((size_t)n + SC_WG - 1) / SC_WG)), dim3(SC_WG), 0, (hipStream_t)stream, rew_block_dev, done_block_dev,
                       nsteps, n, gamma, return_dev, length_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_score_block_tail(const float* rew_block_dev, const uint8_t* done_block_dev, int nsteps, int n, float gamma, const float* tail_dev,
                                     const double* ret_var_dev, double epsilon, float* return_dev, int32_t* length_dev, void* stream) {
    using namespace usim;
    if (!rew_block_dev || !done_block_dev || !return_dev || n <= 0 || nsteps <= 0) return USIM_ERR_INVALID;
    if (!isfinite(gamma) || !isfinite(epsilon) || epsilon < 0.0) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_score_block_tail_kernel, dim3((unsigned)(((size_t)n + SC_WG - 1) / SC_WG)), dim3(SC_WG), 0, (hipStream_t)stream, rew_block_dev,
                       done_block_dev, nsteps, n, gamma, tail_dev, ret_var_dev, epsilon, return_dev, length_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}
