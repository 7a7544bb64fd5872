// usim_plan.hip -- usim_plan_sample / usim_plan_update: the two planner-side launches of a batched MPPI shooting planner (planner.py
// MPPIPlanner) -- the candidate sampler before usim_rollout_actions and the exponentially weighted update after usim_score_block, in place of a dozen small tensor
// kernels (randn, cumulative smoothing, clamp, softmax, einsum, roll, index_select) between 18 us simulator steps.  A translation unit of its own: it takes no
// usim_handle and shares nothing with the step kernels but the public header and usim_devmath.h (DI, philox, u4, PI_F).
//
// Layout: G controlled environments ("groups"), K candidates each, n = G K simulated environments; environments [g K, (g + 1) K) are the candidates of group g and
// candidate 0 of every group is the unperturbed nominal.  mean [G][H][A], cand [H][n][A] (what usim_rollout_actions consumes), ret [n].
//
// usim_plan_sample: one thread per (candidate, component) walks the H steps serially; for a fixed step consecutive threads write consecutive words of cand, so a
// wave's stores coalesce.  The noise of (candidate c = g K + k, step t, component a) is a function of (seed, counter, c, t, a) alone: one Philox4x32-10 block per
// pair of components, counter words (c, counter + *counter_base, 4 t + (a >> 1), PLAN_TAG), Box-Muller exactly as usim_policy_step (the same u1 / u2 construction,
// hardware log / sine / cosine), smoothed over the horizon by  e[0] = xi[0],  e[t] = fmaf(s, e[t - 1], sqrt(1 - s^2) xi[t]).
//
// usim_plan_update: one 256-thread workgroup per (group, step).  Every workgroup recomputes the group's weights from its K returns -- cheap, and it keeps the launch
// free of any exchange between workgroups -- and then reduces its contiguous K A-word slab cand[t][g K .. g K + K): a group of thousands of candidates is read by H
// workgroups, not by one CU.  THE REDUCTION ORDER IS FIXED, so the result is a function of the inputs alone -- no floating-point atomics, nothing ordered by arrival:
//   1. thread j takes candidates j, j + 256, j + 512, ... in ascending order (best: strict >, so the lowest index wins within a thread; sums: s += term, acc =
//      fmaf(w, cand, acc), from 0)
//   2. inside a wave the 64 partial results meet in a butterfly over lane distances 32, 16, 8, 4, 2, 1 (x = x + shfl_xor(x, d): both lanes of a pair add the same two
//      numbers, so all lanes end with the same bits; best: the pair (value, index) under "larger value, then lower index", a total order)
//   3. the four waves' results meet through LDS as ((w0 + w1) + w2) + w3
// The same three stages serve the argmax, the normaliser sum_k exp((ret_k - ret_best) / temperature) and the A weighted sums of the slab.
//
// The guided planner adds three launches (include/usim.h states their arithmetic): usim_plan_sample_elem, the sampler with one standard deviation per element of the
// nominal (the same kernel body, a template parameter); usim_plan_refit, a cross-entropy refit of the nominal and those deviations from a group's elite candidates,
// between the rounds of one control step; usim_plan_tail, the last step of the shifted nominal from the actor's actions, after usim_plan_update.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/usim.h"
#include "usim_devmath.h"

namespace usim {

constexpr int PN_WG = 256;                                       // threads per workgroup of both kernels
constexpr int PN_WAVES = PN_WG / 64;
constexpr int PN_MAXA = 8;                                       // act_dim <= 8: four Philox blocks per (candidate, step), eight accumulators per thread
constexpr uint32_t PLAN_TAG = 0x504c414eu;                       // fourth counter word of the planner's noise ("PLAN"; the policy's is "POLY")

// ELEM: sigma is [G][H][A], one standard deviation per element of the nominal (usim_plan_sample_elem), not [A]; nothing else differs
template <bool ELEM>
__global__ __launch_bounds__(PN_WG) void usim_plan_sample_kernel(float* __restrict__ mean, const float* __restrict__ sigma, const float* __restrict__ act_low,
                                                                 const float* __restrict__ act_high, const uint8_t* __restrict__ restart, int per_group, int horizon,
                                                                 int adim, size_t words, float smooth, float fresh, uint32_t key0, uint32_t key1, uint32_t ctr0,
                                                                 const uint32_t* __restrict__ ctr_base, float* __restrict__ cand) {
    const size_t i = (size_t)blockIdx.x * PN_WG + threadIdx.x;   // word (candidate, component) of one step's slice
    if (i >= words) return;
    const uint32_t c = (uint32_t)(i / (size_t)adim), a = (uint32_t)(i - (size_t)c * adim);
    const uint32_t g = c / (uint32_t)per_group, k = c - g * (uint32_t)per_group;
    const uint32_t ctr = ctr0 + (ctr_base ? *ctr_base : 0u);      // call counter: host part + a device word (a recorded graph advances the latter)
    const bool fresh_nominal = restart && restart[g] != 0;       // the group's environment has just started an episode: nominal 0, also written back (by candidate 0)
    float* mrow = mean + (size_t)g * horizon * adim + a;
    const float* srow = ELEM ? sigma + (size_t)g * horizon * adim + a : sigma + a;
    const float lo = act_low[a], hi = act_high[a];
    float sg = ELEM ? 0.f : srow[0];
    float e = 0.f;
    for (int t = 0; t < horizon; ++t) {
        float m = 0.f;
        if (fresh_nominal) {
            if (k == 0) mrow[(size_t)t * adim] = 0.f;            // (no thread reads the nominal of a restarted group)
        } else {
            m = mrow[(size_t)t * adim];
            if (!isfinite(m)) m = 0.f;                           // a non-finite word counts as 0, as an action does in usim_step
        }
        if (k != 0) {
            // N(0, 1) for (candidate, step, component): Box-Muller on one Philox block per pair of components (usim_policy_step's recipe)
            const u4 rr = philox(c, ctr, 4u * (uint32_t)t + (a >> 1), PLAN_TAG, key0, key1);
            const float u1 = ((float)(rr.a >> 8) + 1.0f) * (1.0f / 16777216.0f), u2 = (float)(rr.b >> 8) * (1.0f / 16777216.0f);
            const float rad = sqrtf(-2.f * __logf(u1)), ang = 2.f * PI_F * u2;
            const float xi = (a & 1) ? rad * __sinf(ang) : rad * __cosf(ang);
            e = t == 0 ? xi : fmaf(smooth, e, fresh * xi);
        }
        if (ELEM) sg = srow[(size_t)t * adim];
        cand[(size_t)t * words + i] = fminf(fmaxf(fmaf(sg, e, m), lo), hi);
    }
}

// ---- the three-stage reductions of usim_plan_update (file header) ----
DI bool better(float v, int k, float bv, int bk) { return v > bv || (v == bv && k < bk); }

DI float wg_sum(float x, float* lds) {                           // lds: PN_WAVES words of this sum's own
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// exp((ret_k - ret_best) / temperature) of a candidate, 0 for a non-finite return; a group without any finite return puts everything on candidate 0
DI float plan_weight(float v, int k, float bv, bool none, float temperature) {
    if (none) return k == 0 ? 1.f : 0.f;
    return isfinite(v) ? expf((v - bv) / temperature) : 0.f;
}

DI void plan_store(float v, int g, int t, int a, int horizon, int adim, float* __restrict__ plan, float* __restrict__ next_mean, float* __restrict__ act) {
    const size_t w = ((size_t)g * horizon + t) * adim + a;
    if (plan) plan[w] = v;
    if (next_mean) {                                             // the receding horizon: step t becomes step t - 1, the last action is kept
        if (t > 0) next_mean[w - adim] = v;
        if (t == horizon - 1) next_mean[w] = v;
    }
    if (t == 0) act[(size_t)g * adim + a] = v;
}

__global__ __launch_bounds__(PN_WG) void usim_plan_update_kernel(const float* __restrict__ cand, const float* __restrict__ ret, const float* __restrict__ act_low,
                                                                 const float* __restrict__ act_high, int per_group, int horizon, int adim, size_t n, float temperature,
                                                                 float* __restrict__ plan, float* __restrict__ next_mean, float* __restrict__ act,
                                                                 int32_t* __restrict__ best_out, float* __restrict__ weight_out) {
    __shared__ float best_v[PN_WAVES];
    __shared__ int best_k[PN_WAVES];
    __shared__ float norm[PN_WAVES];
    __shared__ float slab_sum[PN_MAXA][PN_WAVES];
    const int tid = threadIdx.x, K = per_group;
    const int g = (int)(blockIdx.x / (unsigned)horizon), t = (int)(blockIdx.x - (unsigned)g * (unsigned)horizon);
    const size_t first = (size_t)g * K;                          // the group's candidate 0
    const float* __restrict__ r = ret + first;
    const bool lead = t == 0;                                    // the workgroup of step 0 also writes the group's best and weights

    // ---- the candidate with the largest finite return, ties to the lowest index; (-inf, INT_MAX) stands for "none yet" and loses against every finite return ----
    float bv = -INFINITY;
    int bk = INT_MAX;
    for (int k = tid; k < K; k += PN_WG) {
        const float v = r[k];
        if (isfinite(v) && v > bv) { bv = v; bk = k; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(bv, d);
        const int ok = __shfl_xor(bk, d);
        if (better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    }
    if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_k[tid >> 6] = bk; }
    __syncthreads();
    bv = best_v[0]; bk = best_k[0];
#pragma unroll
    for (int w = 1; w < PN_WAVES; ++w)
        if (better(best_v[w], best_k[w], bv, bk)) { bv = best_v[w]; bk = best_k[w]; }
    const bool none = bk == INT_MAX;
    const int best = none ? 0 : bk;
    if (lead && tid == 0 && best_out) best_out[g] = best;
    const float* __restrict__ slab = cand + ((size_t)t * n + first) * adim;       // cand[t][g K .. g K + K): K A contiguous words

    if (temperature == 0.f) {
        // ---- a selection, not a product: the chosen candidate's words as they are ----
        if (tid < adim) plan_store(slab[(size_t)best * adim + tid], g, t, tid, horizon, adim, plan, next_mean, act);
        if (lead && weight_out)
            for (int k = tid; k < K; k += PN_WG) weight_out[first + k] = k == best ? 1.f : 0.f;
        return;
    }

    // ---- the normaliser ----
    float s = 0.f;
    for (int k = tid; k < K; k += PN_WG) s += plan_weight(r[k], k, bv, none, temperature);
    const float total = wg_sum(s, norm);                         // >= 1: the best candidate's term is exp(0)

    // ---- the weighted sums of the slab ----
    float acc[PN_MAXA];
#pragma unroll
    for (int a = 0; a < PN_MAXA; ++a) acc[a] = 0.f;
    for (int k = tid; k < K; k += PN_WG) {
        const float w = plan_weight(r[k], k, bv, none, temperature) / total;
        if (lead && weight_out) weight_out[first + k] = w;
        const float* __restrict__ row = slab + (size_t)k * adim;
#pragma unroll
        for (int a = 0; a < PN_MAXA; ++a)
            if (a < adim) acc[a] = fmaf(w, row[a], acc[a]);
    }
    float mine = 0.f;                                            // thread a < A ends with component a
#pragma unroll
    for (int a = 0; a < PN_MAXA; ++a) {
        const float v = wg_sum(acc[a], slab_sum[a]);
        if (a == tid) mine = v;
    }
    if (tid < adim) plan_store(fminf(fmaxf(mine, act_low[tid]), act_high[tid]), g, t, tid, horizon, adim, plan, next_mean, act);
}

// ---- usim_plan_refit: one cross-entropy refit of (mean, sigma_elem) per group; one workgroup per group ranks its K returns ONCE, then reduces the H A words ----
// key[k] is the return, -inf for a non-finite one (it then loses against every finite return and is never elite itself).  Rank of a finite candidate = how many
// candidates come before it under "larger return, then lower index" (`better`, a total order): every thread takes candidates tid, tid + 256, ... and walks all K keys,
// which every lane reads at the same LDS address (a broadcast) -- K^2 / 256 comparisons per thread, 65536 at the largest K.  Elite <=> rank < elites, so exactly
// min(elites, finite returns) candidates are.  The place of an elite in the list is the number of elites below its index: the list ascends in candidate index, whatever
// order the threads run in.  The count meets in an LDS INTEGER atomic (an integer sum does not depend on the order of arrival).
// Then thread j takes the words w = j, j + 256, ... of the group's [H][A] block (w = t A + a) and walks the list in ascending order, all in float32:
//   s = s + x from 0;  m = s / E;  d = x - m, q = fmaf(d, d, q) from 0;  sd = sqrtf(q / E)
//   mean = clip(fmaf(momentum, mean_old, c m), low, high);  sigma = fmaxf(fmaf(momentum, sigma_old, c sd), sigma_min),  c = (float)(1 - (double)momentum) from the host
// Every word is read and written by one thread, so the update is in place.  LDS: 4 K bytes of keys, 4 K of list, K of flags = 36 KB at K = 4096.
constexpr int PN_REFIT_MAXK = USIM_PLAN_REFIT_MAX_K;

__global__ __launch_bounds__(PN_WG) void usim_plan_refit_kernel(const float* __restrict__ cand, const float* __restrict__ ret, const float* __restrict__ act_low,
                                                                const float* __restrict__ act_high, int per_group, int horizon, int adim, size_t n, int elites,
                                                                float momentum, float fresh, float sigma_min, float* __restrict__ mean, float* __restrict__ sigma,
                                                                int32_t* __restrict__ elite_out) {
    __shared__ float key[PN_REFIT_MAXK];
    __shared__ int list[PN_REFIT_MAXK];
    __shared__ uint8_t flag[PN_REFIT_MAXK];
    __shared__ int count;
    const int tid = threadIdx.x, K = per_group, g = (int)blockIdx.x;
    const size_t first = (size_t)g * K;
    if (tid == 0) count = 0;
    for (int k = tid; k < K; k += PN_WG) {
        const float v = ret[first + k];
        key[k] = isfinite(v) ? v : -INFINITY;
    }
    __syncthreads();
    int mine = 0;
    for (int k = tid; k < K; k += PN_WG) {
        const float v = key[k];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += better(key[j], j, v, k) ? 1 : 0;
        const bool elite = v != -INFINITY && rank < elites;
        flag[k] = elite ? 1 : 0;
        mine += elite ? 1 : 0;
    }
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    for (int k = tid; k < K; k += PN_WG) {
        if (!flag[k]) continue;
        int place = 0;
        for (int j = 0; j < k; ++j) place += flag[j];
        list[place] = k;                                         // place < count <= min(elites, K)
    }
    __syncthreads();
    const int E = count;
    if (elite_out)
        for (int p = tid; p < elites; p += PN_WG) elite_out[(size_t)g * elites + p] = p < E ? list[p] : -1;
    if (E == 0) return;                                          // no finite return: mean and sigma stay as they are

    const int words = horizon * adim;
    const float fe = (float)E;
    for (int w = tid; w < words; w += PN_WG) {
        const int t = w / adim, a = w - t * adim;
        const float* __restrict__ col = cand + ((size_t)t * n + first) * adim + a;      // cand[t][g K + k][a] = col[k A]
        float s = 0.f;
        for (int p = 0; p < E; ++p) s += col[(size_t)list[p] * adim];
        const float m = s / fe;
        float q = 0.f;
        for (int p = 0; p < E; ++p) {
            const float d = col[(size_t)list[p] * adim] - m;
            q = fmaf(d, d, q);
        }
        const float sd = sqrtf(q / fe);
        const size_t word = (size_t)g * words + w;
        float mo = mean[word];
        if (!isfinite(mo)) mo = 0.f;                             // as the sampler reads the nominal
        mean[word] = fminf(fmaxf(fmaf(momentum, mo, fresh * m), act_low[a]), act_high[a]);
        sigma[word] = fmaxf(fmaf(momentum, sigma[word], fresh * sd), sigma_min);
    }
}

// ---- usim_plan_tail: the last step of the shifted nominal from the actor's action at each candidate's final observation; one workgroup per group ----
// x_k = pol_act[g K + k] where the candidate played all H steps without a done (length == H and done_last == 0), else its own last action cand[H - 1][g K + k].  The
// weights are those usim_plan_update wrote, and the sum runs in that kernel's three stages (file header).  A candidate of weight 0 is skipped: fmaf(0, x, acc) = acc
// for every finite x, and a non-finite action of a candidate that carries no weight must not reach the nominal.
__global__ __launch_bounds__(PN_WG) void usim_plan_tail_kernel(const float* __restrict__ cand, const float* __restrict__ weight, const int32_t* __restrict__ best,
                                                               const int32_t* __restrict__ length, const uint8_t* __restrict__ done_last,
                                                               const float* __restrict__ pol_act, const float* __restrict__ act_low, const float* __restrict__ act_high,
                                                               int per_group, int horizon, int adim, size_t n, float temperature, float* __restrict__ next_mean) {
    __shared__ float slab_sum[PN_MAXA][PN_WAVES];
    const int tid = threadIdx.x, K = per_group, g = (int)blockIdx.x;
    const size_t first = (size_t)g * K;
    const float* __restrict__ last = cand + ((size_t)(horizon - 1) * n + first) * adim;  // cand[H - 1][g K .. g K + K)
    const float* __restrict__ pol = pol_act + first * adim;
    float* __restrict__ out = next_mean + ((size_t)g * horizon + (horizon - 1)) * adim;

    if (temperature == 0.f) {                                    // a selection: the best candidate's x as it is
        const int k = best[g];
        if (tid < adim && k >= 0 && k < K) {                     // (an index from device memory: outside the group nothing is written)
            const bool whole = length[first + k] == horizon && done_last[first + k] == 0;
            out[tid] = (whole ? pol : last)[(size_t)k * adim + tid];
        }
        return;
    }

    float acc[PN_MAXA];
#pragma unroll
    for (int a = 0; a < PN_MAXA; ++a) acc[a] = 0.f;
    for (int k = tid; k < K; k += PN_WG) {
        const float w = weight[first + k];
        if (w == 0.f) continue;
        const bool whole = length[first + k] == horizon && done_last[first + k] == 0;
        const float* __restrict__ row = (whole ? pol : last) + (size_t)k * adim;
#pragma unroll
        for (int a = 0; a < PN_MAXA; ++a)
            if (a < adim) acc[a] = fmaf(w, row[a], acc[a]);
    }
    float mine = 0.f;
#pragma unroll
    for (int a = 0; a < PN_MAXA; ++a) {
        const float v = wg_sum(acc[a], slab_sum[a]);
        if (a == tid) mine = v;
    }
    if (tid < adim) out[tid] = fminf(fmaxf(mine, act_low[tid]), act_high[tid]);
}

}  // namespace usim

static bool plan_shape_ok(int groups, int per_group, int horizon, int act_dim) {
    return groups > 0 && per_group > 0 && horizon > 0 && act_dim >= 1 && act_dim <= usim::PN_MAXA && (int64_t)groups * per_group <= INT_MAX &&
           (int64_t)groups * horizon <= INT_MAX;                 // (n is an int everywhere in the library; one workgroup of the update per (group, step))
}

extern "C" int usim_plan_sample(float* mean_dev, const float* sigma_dev, const float* act_low_dev, const float* act_high_dev, const uint8_t* restart_dev, int groups,
                                int per_group, int horizon, int act_dim, float smoothing, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev,
                                float* cand_dev, void* stream) {
    using namespace usim;
    if (!mean_dev || !sigma_dev || !act_low_dev || !act_high_dev || !cand_dev || !plan_shape_ok(groups, per_group, horizon, act_dim)) return USIM_ERR_INVALID;
    if (!(smoothing >= 0.f && smoothing < 1.f)) return USIM_ERR_INVALID;                    // (a NaN fails both comparisons)
    const float fresh = (float)sqrt(1.0 - (double)smoothing * (double)smoothing);           // the weight of the new draw, rounded once
    const size_t words = (size_t)groups * per_group * act_dim;
    hipLaunchKernelGGL(usim_plan_sample_kernel<false>, dim3((unsigned)((words + PN_WG - 1) / PN_WG)), dim3(PN_WG), 0, (hipStream_t)stream, mean_dev, sigma_dev, act_low_dev,
                       act_high_dev, restart_dev, per_group, horizon, act_dim, words, smoothing, fresh, (uint32_t)seed, (uint32_t)(seed >> 32), counter,
                       counter_base_dev, cand_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_plan_update(const float* cand_dev, const float* ret_dev, const float* act_low_dev, const float* act_high_dev, int groups, int per_group, int horizon,
                                int act_dim, float temperature, float* plan_dev, float* next_mean_dev, float* act_dev, int32_t* best_dev, float* weight_dev,
                                void* stream) {
    using namespace usim;
    if (!cand_dev || !ret_dev || !act_low_dev || !act_high_dev || !act_dev || !plan_shape_ok(groups, per_group, horizon, act_dim)) return USIM_ERR_INVALID;
    if (!(temperature >= 0.f) || !isfinite(temperature)) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_plan_update_kernel, dim3((unsigned)groups * (unsigned)horizon), dim3(PN_WG), 0, (hipStream_t)stream, cand_dev, ret_dev, act_low_dev,
                       act_high_dev, per_group, horizon, act_dim, (size_t)groups * per_group, temperature, plan_dev, next_mean_dev, act_dev, best_dev, weight_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_plan_sample_elem(float* mean_dev, const float* sigma_elem_dev, const float* act_low_dev, const float* act_high_dev, const uint8_t* restart_dev,
                                     int groups, int per_group, int horizon, int act_dim, float smoothing, uint64_t seed, uint32_t counter,
                                     const uint32_t* counter_base_dev, float* cand_dev, void* stream) {
    using namespace usim;
    if (!mean_dev || !sigma_elem_dev || !act_low_dev || !act_high_dev || !cand_dev || !plan_shape_ok(groups, per_group, horizon, act_dim)) return USIM_ERR_INVALID;
    if (!(smoothing >= 0.f && smoothing < 1.f)) return USIM_ERR_INVALID;
    const float fresh = (float)sqrt(1.0 - (double)smoothing * (double)smoothing);
    const size_t words = (size_t)groups * per_group * act_dim;
    hipLaunchKernelGGL(usim_plan_sample_kernel<true>, dim3((unsigned)((words + PN_WG - 1) / PN_WG)), dim3(PN_WG), 0, (hipStream_t)stream, mean_dev, sigma_elem_dev,
                       act_low_dev, act_high_dev, restart_dev, per_group, horizon, act_dim, words, smoothing, fresh, (uint32_t)seed, (uint32_t)(seed >> 32), counter,
                       counter_base_dev, cand_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_plan_refit(const float* cand_dev, const float* ret_dev, const float* act_low_dev, const float* act_high_dev, int groups, int per_group, int horizon,
                               int act_dim, int elites, float momentum, float sigma_min, float* mean_dev, float* sigma_elem_dev, int32_t* elite_dev, void* stream) {
    using namespace usim;
    if (!cand_dev || !ret_dev || !act_low_dev || !act_high_dev || !mean_dev || !sigma_elem_dev || !plan_shape_ok(groups, per_group, horizon, act_dim))
        return USIM_ERR_INVALID;
    if (per_group > PN_REFIT_MAXK || elites < 1 || elites > per_group || (int64_t)horizon * act_dim > INT_MAX) return USIM_ERR_INVALID;
    if (!(momentum >= 0.f && momentum < 1.f) || !(sigma_min > 0.f) || !isfinite(sigma_min)) return USIM_ERR_INVALID;       // (a NaN fails the comparisons)
    const float fresh = (float)(1.0 - (double)momentum);         // the weight of the elites' moments, rounded once
    hipLaunchKernelGGL(usim_plan_refit_kernel, dim3((unsigned)groups), dim3(PN_WG), 0, (hipStream_t)stream, cand_dev, ret_dev, act_low_dev, act_high_dev, per_group,
                       horizon, act_dim, (size_t)groups * per_group, elites, momentum, fresh, sigma_min, mean_dev, sigma_elem_dev, elite_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_plan_tail(const float* cand_dev, const float* weight_dev, const int32_t* best_dev, const int32_t* length_dev, const uint8_t* done_last_dev,
                              const float* pol_act_dev, const float* act_low_dev, const float* act_high_dev, int groups, int per_group, int horizon, int act_dim,
                              float temperature, float* next_mean_dev, void* stream) {
    using namespace usim;
    if (!cand_dev || !weight_dev || !best_dev || !length_dev || !done_last_dev || !pol_act_dev || !act_low_dev || !act_high_dev || !next_mean_dev ||
        !plan_shape_ok(groups, per_group, horizon, act_dim))
        return USIM_ERR_INVALID;
    if (!(temperature >= 0.f) || !isfinite(temperature)) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_plan_tail_kernel, dim3((unsigned)groups), dim3(PN_WG), 0, (hipStream_t)stream, cand_dev, weight_dev, best_dev, length_dev, done_last_dev,
                       pol_act_dev, act_low_dev, act_high_dev, per_group, horizon, act_dim, (size_t)groups * per_group, temperature, next_mean_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}
