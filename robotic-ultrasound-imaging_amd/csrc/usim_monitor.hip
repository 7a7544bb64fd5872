// usim_monitor.hip -- usim_monitor_step and usim_explained_variance: the episode statistics of a training loop kept ON THE DEVICE.  SB3 wraps every environment in
// a Monitor (src/rl.py:39) and logs rollout/ep_rew_mean from a deque(maxlen = 100) of the finished episodes; the step kernels already leave done, ep_return and
// ep_length behind every usim_step, so the consumer is one small launch per step that stays inside a recorded rollout -- nothing is indexed by a mask, nothing
// synchronises.  A translation unit of its own: it shares nothing with the step kernels but the public header.
//
// The monitor block (32-bit words; include/usim.h USIM_MONITOR_*), all zero = an empty monitor:
//   [0..1] episodes (int64)   [2..3] length_sum (int64)   [4..5] return_sum (float64)   [6..7] truncated (int64)   [8..9] launches (int64)   [10..15] zero
//   [16 ..)  the ring: `window` rows {return bits, length, environment index, low 32 bits of `launches` before this launch advanced it}
//
// usim_monitor_step: ONE workgroup of 1024 threads; thread t owns environments t, t + 1024, ...
//   pass 1  c = the number of counted environments (done != 0, and count < target where targets are given).  Without targets and with done on the 16-byte grid the
//           flags are read 16 bytes per load; otherwise environment by environment.
//   pass 2  chunk by chunk of 1024 environments: the rank of a counted environment among the counted ones = a running base over the chunks + the counts of the lower
//           waves of its chunk (through LDS) + the lower lanes of its wave (ballot).  Episode e = episodes + rank goes to ring row e mod window -- but only the last
//           `window` of the c are stored (rank >= c - window), so no row is stored twice in a launch.  count_dev is advanced, and every thread keeps its own partial
//           sums in the order of its environments.  The launch is a chain of memory round trips, not of arithmetic: a chunk's flag, return, length (and count /
//           target) are loaded together, and the next chunk's loads are issued before this chunk's barrier.
//   header  every thread reads it at the start; the partial sums are combined in a fixed order -- a butterfly over lane distances 32 .. 1 inside each wave, then the
//           16 waves in ascending order -- and thread 0 writes it once, after a barrier: read and advanced once per launch.
// The words of ep_return / ep_length where an environment is not counted are loaded and dropped: they enter nothing.  No atomics, nothing ordered by arrival, no workgroup waits
// for another (there is one): the same block and the same inputs give the same block bit for bit.
//
// usim_explained_variance: SB3's explained_variance(values, returns) = 1 - var(returns - values) / var(returns) in one launch of one workgroup: float64 sums of
// y - y[0], (y - y[0])^2, e - e[0], (e - e[0])^2 (e = y - v; the shift by the first element keeps a large mean from cancelling the variance), thread t over elements
// t, t + 1024, ... ascending, combined in the same fixed order as above.  NaN when var(returns) == 0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/usim.h"

namespace usim {

constexpr int MN_WG = 1024;                                      // threads of the one workgroup = environments per chunk
constexpr int MN_WAVES = MN_WG / 64;
static_assert(USIM_MONITOR_HEADER_WORDS == 16 && USIM_MONITOR_ROW_WORDS == 4, "block layout: a 64-byte header, 16-byte ring rows");

// number of non-zero bytes of w: bit 7 of every byte is set where the low seven bits carry into it or it is set already (no carry crosses a byte)
__device__ __forceinline__ uint32_t mn_nonzero_bytes(unsigned long long w) {
    constexpr unsigned long long LO7 = 0x7f7f7f7f7f7f7f7full;
    return (uint32_t)__popcll((((w & LO7) + LO7) | w) & ~LO7);
}

// the sum of v over the workgroup, the same bits in every thread: butterfly inside the wave, then the waves in ascending order.  `part` is MN_WAVES words of LDS.
template <typename T>
__device__ __forceinline__ T mn_block_sum(T v, T* part) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                             // the previous use of `part` has been read
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = part[0];
#pragma unroll
    for (int k = 1; k < MN_WAVES; ++k) s += part[k];
    return s;
}

__global__ __launch_bounds__(MN_WG) void usim_monitor_step_kernel(const uint8_t* __restrict__ done, const uint32_t* __restrict__ ep_return,
                                                                  const int32_t* __restrict__ ep_length, int n, int window, int horizon,
                                                                  const int32_t* __restrict__ target, int32_t* __restrict__ count, uint32_t* __restrict__ monitor) {
    __shared__ uint32_t wave_count[2][MN_WAVES];
    __shared__ double part_d[MN_WAVES];
    __shared__ long long part_l[MN_WAVES], part_t[MN_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long* head_l = reinterpret_cast<long long*>(monitor);
    const double* head_d = reinterpret_cast<const double*>(monitor);
    // the header, read by every thread (one address each: a broadcast) before anything else; written by thread 0 after the last barrier
    const long long episodes0 = head_l[0], length0 = head_l[1], truncated0 = head_l[3], launches0 = head_l[4];
    const double return0 = head_d[2];

    // the words of one environment.  ep_return / ep_length are loaded with the flag -- not after the rank is known, which would put a second memory round trip into
    // every chunk -- and used only where the environment is counted
    const int chunks = (int)(((long long)n + MN_WG - 1) / MN_WG);
    uint32_t cur_d = 0, cur_r = 0, nxt_d = 0, nxt_r = 0;        // flag byte, return bits
    int32_t cur_l = 0, cur_have = 0, cur_want = 1, nxt_l = 0, nxt_have = 0, nxt_want = 1;      // length; count and target (without targets: 0 < 1)
#define MN_FETCH(k, d_, r_, l_, have_, want_)                                                       \
    {                                                                                               \
        const long long e_ = (long long)(k) * MN_WG + t;                                            \
        d_ = 0; r_ = 0; l_ = 0; have_ = 0; want_ = 1;                                               \
        if (e_ < n) {                                                                               \
            d_ = done[e_]; r_ = ep_return[e_]; l_ = ep_length[e_];                                  \
            if (target) { have_ = count[e_]; want_ = target[e_]; }                                  \
        }                                                                                           \
    }
    MN_FETCH(0, cur_d, cur_r, cur_l, cur_have, cur_want)         // in flight during pass 1

    // ---- pass 1: c, the counted environments of this launch
    long long mine = 0;
    if (!target && (reinterpret_cast<uintptr_t>(done) & 15) == 0) {
        const uint4* d16 = reinterpret_cast<const uint4*>(done);
        const int quads = n / 16;
        for (int i = t; i < quads; i += MN_WG) {
            const uint4 v = d16[i];
            mine += mn_nonzero_bytes(((unsigned long long)v.y << 32) | v.x) + mn_nonzero_bytes(((unsigned long long)v.w << 32) | v.z);
        }
        if (t < (n & 15)) mine += done[(size_t)quads * 16 + t] != 0;
    } else {                                                     // targets, or a caller's array off the 16-byte grid: environment by environment
        for (long long i = t; i < n; i += MN_WG) mine += done[i] != 0 && (!target || count[i] < target[i]);
    }
    const long long c = mn_block_sum(mine, part_l);
    const long long keep_from = c - (long long)window;          // ranks below this would be overwritten inside this launch: not stored

    // ---- pass 2: rank, ring rows, count_dev, partial sums
    double ret_sum = 0.0;
    long long len_sum = 0, trunc = 0, base = 0;
    for (int k = 0; k < chunks; ++k) {
        const long long env = (long long)k * MN_WG + t;
        if (k + 1 < chunks) MN_FETCH(k + 1, nxt_d, nxt_r, nxt_l, nxt_have, nxt_want)      // the next chunk's loads are issued before this chunk's barrier (another environment: count_dev[env] below does not alias)
        const bool counted = cur_d != 0 && cur_have < cur_want;
        if (counted && target) count[env] = cur_have + 1;
        const unsigned long long bal = __ballot(counted);
        uint32_t* wc = wave_count[k & 1];                        // two buffers: a wave two chunks ahead would have had to pass the barrier of the chunk between
        if (lane == 0) wc[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, here = 0;
#pragma unroll
        for (int w = 0; w < MN_WAVES; ++w) {
            const uint32_t x = wc[w];
            if (w < wave) before += x;
            here += x;
        }
        if (counted) {
            const long long rank = base + before + (long long)__popcll(bal & ((1ull << lane) - 1ull));
            const uint32_t r = cur_r;
            const int32_t l = cur_l;
            ret_sum += (double)__uint_as_float(r);
            len_sum += l;
            trunc += horizon > 0 && l >= horizon;
            if (rank >= keep_from) {
                long long row = (episodes0 + rank) % (long long)window;
                if (row < 0) row += window;                      // (a block that was not a monitor's: still inside the ring)
                reinterpret_cast<uint4*>(monitor + USIM_MONITOR_HEADER_WORDS)[row] = make_uint4(r, (uint32_t)l, (uint32_t)env, (uint32_t)launches0);
            }
        }
        base += here;
        cur_d = nxt_d; cur_r = nxt_r; cur_l = nxt_l; cur_have = nxt_have; cur_want = nxt_want;
    }
#undef MN_FETCH

    // ---- header: read (above) and advanced once per launch.  The three sums in one exchange: a butterfly inside each wave, then the waves in ascending order
    for (int o = 32; o > 0; o >>= 1) {
        ret_sum += __shfl_xor(ret_sum, o);
        len_sum += __shfl_xor(len_sum, o);
        trunc += __shfl_xor(trunc, o);
    }
    __syncthreads();                                             // pass 1's sum has been read out of part_l
    if (lane == 0) { part_d[wave] = ret_sum; part_l[wave] = len_sum; part_t[wave] = trunc; }
    __syncthreads();
    if (t == 0) {
        double ret_all = part_d[0];
        long long len_all = part_l[0], trunc_all = part_t[0];
#pragma unroll
        for (int w = 1; w < MN_WAVES; ++w) { ret_all += part_d[w]; len_all += part_l[w]; trunc_all += part_t[w]; }
        head_l[0] = episodes0 + base;
        head_l[1] = length0 + len_all;
        reinterpret_cast<double*>(monitor)[2] = return0 + ret_all;
        head_l[3] = truncated0 + trunc_all;
        head_l[4] = launches0 + 1;
        head_l[5] = 0; head_l[6] = 0; head_l[7] = 0;
    }
}

__global__ __launch_bounds__(MN_WG) void usim_explained_variance_kernel(const float* __restrict__ values, const float* __restrict__ returns, long long count,
                                                                        float* __restrict__ out) {
    __shared__ double part[MN_WAVES];
    const double y0 = (double)returns[0], e0 = y0 - (double)values[0];
    double sy = 0.0, syy = 0.0, se = 0.0, see = 0.0;
    for (long long i = threadIdx.x; i < count; i += MN_WG) {
        const double yr = (double)returns[i];
        const double y = yr - y0, e = (yr - (double)values[i]) - e0;
        sy += y; syy = fma(y, y, syy);
        se += e; see = fma(e, e, see);
    }
    sy = mn_block_sum(sy, part); syy = mn_block_sum(syy, part);
    se = mn_block_sum(se, part); see = mn_block_sum(see, part);
    if (threadIdx.x == 0) {
        const double N = (double)count, my = sy / N, me = se / N;
        const double var_y = syy / N - my * my, var_e = see / N - me * me;
        out[0] = var_y == 0.0 ? __uint_as_float(0x7fc00000u) : (float)(1.0 - var_e / var_y);
    }
}

}  // namespace usim

extern "C" int usim_monitor_words(int window) {
    if (window < 1 || window > USIM_MONITOR_MAX_WINDOW) return USIM_ERR_INVALID;
    return USIM_MONITOR_HEADER_WORDS + USIM_MONITOR_ROW_WORDS * window;
}

extern "C" int usim_monitor_step(const usim_step_io* io, int n, int window, int horizon, const int32_t* target_dev, int32_t* count_dev, uint32_t* monitor_dev,
                                 void* stream) {
    using namespace usim;
    if (!io || !io->done_dev || !io->ep_return_dev || !io->ep_length_dev || !monitor_dev || (reinterpret_cast<uintptr_t>(monitor_dev) & 15) || n <= 0 ||
        window < 1 || window > USIM_MONITOR_MAX_WINDOW || (target_dev && !count_dev))
        return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_monitor_step_kernel, dim3(1), dim3(MN_WG), 0, (hipStream_t)stream, io->done_dev, reinterpret_cast<const uint32_t*>(io->ep_return_dev),
                       io->ep_length_dev, n, window, horizon, target_dev, count_dev, monitor_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_explained_variance(const float* values_dev, const float* returns_dev, int64_t count, float* out_dev, void* stream) {
    using namespace usim;
    if (!values_dev || !returns_dev || !out_dev || count <= 0) return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_explained_variance_kernel, dim3(1), dim3(MN_WG), 0, (hipStream_t)stream, values_dev, returns_dev, (long long)count, out_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}
