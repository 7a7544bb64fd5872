// usim_metrics.hip -- usim_metrics_step and usim_record_step: the evaluation side of the reference's workflow kept ON THE DEVICE.  The reference states its results as
// the thirteen error metrics of src/utils/error.py:148-191 over the 24 CSV files ultrasound.py:552-614 dumps per episode; the step kernels already emit every channel
// of those files for every environment (usim_step_io.log_dev, [n][53]), so the consumers are small launches after every usim_step that stay inside a recorded rollout:
// nothing is indexed by a mask, nothing synchronises.  A translation unit of its own: it shares nothing with the step kernels but the public header.
//
// The metrics block (32-bit words; include/usim.h USIM_METRICS_*), all zero = an empty one:
//   [0..1] episodes (int64)   [2..3] launches (int64)   [4..5] length_sum (int64)   [6..7] nonfinite (int64)   [8..33] total[13] (float64)   [34..59] total_sq[13] (float64)
//   [60..63] zero
//   [64 ..)                the ring: `window` rows of 32 words {13 float64 metrics, environment index, episode length, low 32 bits of `launches` before this call, 0, 0, 0}
//   [64 + 32 window ..)    the accumulators, float64 [n][13]
//
// usim_metrics_step is TWO launches, always the same two:
//   accumulate  one thread per (environment, metric), consecutive threads = consecutive doubles of the accumulators: acc[i][m] += term_m(row i), float64 on the float32
//               words widened first (the summands of error_metrics.step_terms).  The thirteen threads of an environment read the few words of its 53-word row they
//               need -- the lanes of a wave cover five neighbouring rows, whole cache lines of the record -- and which words is arithmetic on m, not a branch: the
//               record's words and the accumulator are loaded together, one memory round trip before the store.
//   append      ONE workgroup of 1024 threads; thread t owns environments t, t + 1024, ...
//     pass 1    c = the number of counted environments (done != 0, and count < target where targets are given).
//     pass 2    chunk by chunk of 1024 environments: the rank of a counted environment among the counted ones = a running base over the chunks + the counts of the lower
//               waves of its chunk (through LDS) + the lower lanes of its wave (ballot), as usim_monitor.hip ranks them; the next chunk's flags are loaded before this
//               chunk's barrier.  The thread of a done environment reads its accumulator row and zeroes it; a counted one divides by horizon and stores ring row
//               (episodes + rank) mod window -- only the last `window` of the c are stored -- and stages the thirteen values in LDS at its rank.  The stage holds
//               256 episodes: when a chunk runs past its end, and once after the last chunk, threads 0 .. 25 walk it IN RANK ORDER, thread m adding metric m to
//               total[m], thread 13 + m its square to total_sq[m]: the sums are sequential in ascending environment index, kept in registers between the walks.
//               An episode with a non-finite metric is skipped by the walk and counted in `nonfinite`.  A call that counts up to 256 episodes -- every step of a
//               rollout but the synchronised ones -- walks once and takes one barrier per chunk.
//     header    read by every thread at the start, written once after the last chunk: the integer sums through a butterfly and the waves in ascending order.
// No floating-point atomics, nothing ordered by arrival: the same block and the same inputs give the same block bit for bit.
//
// usim_record_step: one launch, one wave per tracked row r: lane 0 reads filled[r] and the time channel of environment env_index[r], every lane below 53 copies one
// word of the record into rows[r][filled[r]][t]; where the environment is done lane 0 closes the episode.  Index and t come from device memory: both are checked.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/usim.h"

namespace usim {

constexpr int MT_LOG = 53;                                       // words of one row of log_dev
constexpr int MT_TIME = 40;                                      // the time channel: (timestep - 1) / horizon * 100
constexpr int MT_M = USIM_METRICS;
constexpr int MT_ACC_WG = 256;                                   // accumulate: threads of one workgroup = (environment, metric) items
constexpr int MT_WG = 1024, MT_WAVES = MT_WG / 64;               // append: threads of the one workgroup = environments per chunk
constexpr int MT_STAGE = 256;                                    // append: episodes the LDS stage holds between two ordered walks
static_assert(USIM_METRICS == 13 && USIM_METRICS_HEADER_WORDS == 64 && USIM_METRICS_ROW_WORDS == 32, "block layout: a 256-byte header, 128-byte ring rows");
static_assert(8 + 4 * MT_M == 60 && 2 * MT_M + 3 <= USIM_METRICS_ROW_WORDS, "header and ring row hold thirteen float64 metrics");

// t of a row: rint(time * horizon / 100) in float64, the rule of episode_log.EpisodeLogger (Python's round() is to even, as rint)
__device__ __forceinline__ double mt_row_time(uint32_t time_bits, int horizon) { return rint((double)__uint_as_float(time_bits) * (double)horizon / 100.0); }

// the columns of summand m of error_metrics.step_terms, a byte each: m < 7 is (A - B)^2 -- A of m = 5 being the norm of columns 6, 7, 8 --, m >= 7 is column A itself
constexpr unsigned long long MT_COL_A_LO = 0x130a061716140100ull;    // m = 0 .. 7:  0, 1, 20, 22, 23, 6, 10, 19
constexpr unsigned long long MT_COL_A_HI = 0x0000002b2d2c2a29ull;    // m = 8 .. 12: 41, 42, 44, 45, 43
constexpr unsigned long long MT_COL_B_LO = 0x0009091815150403ull;    // m = 0 .. 6:  3, 4, 21, 21, 24, 9, 9  (m >= 7: column 0, loaded and dropped)

__global__ __launch_bounds__(MT_ACC_WG) void usim_metrics_accumulate_kernel(const float* __restrict__ log, int n, double* __restrict__ acc) {
    const long long item = (long long)blockIdx.x * MT_ACC_WG + threadIdx.x;        // (environment, metric) = a double of the accumulators
    if (item >= (long long)n * MT_M) return;
    const long long e = item / MT_M;
    const int m = (int)(item - e * MT_M), shift = 8 * (m & 7);
    const int col_a = (int)(((m < 8 ? MT_COL_A_LO : MT_COL_A_HI) >> shift) & 0xff), col_b = m < 8 ? (int)((MT_COL_B_LO >> shift) & 0xff) : 0;
    const float* row = log + e * MT_LOG;
    const double before = acc[item];                             // in flight with the record's words
    const float wa = row[col_a], wb = row[col_b], wy = row[7], wz = row[8];
    double a = (double)wa;
    const double b = (double)wb, y = (double)wy, z = (double)wz;
    if (m == 5) a = sqrt(a * a + y * y + z * z);                 // |v|
    const double d = a - b;
    acc[item] = before + (m < 7 ? d * d : a);
}

__global__ __launch_bounds__(MT_WG) void usim_metrics_append_kernel(const uint8_t* __restrict__ done, const uint32_t* __restrict__ log, int n, int window, int horizon,
                                                                    const int32_t* __restrict__ target, int32_t* __restrict__ count, uint32_t* __restrict__ block) {
    __shared__ uint32_t wave_count[2][MT_WAVES];
    __shared__ double stage[MT_STAGE][MT_M];                     // the finished metrics of the counted environments of ranks staged_from .. staged_from + MT_STAGE - 1
    __shared__ uint8_t stage_ok[MT_STAGE];                       // ... all thirteen finite
    __shared__ long long part[3][MT_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long* head_l = reinterpret_cast<long long*>(block);
    double* head_d = reinterpret_cast<double*>(block);
    double* acc = reinterpret_cast<double*>(block + USIM_METRICS_HEADER_WORDS + (size_t)USIM_METRICS_ROW_WORDS * window);
    // the header, read by every thread (one address each: a broadcast) before anything else; written after the last chunk
    const long long episodes0 = head_l[0], launches0 = head_l[1], length0 = head_l[2], nonfinite0 = head_l[3];
    double running = t < 2 * MT_M ? head_d[4 + t] : 0.0;        // thread m: total[m]; thread 13 + m: total_sq[m]

    // the flag (and count / target) of one environment of this thread; the next chunk's are loaded before this chunk's barrier
    uint32_t nxt_d = 0;
    int32_t nxt_have = 0, nxt_want = 1;                          // (without targets: 0 < 1)
#define MT_FETCH(k)                                                                                 \
    {                                                                                               \
        const long long e_ = (long long)(k) * MT_WG + t;                                            \
        nxt_d = 0; nxt_have = 0; nxt_want = 1;                                                      \
        if (e_ < n) {                                                                               \
            nxt_d = done[e_];                                                                       \
            if (target) { nxt_have = count[e_]; nxt_want = target[e_]; }                            \
        }                                                                                           \
    }
    MT_FETCH(0)                                                  // in flight during pass 1

    // ---- pass 1: c, the counted environments of this call
    long long mine = 0;
    for (long long i = t; i < n; i += MT_WG) mine += done[i] != 0 && (!target || count[i] < target[i]);
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane == 0) part[0][wave] = mine;
    __syncthreads();
    long long c = 0;
#pragma unroll
    for (int w = 0; w < MT_WAVES; ++w) c += part[0][w];
    const long long keep_from = c - (long long)window;          // ranks below this would be overwritten inside this call: not stored

    // ---- pass 2: accumulator rows of the done environments, rank, ring rows, count_dev, the ordered sums
    const double h = (double)horizon;
    long long len_sum = 0, bad = 0, base = 0;
    long long staged_from = 0;                                   // the rank of stage[0]
    // threads 0 .. 25 add the first `staged` episodes of the stage to their sums, one after the other
    auto walk = [&](uint32_t staged) {
        if (t < 2 * MT_M) {
            const int m = t < MT_M ? t : t - MT_M;
            const bool square = t >= MT_M;
            for (uint32_t j = 0; j < staged; ++j) {
                if (!stage_ok[j]) continue;
                const double v = stage[j][m];
                running += square ? v * v : v;
            }
        }
    };
    const int chunks = (int)(((long long)n + MT_WG - 1) / MT_WG);
    for (int k = 0; k < chunks; ++k) {
        const long long env = (long long)k * MT_WG + t;
        const uint32_t cur_d = nxt_d;
        const int32_t cur_have = nxt_have, cur_want = nxt_want;
        if (k + 1 < chunks) MT_FETCH(k + 1)                      // (another environment: the count_dev[env] store below does not alias)
        const bool is_done = cur_d != 0, counted = is_done && cur_have < cur_want;
        if (counted && target) count[env] = cur_have + 1;
        double fin[MT_M];
        int32_t length = 0;
        bool ok = true;
        if (is_done) {
            double* a = acc + env * MT_M;
            if (counted) {
                const uint32_t time_bits = log[env * MT_LOG + MT_TIME];
#pragma unroll
                for (int m = 0; m < MT_M; ++m) fin[m] = a[m];
#pragma unroll
                for (int m = 0; m < MT_M; ++m) {
                    fin[m] /= h;
                    ok = ok && isfinite(fin[m]);
                }
                const double td = mt_row_time(time_bits, horizon);
                length = td >= -1.0 && td < 2147483647.0 ? (int32_t)td + 1 : 0;       // (a time word that is not a step number: no length)
            }
#pragma unroll
            for (int m = 0; m < MT_M; ++m) a[m] = 0.0;           // zeroed for every done environment, counted or not
        }
        const unsigned long long bal = __ballot(counted);
        uint32_t* wc = wave_count[k & 1];                        // two buffers: a wave two chunks ahead would have had to pass the barrier of the chunk between
        if (lane == 0) wc[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, here = 0;
#pragma unroll
        for (int w = 0; w < MT_WAVES; ++w) {
            const uint32_t x = wc[w];
            if (w < wave) before += x;
            here += x;
        }
        const uint32_t slot = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (counted) {
            len_sum += length;
            bad += !ok;
            if (base + slot >= keep_from) {
                long long row = (episodes0 + base + slot) % (long long)window;
                if (row < 0) row += window;                      // (a block that was not a metrics block: still inside the ring)
                uint32_t* r32 = block + USIM_METRICS_HEADER_WORDS + (size_t)USIM_METRICS_ROW_WORDS * row;
                double* r64 = reinterpret_cast<double*>(r32);
#pragma unroll
                for (int m = 0; m < MT_M; ++m) r64[m] = fin[m];
                r32[2 * MT_M] = (uint32_t)env;
                r32[2 * MT_M + 1] = (uint32_t)length;
                reinterpret_cast<uint4*>(r32)[7] = make_uint4((uint32_t)launches0, 0u, 0u, 0u);
            }
        }
        // stage this chunk's counted episodes at their rank; the stage holds ranks [staged_from, staged_from + MT_STAGE): where the chunk runs past its end it is
        // walked first (`base`, `here` and `staged_from` are the same in every thread, so every thread takes the same barriers)
        const long long rank = base + slot, end = base + here;
        while (end - staged_from > MT_STAGE) {
            if (counted && rank >= staged_from && rank - staged_from < MT_STAGE) {
                stage_ok[rank - staged_from] = ok;
#pragma unroll
                for (int m = 0; m < MT_M; ++m) stage[rank - staged_from][m] = fin[m];
            }
            __syncthreads();                                     // staged
            walk(MT_STAGE);
            __syncthreads();                                     // walked: `stage` is free
            staged_from += MT_STAGE;
        }
        if (counted && rank >= staged_from) {                    // (below staged_from + MT_STAGE: end is)
            stage_ok[rank - staged_from] = ok;
#pragma unroll
            for (int m = 0; m < MT_M; ++m) stage[rank - staged_from][m] = fin[m];
        }
        base = end;
    }
    __syncthreads();                                             // the last episodes are staged
    walk((uint32_t)(base - staged_from));
#undef MT_FETCH

    // ---- header: advanced once per call
    for (int o = 32; o > 0; o >>= 1) {
        len_sum += __shfl_xor(len_sum, o);
        bad += __shfl_xor(bad, o);
    }
    if (lane == 0) { part[1][wave] = len_sum; part[2][wave] = bad; }
    __syncthreads();
    if (t < 2 * MT_M) head_d[4 + t] = running;
    if (t == 0) {
        long long len_all = 0, bad_all = 0;
#pragma unroll
        for (int w = 0; w < MT_WAVES; ++w) { len_all += part[1][w]; bad_all += part[2][w]; }
        head_l[0] = episodes0 + base;
        head_l[1] = launches0 + 1;
        head_l[2] = length0 + len_all;
        head_l[3] = nonfinite0 + bad_all;
        head_l[30] = 0; head_l[31] = 0;
    }
}

__global__ __launch_bounds__(64) void usim_record_step_kernel(const uint32_t* __restrict__ log, const uint8_t* __restrict__ done, int n, int horizon,
                                                              const int32_t* __restrict__ env_index, int m, int episodes, uint32_t* __restrict__ record) {
    const int r = blockIdx.x, lane = threadIdx.x;
    int32_t* filled = reinterpret_cast<int32_t*>(record);
    int32_t* lengths = filled + m;
    const size_t head = (((size_t)m + (size_t)m * episodes + 3) / 4) * 4;
    // lane 0 alone touches filled[r]; the others receive what it read
    int e = -1, f = 0, t = -1, length = 0, fin = 0;
    if (lane == 0) {
        e = env_index[r];
        f = filled[r];
        if (e >= 0 && e < n && f >= 0 && f < episodes) {
            const double td = mt_row_time(log[(size_t)e * MT_LOG + MT_TIME], horizon);
            if (td >= 0.0 && td < (double)horizon) t = (int)td;
            length = td >= -1.0 && td < 2147483647.0 ? (int)td + 1 : 0;
            fin = done[e] != 0;
        } else {
            e = -1;                                              // an index outside [0, n), or `episodes` episodes already: nothing is written
        }
    }
    e = __shfl(e, 0); f = __shfl(f, 0); t = __shfl(t, 0);
    if (e < 0) return;
    if (t >= 0 && lane < MT_LOG)
        record[head + (((size_t)r * episodes + f) * horizon + t) * MT_LOG + lane] = log[(size_t)e * MT_LOG + lane];
    if (lane == 0 && fin) {
        lengths[(size_t)r * episodes + f] = length;
        filled[r] = f + 1;
    }
}

}  // namespace usim

extern "C" int usim_metrics_words(int n, int window) {
    if (n <= 0 || window < 1 || window > USIM_MONITOR_MAX_WINDOW) return USIM_ERR_INVALID;
    const long long words = (long long)USIM_METRICS_HEADER_WORDS + (long long)USIM_METRICS_ROW_WORDS * window + 2ll * USIM_METRICS * n;
    return words > INT_MAX ? USIM_ERR_INVALID : (int)words;
}

extern "C" int usim_metrics_step(const usim_step_io* io, int n, int window, int horizon, const int32_t* target_dev, int32_t* count_dev, uint32_t* metrics_dev,
                                 void* stream) {
    using namespace usim;
    if (!io || !io->log_dev || !io->done_dev || !metrics_dev || (reinterpret_cast<uintptr_t>(metrics_dev) & 15) || n <= 0 || horizon <= 0 || window < 1 ||
        window > USIM_MONITOR_MAX_WINDOW || (target_dev && !count_dev))
        return USIM_ERR_INVALID;
    double* acc = reinterpret_cast<double*>(metrics_dev + USIM_METRICS_HEADER_WORDS + (size_t)USIM_METRICS_ROW_WORDS * window);
    const unsigned groups = (unsigned)(((long long)n * MT_M + MT_ACC_WG - 1) / MT_ACC_WG);
    hipLaunchKernelGGL(usim_metrics_accumulate_kernel, dim3(groups), dim3(MT_ACC_WG), 0, (hipStream_t)stream, io->log_dev, n, acc);
    hipLaunchKernelGGL(usim_metrics_append_kernel, dim3(1), dim3(MT_WG), 0, (hipStream_t)stream, io->done_dev, reinterpret_cast<const uint32_t*>(io->log_dev), n, window,
                       horizon, target_dev, count_dev, metrics_dev);
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}

extern "C" int usim_record_words(int m, int episodes, int horizon) {
    if (m <= 0 || episodes <= 0 || horizon <= 0) return USIM_ERR_INVALID;
    const long long slots = (long long)m * episodes;
    if (slots > INT_MAX) return USIM_ERR_INVALID;
    const long long head = ((long long)m + slots + 3) / 4 * 4;
    if (slots * horizon > INT_MAX) return USIM_ERR_INVALID;
    const long long words = head + slots * horizon * 53;
    return words > INT_MAX ? USIM_ERR_INVALID : (int)words;
}

extern "C" int usim_record_step(const usim_step_io* io, int n, int horizon, const int32_t* env_index_dev, int m, int episodes, float* record_dev, void* stream) {
    using namespace usim;
    if (!io || !io->log_dev || !io->done_dev || !env_index_dev || !record_dev || (reinterpret_cast<uintptr_t>(record_dev) & 15) || n <= 0 || m <= 0 || episodes <= 0 ||
        horizon <= 0)
        return USIM_ERR_INVALID;
    hipLaunchKernelGGL(usim_record_step_kernel, dim3((unsigned)m), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(io->log_dev), io->done_dev, n,
                       horizon, env_index_dev, m, episodes, reinterpret_cast<uint32_t*>(record_dev));
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}
