// usim_pack.hip -- usim_pack_step: everything the host needs from one usim_step in ONE contiguous block, so that a numpy-facing caller (vec_env.py step_async /
// step_wait, the SB3 VecEnv protocol of src/rl.py:130) moves it with one device-to-host copy, plus a second, short one on the steps where episodes ended.
// A translation unit of its own: it shares nothing with the step kernels but the public header.
//
// Layout of the block, in 32-bit words (include/usim.h USIM_PACK_*):
//   [0]                 c = number of finished environments (int32)          [1..3] zero
//   [4 .. 4 + 21 n)     head [n][21]: obs[19], rew, done as 0.0f / 1.0f
//   then                episode rows [c][23]: env index, ep_length, ep_return, status, terminal_observation[19] -- in ascending env index; rows >= c are not written
//
// One workgroup of 256 owns 256 consecutive environments.
//   head:  its 256 x 21 words are contiguous in the block and start on a 16-byte boundary (4 + 21 * 256 b words), so a thread builds four consecutive words and stores
//          them as one 16-byte store; the sources ([n][19] rows, rew, done) do not line up with that, so they are read word by word -- neighbouring lanes read
//          neighbouring words, the cache lines are shared.
//   rows:  the slot of a finished environment is the number of finished environments before it: (a) those of the workgroups before this one -- every workgroup counts
//          the non-zero bytes of done[0 .. 256 b) itself, 16 bytes per load (8 KB at 8192 environments, from L2 after the first workgroup); (b) those of the earlier waves
//          of this workgroup, through LDS; (c) those of the lower lanes of its wave, from the ballot.  No workgroup waits for another and nothing is ordered by arrival:
//          the same inputs give the same block, bit for bit.
// Floats travel as their bits (uint32_t): a NaN stays the same NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/usim.h"

namespace usim {

constexpr int PK_WG = 256;                                       // threads = environments per workgroup
constexpr int PK_HEAD = USIM_PACK_HEAD_WORDS, PK_ROW = USIM_PACK_EPISODE_WORDS, PK_OBS = USIM_OBS_DIM;
static_assert(PK_HEAD == PK_OBS + 2 && PK_ROW == PK_OBS + 4, "block layout: obs, rew, done / env, length, return, status, terminal observation");
static_assert((PK_WG * PK_HEAD) % 4 == 0, "a workgroup's part of the head starts on a 16-byte boundary");

struct PackArgs {
    const uint32_t* obs; const uint32_t* rew; const uint8_t* done;                                   // required
    const uint32_t* term; const uint32_t* ep_return; const uint32_t* ep_length; const uint32_t* status;    // each may be nullptr: zero words
};

// number of non-zero bytes of w: bit 7 of every byte is set where the low seven bits carry into it or it is set already (no carry crosses a byte: 0x7f + 0x7f < 0x100)
__device__ __forceinline__ uint32_t nonzero_bytes(unsigned long long w) {
    constexpr unsigned long long LO7 = 0x7f7f7f7f7f7f7f7full;
    return (uint32_t)__popcll((((w & LO7) + LO7) | w) & ~LO7);
}

// word `col` of head row `env`
__device__ __forceinline__ uint32_t head_word(const PackArgs& a, size_t env, int col) {
    if (col < PK_OBS) return a.obs[env * PK_OBS + col];
    if (col == PK_OBS) return a.rew[env];
    return a.done[env] ? 0x3f800000u : 0u;                       // 1.0f / 0.0f
}

__global__ __launch_bounds__(PK_WG) void usim_pack_step_kernel(PackArgs a, int n, uint32_t* __restrict__ packed) {
    __shared__ uint32_t before_part[PK_WG / 64], wave_count[PK_WG / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t first = (size_t)blockIdx.x * PK_WG;             // first environment of this workgroup (first < n by the grid size)
    const int mine = (size_t)n - first < (size_t)PK_WG ? (int)((size_t)n - first) : PK_WG;      // environments of this workgroup: 1 .. 256

    // ---- (a) finished environments before this workgroup: non-zero bytes of done[0 .. first), first a multiple of 256
    uint32_t before = 0;
    if ((reinterpret_cast<uintptr_t>(a.done) & 15) == 0) {
        const uint4* d16 = reinterpret_cast<const uint4*>(a.done);
        for (size_t i = t; i < first / 16; i += PK_WG) {
            const uint4 v = d16[i];
            before += nonzero_bytes(((unsigned long long)v.y << 32) | v.x) + nonzero_bytes(((unsigned long long)v.w << 32) | v.z);
        }
    } else {                                                     // a caller's array off the 16-byte grid: byte by byte
        for (size_t i = t; i < first; i += PK_WG) before += a.done[i] != 0;
    }
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);

    // ---- (b), (c) this workgroup's own flags
    const size_t env = first + t;
    const bool fin = t < mine && a.done[env] != 0;
    const unsigned long long bal = __ballot(fin);
    if (lane == 0) { before_part[wave] = before; wave_count[wave] = (uint32_t)__popcll(bal); }
    __syncthreads();
    uint32_t slot = 0, here = 0;                                 // slot: finished environments before this lane's; here: those of this workgroup
#pragma unroll
    for (int k = 0; k < PK_WG / 64; ++k) {
        slot += before_part[k];
        if (k < wave) slot += wave_count[k];
        here += wave_count[k];
    }
    const uint32_t wg_first_slot = before_part[0] + before_part[1] + before_part[2] + before_part[3];
    slot += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));

    // ---- the count, by the workgroup that owns the last environment: one 16-byte store (words 1 .. 3 zero)
    if (blockIdx.x == gridDim.x - 1 && t == 0) *reinterpret_cast<uint4*>(packed) = make_uint4(wg_first_slot + here, 0u, 0u, 0u);

    // ---- head: words [21 first, 21 (first + mine)) of the head, four at a time
    uint32_t* head = packed + 4 + first * PK_HEAD;
    const int words = mine * PK_HEAD;
    for (int q = t; q < words / 4; q += PK_WG) {
        int e = (4 * q) / PK_HEAD, col = 4 * q - e * PK_HEAD;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = head_word(a, first + e, col);
            if (++col == PK_HEAD) { col = 0; ++e; }
        }
        reinterpret_cast<uint4*>(head)[q] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    if (t < (words & 3)) {                                       // the ragged last workgroup: up to three words beyond the last whole quad
        const int wd = (words & ~3) + t, e = wd / PK_HEAD;
        head[wd] = head_word(a, first + e, wd - e * PK_HEAD);
    }

    // ---- episode row of a finished environment
    if (fin) {
        uint32_t* row = packed + 4 + (size_t)n * PK_HEAD + (size_t)slot * PK_ROW;
        row[0] = (uint32_t)env;
        row[1] = a.ep_length ? a.ep_length[env] : 0u;
        row[2] = a.ep_return ? a.ep_return[env] : 0u;
        row[3] = a.status ? a.status[env] : 0u;
#pragma unroll
        for (int k = 0; k < PK_OBS; ++k) row[4 + k] = a.term ? a.term[env * PK_OBS + k] : 0u;
    }
}

}  // namespace usim

extern "C" int usim_pack_step(const usim_step_io* io, int n, float* packed_dev, void* stream) {
    using namespace usim;
    if (!io || n <= 0 || !io->obs_dev || !io->rew_dev || !io->done_dev || !packed_dev || (reinterpret_cast<uintptr_t>(packed_dev) & 15)) return USIM_ERR_INVALID;
    const PackArgs a{reinterpret_cast<const uint32_t*>(io->obs_dev), reinterpret_cast<const uint32_t*>(io->rew_dev), io->done_dev,
                     reinterpret_cast<const uint32_t*>(io->term_obs_dev), reinterpret_cast<const uint32_t*>(io->ep_return_dev),
                     reinterpret_cast<const uint32_t*>(io->ep_length_dev), reinterpret_cast<const uint32_t*>(io->status_dev)};
    hipLaunchKernelGGL(usim_pack_step_kernel, dim3((unsigned)(((size_t)n + PK_WG - 1) / PK_WG)), dim3(PK_WG), 0, (hipStream_t)stream, a, n, reinterpret_cast<uint32_t*>(packed_dev));
    return hipGetLastError() == hipSuccess ? USIM_OK : USIM_ERR_HIP;
}
