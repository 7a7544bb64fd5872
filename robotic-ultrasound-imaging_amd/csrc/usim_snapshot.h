// usim_snapshot.h -- usim_save_envs / usim_load_envs: the state of whole environments copied between the handle's state block and a caller-owned device buffer of
// rows (include/usim.h "snapshots"), one kernel launch each way.  Included by usim_api.hip behind the step kernels; it shares only the layout of usim_device.h with them.
//
// A row is the environment's part of the three environment-major regions of the block, one behind the other, as 16-byte quads:
//   [0, 10)                  the F_NSCALAR scalar words at scalar_index(0, env)
//   [10, 10 + lat / 4)       the lattice words of the environment in the F_LAT region (lat = LAT_ENV_WORDS, LATF_ENV_WORDS, or 0 for the rigid torso)
//   then                     the WARM_WORDS warm words at warm_index(.., env), where the handle keeps them
// Every region starts on a 16-byte boundary for every environment (n_pad is a multiple of 64, every per-environment size a multiple of 4 words).
// One group of G lanes moves one row, quad q of the row by lane q mod G: G = 16 for the 10 / 60 / 78 quads of the rigid and top-face rows, a whole wave for the 438 quads
// of the full torso.  The environment / row number is checked against its range before any address is formed from it.
#pragma once
#include "usim_device.h"

namespace usim {

constexpr int SNAP_WG = 256;                                        // threads per workgroup: SNAP_WG / G rows
static_assert(F_NSCALAR % 4 == 0 && LAT_ENV_WORDS % 4 == 0 && LATF_ENV_WORDS % 4 == 0 && WARM_WORDS % 4 == 0 && BANK_ROWS % 4 == 0, "rows and regions are whole 16-byte quads");
constexpr int SNAP_EPISODE_QUAD = F_EPISODE / 4, SNAP_EPISODE_LANE = F_EPISODE % 4;      // the quad of the scalar words that holds the episode counter, and its word

struct SnapLayout { int lat_words, warm_words, bank_row0; };      // of the handle: lattice words per environment (0: none), warm words (0: none), first bank row (warm_index)
__host__ __device__ inline int snap_row_words(const SnapLayout& L) { return F_NSCALAR + L.lat_words + L.warm_words; }

// the quad-aligned start of the three regions of environment `env` inside the state block
struct SnapRegions { size_t scalar, lattice, warm; };
__device__ __forceinline__ SnapRegions snap_regions(const SnapLayout& L, int npad, size_t env) {
    return {scalar_index(0, env), (size_t)F_LAT * npad + env * (size_t)L.lat_words, warm_index(L.bank_row0, npad, env)};
}

// row r of snap <- environment env_index[r] (nullptr: r).  An index outside [0, n) leaves its row as it is.
template <int G>
__global__ __launch_bounds__(SNAP_WG) void usim_save_envs_kernel(const float* __restrict__ st, int n, int npad, SnapLayout L, const int* __restrict__ env_index, int m,
                                                                  float* __restrict__ snap) {
    const size_t row = ((size_t)blockIdx.x * SNAP_WG + threadIdx.x) / G;
    const int gl = threadIdx.x % G;
    if (row >= (size_t)m) return;
    const int env = env_index ? env_index[row] : (int)row;
    if (env < 0 || env >= n) return;
    const SnapRegions R = snap_regions(L, npad, (size_t)env);
    float4* const dst = reinterpret_cast<float4*>(snap + row * (size_t)snap_row_words(L));
    const float4* const sc = reinterpret_cast<const float4*>(st + R.scalar);
    const float4* const lat = reinterpret_cast<const float4*>(st + R.lattice);
    const float4* const wm = reinterpret_cast<const float4*>(st + R.warm);
    constexpr int QS = F_NSCALAR / 4;
    const int ql = L.lat_words / 4, qw = L.warm_words / 4;
    for (int q = gl; q < QS; q += G) dst[q] = sc[q];
    for (int q = gl; q < ql; q += G) dst[QS + q] = lat[q];
    for (int q = gl; q < qw; q += G) dst[QS + ql + q] = wm[q];
}

// environment i <- row row_of_env[i] of snap, every word but the episode counter.  A row number outside [0, m) keeps the environment.
template <int G>
__global__ __launch_bounds__(SNAP_WG) void usim_load_envs_kernel(float* __restrict__ st, int n, int npad, SnapLayout L, const float* __restrict__ snap, int m,
                                                                  const int* __restrict__ row_of_env) {
    const size_t env = ((size_t)blockIdx.x * SNAP_WG + threadIdx.x) / G;
    const int gl = threadIdx.x % G;
    if (env >= (size_t)n) return;
    const int row = row_of_env[env];
    if (row < 0 || row >= m) return;
    const SnapRegions R = snap_regions(L, npad, env);
    const float4* const src = reinterpret_cast<const float4*>(snap + (size_t)row * snap_row_words(L));
    float4* const sc = reinterpret_cast<float4*>(st + R.scalar);
    float4* const lat = reinterpret_cast<float4*>(st + R.lattice);
    float4* const wm = reinterpret_cast<float4*>(st + R.warm);
    constexpr int QS = F_NSCALAR / 4;
    const int ql = L.lat_words / 4, qw = L.warm_words / 4;
    for (int q = gl; q < QS; q += G) {
        float4 v = src[q];
        if (q == SNAP_EPISODE_QUAD) (&v.x)[SNAP_EPISODE_LANE] = st[R.scalar + F_EPISODE];        // the environment keeps its own episode counter (its bank ring is keyed on it)
        sc[q] = v;
    }
    for (int q = gl; q < ql; q += G) lat[q] = src[QS + q];
    for (int q = gl; q < qw; q += G) wm[q] = src[QS + ql + q];
}

}  // namespace usim
