// usim_checkpoint.h -- the layout of a handle's state block, and the checkpoint conversions between that block and the host arrays of usim_get_state / usim_set_state,
// usim_get_body_state / usim_set_body_state, usim_get_warm_start / usim_set_warm_start.  Host arithmetic over host buffers only, no HIP call: usim_api.hip copies the
// block down, calls one function of this file and copies it up; tests/checkpoint_dump.hip runs the same functions on a machine without a GPU (tests/test_checkpoint_host.py).
//
// Every conversion is one loop, written once for both directions (Dir: TO_DEVICE host arrays -> device words, TO_HOST device words -> host arrays; the device side
// is the first argument both ways), over rules that state a word's two directions side by side (word_*).
#pragma once
#include <cstddef>
#include <cstring>

#include "../../include/usim.h"
#include "usim_device.h"

namespace usim {

// The state block of a handle, in words:
//   [0, F_NSCALAR * npad)                    the scalar words, environment-major (scalar_index)
//   [F_LAT * npad, nfields * npad)           the lattice words, lat_words per environment (none: rigid torso), s at lat_s, sdot at lat_sd of an environment's words
//   [bank_row0 * npad, + BANK_ROWS * npad)   the reset bank
//   [warm(0), + warm_words * npad)           the warm rows (warm_words = 0: not allocated)
struct StateLayout {
    int n, npad, n_el, nfields;               // environments, rounded up to the workgroup width; dynamic torso elements; live words per environment
    int lat_words, lat_s, lat_sd;
    int bank_row0, warm_words;
    size_t words;                             // the whole allocation
    size_t live_words() const { return (size_t)nfields * npad; }                       // scalar and lattice region: what usim_get_state / usim_set_state move
    size_t lattice(size_t i) const { return (size_t)F_LAT * npad + i * lat_words; }   // environment i's lattice words
    size_t warm(size_t i) const { return warm_index(bank_row0, npad, i); }            // environment i's warm row
    constexpr int snapshot_words() const { return nfields + warm_words; }              // a snapshot row: an environment's part of every region but the bank (usim_snapshot.h)
};
constexpr StateLayout state_layout(int torso, int n_el, int n, bool warm) {
    const bool full = torso == USIM_TORSO_FULL;
    const int npad = (n + WG - 1) / WG * WG, lat = full ? LATF_ENV_WORDS : (n_el ? LAT_ENV_WORDS : 0), nfields = F_NSCALAR + lat, warm_words = warm ? WARM_WORDS : 0;
    return {n, npad, n_el, nfields, lat, full ? LATF_S : LAT_S, full ? LATF_SD : LAT_SD, nfields /* the bank follows the live rows */, warm_words,
            (size_t)(nfields + BANK_ROWS) * npad + (size_t)warm_words * npad};
}
static_assert(state_layout(USIM_TORSO_NONE, 0, 1, false).nfields == F_NSCALAR && state_layout(USIM_TORSO_TOP, N_TOP, 1, true).nfields == F_TOTAL_TOP &&
              state_layout(USIM_TORSO_FULL, NSH, 1, false).nfields == F_TOTAL_FULL && state_layout(USIM_TORSO_TOP, N_TOP, 65, true).npad == 128, "usim_device.h");
static_assert(state_layout(USIM_TORSO_NONE, 0, 1, false).snapshot_words() == USIM_SNAPSHOT_WORDS_RIGID && state_layout(USIM_TORSO_TOP, N_TOP, 1, false).snapshot_words() == USIM_SNAPSHOT_WORDS_TOP &&
              state_layout(USIM_TORSO_TOP, N_TOP, 1, true).snapshot_words() == USIM_SNAPSHOT_WORDS_TOP_WARM && state_layout(USIM_TORSO_FULL, NSH, 1, false).snapshot_words() == USIM_SNAPSHOT_WORDS_FULL, "include/usim.h");
static_assert(USIM_NSCALAR == F_NSCALAR && USIM_WARM_WORDS == WARM_WORDS && USIM_FULL_BODY_WORDS == 13 + LATF_WARM_WORDS, "include/usim.h");

// ---- the rules: a device word against a host number, both directions ------------------------------------------------------------------------------------
enum Dir : bool { TO_HOST = false, TO_DEVICE = true };
inline float int_bits(int v) { float f; std::memcpy(&f, &v, 4); return f; }
inline int bits_int(float f) { int v; std::memcpy(&v, &f, 4); return v; }
// the same number (float32 on both sides, or a float64 host number narrowed)
template <Dir TO, class D, class H> inline void word_copy(D& dev, H& host) { if constexpr (TO == TO_DEVICE) dev = (float)host; else host = dev; }
// an int on the device, its number on the host (truncated on the way down)
template <Dir TO, class D, class H> inline void word_int(D& dev, H& host) { if constexpr (TO == TO_DEVICE) dev = int_bits((int)host); else host = (H)bits_int(dev); }
// a joint angle: the device holds the excursion dq = q - q0 from the initial pose of the episode (q0 from the side that is read)
template <Dir TO, class D, class H> inline void word_joint(D& dq, H& q, float q0) { if constexpr (TO == TO_DEVICE) dq = q - q0; else q = q0 + dq; }
// a float32 relative to `off` on the device, the float64 sum on the host: exact, so that get -> set restores the bits
template <Dir TO, class D, class H> inline void word_offset(D& dev, H& host, double off) { if constexpr (TO == TO_DEVICE) dev = (float)(host - off); else host = (double)dev + off; }
// an element of the top face in a contact slot: an int on the device, -1 an empty slot; a host number outside [0, N_TOP) (a NaN fails both comparisons) is an empty slot
template <Dir TO, class D, class H> inline void word_element(D& dev, H& host) {
    if constexpr (TO == TO_DEVICE) dev = int_bits(host >= 0.f && host < (float)N_TOP ? (int)host : -1); else host = (float)bits_int(dev);
}

enum class Rule : int { COPY, JOINT, INT };
constexpr Rule scalar_rule(int f) {             // of scalar field f (usim_device.h Field)
    return f >= F_Q && f < F_Q + NJ ? Rule::JOINT : (f == F_T || f == F_TOUCH || f == F_EPISODE || f == F_STATUS) ? Rule::INT : Rule::COPY;
}

// ---- usim_get_state / usim_set_state: `block` the first live_words() words of the state block, scalars [n][USIM_NSCALAR], lattice [n][n_el][2] (s, sdot) or nullptr.
// Words of the padding environments and lattice words that are neither s nor sdot are not touched.
template <Dir TO, class D, class H> inline void state_words(const StateLayout& L, D* block, H* scalars, H* lattice) {
    for (int i = 0; i < L.n; ++i) {
        D* const dev = block + scalar_index(0, i);
        H* const host = scalars + (size_t)i * USIM_NSCALAR;
        const float* const src = TO == TO_DEVICE ? host : dev;
        for (int f = 0; f < F_NSCALAR; ++f) {
            if (scalar_rule(f) == Rule::JOINT) word_joint<TO>(dev[f], host[f], src[F_Q0 + f - F_Q]);
            else if (scalar_rule(f) == Rule::INT) word_int<TO>(dev[f], host[f]);
            else word_copy<TO>(dev[f], host[f]);
        }
        if (!lattice) continue;
        D* const s = block + L.lattice(i) + L.lat_s, * const sd = block + L.lattice(i) + L.lat_sd;
        H* const el = lattice + (size_t)i * L.n_el * 2;
        for (int e = 0; e < L.n_el; ++e) word_copy<TO>(s[e], el[2 * e]);
        for (int e = 0; e < L.n_el; ++e) word_copy<TO>(sd[e], el[2 * e + 1]);
    }
}

// ---- usim_get_body_state / usim_set_body_state (full torso): `lat` the lattice region of the block (from word lattice(0)), body [n][USIM_FULL_BODY_WORDS] float64 -- pose
// and velocity of the free body (13: position (world), quaternion w x y z, linear velocity (world), angular velocity (body frame)), then the warm start of the contact solve
// (LATF_WARM_WORDS: every element's table-contact force and multiplier, the probe slots' elements as numbers and forces).  float64 because the device holds the position
// relative to the robot base in float32.  s, sdot and the padding words between the regions are not touched.
constexpr bool probe_slot_element(int w) { return w >= 4 * NSH && w < 4 * NSH + 8; }      // warm-start word w holds the element number of a probe contact slot
template <Dir TO, class D, class H> inline void body_words(const StateLayout& L, const float* base, D* lat, H* body) {
    for (int i = 0; i < L.n; ++i) {
        D* const e = lat + (size_t)i * LATF_ENV_WORDS;
        H* const o = body + (size_t)i * USIM_FULL_BODY_WORDS;
        for (int a = 0; a < 13; ++a) word_offset<TO>(e[LATF_BODY + a], o[a], a < 3 ? (double)base[a] : 0.0);
        for (int w = 0; w < LATF_WARM_WORDS; ++w) {
            if (probe_slot_element(w)) word_int<TO>(e[LATF_WTAB + w], o[13 + w]);
            else word_copy<TO>(e[LATF_WTAB + w], o[13 + w]);
        }
    }
}

// ---- usim_get_warm_start / usim_set_warm_start (soft top-face torso with usim_config.warm_start): the kept contact list of the solver, rows of WARM_WORDS device words
// against [n][USIM_WARM_WORDS] float32 (the same rows with the elements as numbers)
template <Dir TO, class D, class H> inline void warm_words(int n, D* rows, H* w) {
    for (size_t k = 0; k < (size_t)n * WARM_WORDS; ++k) {
        if (k % WARM_WORDS < WARM_F) word_element<TO>(rows[k], w[k]);
        else word_copy<TO>(rows[k], w[k]);
    }
}
// "nothing kept": every slot empty, no force
inline void empty_warm(int n, float* rows) {
    for (size_t k = 0; k < (size_t)n * WARM_WORDS; ++k) rows[k] = k % WARM_WORDS < WARM_F ? int_bits(-1) : 0.f;
}
static_assert(WARM_EL == 0 && WARM_F == MAXC, "a warm row starts with its MAXC elements");

}  // namespace usim
