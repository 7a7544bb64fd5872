// usim_setup.h -- everything usim_create (usim_api.hip) decides before it touches the device: host arithmetic only, no HIP call, so a program that includes this
// header runs on a machine without a GPU (tests/setup_dump.hip prints what it computes; tests/test_host_setup.py checks that against float64 restatements).
//   - the kernel mapping of a handle (Mapping, resolve_mapping);
//   - the defaults and the argument checks of usim_config (default_config, check_config);
//   - the model constants in double precision, narrowed once (build_model: link-7 composite inertia, arm table, torso lattice tables, the inverse of the lattice
//     normal matrix; ModelTables);
//   - the usim_config -> DevCfg translation with its derived probe and torso constants (translate_config).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/usim.h"
#include "usim_device.h"
#include "usim_robot.h"

namespace usim {

// Kernel mapping of a handle: which kernels its step launches and its reset / refill launches run (the launch table: kernel_of, usim_api.hip).
//   mapping     handle
//   FULL        full torso (lanes_per_env 0, 16, 32 or 64: ignored), one wave per environment
//   RIGID16     rigid torso, lanes 0 or 16 (waves_per_simd ignored)
//   SOFT16_W1   soft torso, lanes 16, 1 wave per SIMD
//   SOFT16_W2   soft torso, lanes 16, 2 waves per SIMD
//   SPLIT16     soft torso, lanes 32 (split kernel, 16-lane groups)
//   SPLIT8      soft torso, lanes 64 (split kernel, 8-lane groups)
// Soft torso, lanes 0: waves_per_simd 0 the split kernel -- up to 4096 envs/GPU lanes 32 (two waves per quad of environments, 16 environments per workgroup
// = one workgroup per CU), beyond lanes 64 (two environments per DPP row, 32 per workgroup: 8192 envs still one workgroup per CU, 23.8 vs 29.3 us/step;
// profiles/r03/bench_matrix.txt) --, a nonzero waves_per_simd (a register budget) lanes 16.  Waves per SIMD: the value given, else 1 up to 4096 envs, 2 beyond.
// Refused: waves_per_simd outside 0 .. 2, any other lanes_per_env; usim_set_mapping also refuses lanes 0 and rigid / full-torso handles.
enum class Mapping : int { FULL, RIGID16, SOFT16_W1, SOFT16_W2, SPLIT16, SPLIT8 };
inline bool resolve_mapping(int torso, int lanes_per_env, int waves_per_simd, int n_envs, Mapping* m) {
    if (waves_per_simd < 0 || waves_per_simd > 2) return false;
    if (torso == USIM_TORSO_NONE) { *m = Mapping::RIGID16; return lanes_per_env == 0 || lanes_per_env == 16; }
    if (lanes_per_env != 0 && lanes_per_env != 16 && lanes_per_env != 32 && lanes_per_env != 64) return false;
    const int lanes = lanes_per_env ? lanes_per_env : (waves_per_simd ? 16 : (n_envs <= 4096 ? 32 : 64));
    const int waves = waves_per_simd ? waves_per_simd : (n_envs <= 4096 ? 1 : 2);
    *m = torso == USIM_TORSO_FULL ? Mapping::FULL : lanes == 32 ? Mapping::SPLIT16 : lanes == 64 ? Mapping::SPLIT8 : (waves == 1 ? Mapping::SOFT16_W1 : Mapping::SOFT16_W2);
    return true;
}
constexpr bool soft_torso(Mapping m) { return m != Mapping::FULL && m != Mapping::RIGID16; }
constexpr bool multi_step(Mapping m) { return m != Mapping::FULL; }           // several control steps per launch (usim_rollout_random)
// control steps of the next launch of a rollout: what remains, at most kmax (the handle's steps per launch; 1 without multi_step), and never across the refill
// period of the reset bank, of which period_left steps remain (an environment consumes at most one ring slot per step)
constexpr int launch_steps(int remaining, int kmax, int period_left) {
    const int k = remaining < kmax ? remaining : kmax;
    return k < period_left ? k : period_left;
}
static_assert(launch_steps(1000, 256, 1) == 1, "a period with one step left");
static_assert(launch_steps(1000, 256, BANK_DEPTH) == 256 && launch_steps(1000, 64, BANK_DEPTH) == 64, "a period just refilled");
static_assert(launch_steps(1000, 1, BANK_DEPTH) == 1 && launch_steps(1000, 1, 1) == 1, "kmax = 1: one step per launch");
static_assert(launch_steps(3, 256, 200) == 3 && launch_steps(1, 256, BANK_DEPTH) == 1, "remaining smaller than everything");

// the defaults of usim_default_config (the caller has checked struct_size: nothing is written to a struct of another layout)
inline void default_config(usim_config* c) {
    std::memset(c, 0, sizeof *c);
    c->mode = USIM_MODE_TRACKING; c->torso = USIM_TORSO_TOP; c->horizon = 1000; c->early_termination = 1;
    c->deterministic_trajectory = 0; c->torso_solref_randomization = 1; c->initial_probe_pos_randomization = 1;
    c->friction_randomization = 0; c->torso_drop = 0; c->pgs_iters = 24; c->ik_iters = 5; c->env_offset = 0; c->lanes_per_env = 0; c->torso_shape = 0; c->waves_per_simd = 0; c->robot = 0; c->seed = 3;
    c->control_dt = 0.002; c->substeps = 1; c->kp_fixed = 300; c->damping_ratio = 1; c->kp_min = 0; c->kp_max = 500; c->out_max_pos = 0.05; c->out_max_ori = 0.5;
    c->stiffness = 1324.17; c->damping = 17.59; c->elem_friction = 0.01; c->probe_friction = 1e-4; c->probe_friction2 = 1.0; c->probe_geoms = 2; c->probe_radius = 0.021; c->probe_halflen = 0.0065;
    c->pair_model = 1; c->probe_radius2 = 0.035; c->probe_height = 0.020; c->probe_halfwidth = 0.0; c->probe_tip = -0.0005;      // round-4 fit, kept in round 5 (oracle: PROBE_*; profiles/r04/probe_fit.txt, profiles/r05/probe_fit.txt)
    c->armature_scale = 1.0; c->joint_frictionloss = 0.1;                 // robosuite's defaults for robot joints (include/usim.h)
    c->struct_size = (int32_t)sizeof(usim_config);
}

// the configurations usim_create refuses
inline bool check_config(const usim_config& c) {
    if (c.struct_size != (int32_t)sizeof(usim_config)) return false;     // built against another layout of include/usim.h
    if (c.probe_radius2 <= 0 || !(c.probe_height > std::fabs(c.probe_radius2 - c.probe_radius))) return false;
    if (!(c.probe_halfwidth >= 0) || !(std::fabs(c.probe_tip) <= 0.02) || c.torso_drop < 0 || c.torso_drop > 2) return false;
    if (c.mode < 0 || c.mode > 3 || c.torso < 0 || c.torso > 2 || !(c.armature_scale >= 0) || !(c.joint_frictionloss >= 0) || c.horizon <= 0 || c.control_dt <= 0 ||
        c.probe_halflen < 1e-4 || c.probe_radius <= 0 || c.pgs_iters < 0 || c.ik_iters < 0 || c.torso_shape < 0 ||
        c.torso_shape > 1 || c.waves_per_simd < 0 || c.waves_per_simd > 2 || c.robot < 0 || c.robot > 1 || c.warm_start < 0 || c.warm_start > 1) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// model data (the Panda chain constants themselves live in usim_kernels.hip)
// ---------------------------------------------------------------------------------------------------------
const double kGoalQuat[4] = {-0.69192486, 0.72186726, -0.00514253, -0.01100909};   // ultrasound.py:174 (x,y,z,w)
const double kBase[3] = {-0.56, 0.0, 0.913};                                         // ultrasound.py:279-280 + mount height
// torso spawn height = table 0.8 + z_offset 0.005 - bottom_site z (ultrasound.py:146,313): box -0.0522 (soft_box.xml:14), cylinder
// -0.05 (soft_human_torso.xml:14); trajectory height / waypoint grid width per shape (ultrasound.py:184,186)
const double kTorsoZ[2] = {0.8 + 0.005 + 0.0522, 0.8 + 0.005 + 0.05};
const double kTopOff[2] = {0.039, 0.041}, kYRange[2] = {0.09, 0.05};
const double kProbePos[3] = {-0.004, -0.063, 0.128};                                 // ultrasound_probe_gripper.xml:6
const double kProbeCom[3] = {0.0013, 0.021, -0.043};                                 // stand-in (mesh missing from the snapshot)
const double kProbeI[3] = {1.6e-3, 1.6e-3, 2.0e-4};

inline void pack_sym(const double I[3][3], float* o) { o[0] = (float)I[0][0]; o[1] = (float)I[0][1]; o[2] = (float)I[0][2]; o[3] = (float)I[1][1]; o[4] = (float)I[1][2]; o[5] = (float)I[2][2]; }

inline bool on_shell(int a, int b, int c) {
    if (a < 0 || a >= 9 || b < 0 || b >= 4 || c < 0 || c >= 11) return false;
    return a == 0 || a == 8 || b == 0 || b == 3 || c == 0 || c == 10;
}

// soft equality constraints of the lattice (composite solrefsmooth, d_max 0.95): weight of the pin to the rest position and of a tendon to a neighbour
const double kDMax = 0.95, kWFix = kDMax / (1 - kDMax), kWTen = 0.5 * kDMax / (1 - kDMax);
inline double lattice_diag(int nn) { return 1.0 + kWFix + kWTen * nn; }      // diagonal of the lattice Laplacian: an element with nn tendons

// one element of the 9 x 4 x 11 torso shell (soft_box.xml:9): lattice cell, world-axes position and slide axis (float, as uploaded), the shell ids
// of its 6-neighbourhood (x-, x+, y-, y+, z-, z+; -1 off the shell) and their number
struct ShellElement { int a, b, c; float pos[3], axis[3]; int nbr[6], nn; };

// the 270 shell elements in creation order (ix outer, iy, iz inner: the index is the shell id)
inline std::vector<ShellElement> torso_shell(int shape) {
    int id[9][4][11], n = 0;
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 4; ++b) for (int c = 0; c < 11; ++c) id[a][b][c] = on_shell(a, b, c) ? n++ : -1;
    std::vector<ShellElement> sh;
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 4; ++b) for (int c = 0; c < 11; ++c) {
        if (id[a][b][c] < 0) continue;
        ShellElement el{a, b, c, {}, {}, {}, 0};
        double loc[3] = {(a - 4) * 0.035, (b - 1.5) * 0.035, (c - 5) * 0.035};
        // composite type "cylinder" (soft_human_torso.xml:9): direction in the local x-y cross-section projected on the unit circle, max-norm radius kept ->
        // the box section becomes an ellipse 0.14 x 0.0525
        const double xn = loc[0] / 0.14, yn = loc[1] / 0.0525, l0 = std::fmax(std::fabs(xn), std::fabs(yn)), nn = std::sqrt(xn * xn + yn * yn);
        if (shape == 1 && nn > 0) { loc[0] = 0.14 * l0 * xn / nn; loc[1] = 0.0525 * l0 * yn / nn; }
        const double len = std::sqrt(loc[0] * loc[0] + loc[1] * loc[1] + loc[2] * loc[2]);
        const double w[3] = {-loc[2], -loc[0], loc[1]};                  // parent quat (0.5, 0.5, -0.5, -0.5): world x = -local z, y = -local x, z = local y
        for (int k = 0; k < 3; ++k) { el.pos[k] = (float)w[k]; el.axis[k] = (float)(w[k] / len); }
        const int d3[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
        for (int d = 0; d < 6; ++d) {
            const int a2 = a + d3[d][0], b2 = b + d3[d][1], c2 = c + d3[d][2];
            el.nbr[d] = on_shell(a2, b2, c2) ? id[a2][b2][c2] : -1;
            el.nn += el.nbr[d] >= 0;
        }
        sh.push_back(el);
    }
    return sh;
}

// dense symmetric positive definite inverse by Gauss-Jordan in double precision
inline std::vector<double> invert(std::vector<double> a, int n) {
    std::vector<double> inv((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r) if (std::fabs(a[(size_t)r * n + c]) > std::fabs(a[(size_t)p * n + c])) p = r;
        if (p != c) for (int k = 0; k < n; ++k) { std::swap(a[(size_t)p * n + k], a[(size_t)c * n + k]); std::swap(inv[(size_t)p * n + k], inv[(size_t)c * n + k]); }
        double d = 1.0 / a[(size_t)c * n + c];
        for (int k = 0; k < n; ++k) { a[(size_t)c * n + k] *= d; inv[(size_t)c * n + k] *= d; }
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            double f = a[(size_t)r * n + c];
            if (f == 0.0) continue;
            for (int k = 0; k < n; ++k) { a[(size_t)r * n + k] -= f * a[(size_t)c * n + k]; inv[(size_t)r * n + k] -= f * inv[(size_t)c * n + k]; }
        }
    }
    return inv;
}

// Arm table of the 16-lane kernels (usim_device.h ArmTable) from the z-aligned chain: lanes 0 .. 6 the links (padding links of a shorter
// chain: identity transform, no mass, no joint), lane 7 the end-effector site as a fixed child of the last link.
inline void build_arm_table(const usim_host::Chain& c, float* tb, const double armature_scale) {
    for (int l = 0; l < A16_LANES; ++l) {
        float* r = tb + l * AT_STRIDE;
        for (int k = 0; k < AT_STRIDE; ++k) r[k] = 0.f;
        r[AT_RFIX + 0] = 1.f; r[AT_RFIX + 4] = 1.f; r[AT_RFIX + 8] = 1.f;      // identity columns
        r[AT_QMIN] = -1.0e30f; r[AT_QMAX] = 1.0e30f; r[AT_TAUMAX] = 1.0f;
        const usim_host::M3* rot = nullptr; usim_host::V3 pos;
        if (l < NJ) {
            const usim_host::Link& k = c.link[l];
            rot = &k.rfix; pos = k.lpos;
            r[AT_LCOM] = (float)k.lcom.x; r[AT_LCOM + 1] = (float)k.lcom.y; r[AT_LCOM + 2] = (float)k.lcom.z;
            r[AT_MASS] = (float)k.mass;
            r[AT_INERTIA + 0] = (float)k.inertia.m[0][0]; r[AT_INERTIA + 1] = (float)k.inertia.m[0][1]; r[AT_INERTIA + 2] = (float)k.inertia.m[0][2];
            r[AT_INERTIA + 3] = (float)k.inertia.m[1][1]; r[AT_INERTIA + 4] = (float)k.inertia.m[1][2]; r[AT_INERTIA + 5] = (float)k.inertia.m[2][2];
            r[AT_QMIN] = (float)k.qmin; r[AT_QMAX] = (float)k.qmax; r[AT_TAUMAX] = (float)k.taumax; r[AT_INITQ] = (float)k.initq;
            r[AT_JOINT] = k.joint ? 1.f : 0.f;
            r[AT_ARMATURE] = k.joint ? (float)(armature_scale * 5.0 / (l + 1)) : 0.f;
        } else if (l == 7) { rot = &c.site_rot; pos = c.site; }
        if (rot) {
            for (int col = 0; col < 3; ++col) for (int row = 0; row < 3; ++row) r[AT_RFIX + 3 * col + row] = (float)rot->m[row][col];   // stored by columns
            r[AT_LPOS] = (float)pos.x; r[AT_LPOS + 1] = (float)pos.y; r[AT_LPOS + 2] = (float)pos.z;
        }
    }
}

// Full torso (usim_full.h): all 270 shell elements in creation order (ix outer, iy, iz inner: the shell id), their 6-neighbourhood restricted to the shell, and the
// constants of the torso's Hessian H = [M I, 0, m N; 0, I_b, 0; m N', 0, m L] in float64: L^-1, P = L^-1 N', S^-1 = (M I - m N P)^-1, I_b^-1.
inline int build_full_tables(int shape, std::vector<float>& words) {
    const double m = 0.01;
    std::vector<float> tb(FT_WORDS, 0.f);
    int* tbi = reinterpret_cast<int*>(tb.data());
    const std::vector<ShellElement> sh = torso_shell(shape);
    if ((int)sh.size() != NSH) return USIM_ERR_INVALID;
    std::vector<double> ax((size_t)NSH * 3), L((size_t)NSH * NSH, 0.0);
    for (int e = 0; e < FNE; ++e) { tb[FT_DIAG + e] = 1.f; for (int d = 0; d < 4; ++d) tbi[FT_NBR + 4 * e + d] = FNE - 1; }
    double mt = m, Ib[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};                 // 270 elements + the composite's centre geom, 0.01 kg each
    for (int e = 0; e < NSH; ++e) {
        const ShellElement& el = sh[e];
        double cpos[3];
        for (int k = 0; k < 3; ++k) {
            tb[FT_POS + 3 * e + k] = el.pos[k]; tb[FT_AXIS + 3 * e + k] = el.axis[k];
            ax[(size_t)e * 3 + k] = (double)el.axis[k];
            cpos[k] = (double)el.pos[k] - (0.0075 + 0.025) * ax[(size_t)e * 3 + k];          // capsule centre
        }
        mt += m;
        const double dd = cpos[0] * cpos[0] + cpos[1] * cpos[1] + cpos[2] * cpos[2];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Ib[3 * i + j] += m * ((i == j ? dd : 0.0) - cpos[i] * cpos[j]);
        int nn = 0;
        for (int d = 0; d < 6; ++d) {
            if (el.nbr[d] < 0) continue;
            if (nn >= 4) return USIM_ERR_INVALID;
            tbi[FT_NBR + 4 * e + nn++] = el.nbr[d];
            L[(size_t)e * NSH + el.nbr[d]] = -kWTen;
        }
        L[(size_t)e * NSH + e] = lattice_diag(nn);
        tb[FT_DIAG + e] = (float)lattice_diag(nn);
    }
    const std::vector<double> Li = invert(L, NSH);
    std::vector<double> P((size_t)NSH * 3, 0.0);
    for (int i = 0; i < NSH; ++i) for (int j = 0; j < NSH; ++j) {
        tb[FT_LINV + (size_t)i * FT_LROW + j] = (float)Li[(size_t)i * NSH + j];
        for (int k = 0; k < 3; ++k) P[(size_t)i * 3 + k] += Li[(size_t)i * NSH + j] * ax[(size_t)j * 3 + k];
    }
    std::vector<double> S(9, 0.0);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        double t = (i == j) ? mt : 0.0;
        for (int e = 0; e < NSH; ++e) t -= m * ax[(size_t)e * 3 + i] * P[(size_t)e * 3 + j];
        S[3 * i + j] = t;
    }
    const std::vector<double> Si = invert(S, 3), Ibi = invert(std::vector<double>(Ib, Ib + 9), 3);
    for (int e = 0; e < NSH; ++e) for (int k = 0; k < 3; ++k) tb[FT_P + 3 * e + k] = (float)P[(size_t)e * 3 + k];
    for (int k = 0; k < 9; ++k) { tb[FT_CONST + k] = (float)Si[k]; tb[FT_CONST + 9 + k] = (float)Ibi[k]; }
    tb[FT_CONST + 18] = (float)mt;
    tb[FT_CONST + 19] = (float)((1.0 / m + 2.0 / (NSH * m)) / 3.0);      // element alone: the table is static
    words.swap(tb);
    return USIM_OK;
}

// what build_model fills: the model constants (M.tables is set by usim_create, which uploads the words), the words of the handle's table block and its number of
// dynamic torso elements
struct ModelTables { DevModel M; std::vector<float> words; int n_el = 0; };

inline int build_model(const usim_config& cfg, ModelTables* out) {
    DevModel& M = out->M;
    std::memset(&M, 0, sizeof M);
    // robot chain (z-aligned, end effector folded into the last link): arm table + the end-effector constants of the kernels
    const usim_host::RobotDesc desc = (cfg.robot == USIM_ROBOT_UR5E) ? usim_host::ur5e_desc() : usim_host::panda_desc();
    const usim_host::Chain chain = usim_host::z_aligned_chain(desc, {kProbePos[0], kProbePos[1], kProbePos[2]}, {kProbeCom[0], kProbeCom[1], kProbeCom[2]},
                                                              {kProbeI[0], kProbeI[1], kProbeI[2]}, 1.0, 0.5, 0.05);
    {
        const usim_host::Link& last = chain.link[chain.nj - 1];
        M.m7 = (float)last.mass;
        const double c7[3] = {last.lcom.x, last.lcom.y, last.lcom.z}, s7[3] = {chain.site.x, chain.site.y, chain.site.z}, h7[3] = {chain.hand.x, chain.hand.y, chain.hand.z},
                     p7[3] = {chain.pcom.x, chain.pcom.y, chain.pcom.z}, ib[3] = {chain.ik_bias.x, chain.ik_bias.y, chain.ik_bias.z};
        for (int i = 0; i < 3; ++i) { M.c7[i] = (float)c7[i]; M.site7[i] = (float)s7[i]; M.hand7[i] = (float)h7[i]; M.pcom7[i] = (float)p7[i]; M.ikb[i] = (float)ib[i]; }
        pack_sym(last.inertia.m, M.I7); pack_sym(chain.pI.m, M.pI7);
    }
    const int shape = cfg.torso_shape ? 1 : 0;
    const double kTorso[3] = {0.0, 0.0, kTorsoZ[shape]};
    for (int i = 0; i < 3; ++i) { M.torso[i] = (float)(kTorso[i] - kBase[i]); M.base[i] = (float)kBase[i]; }
    {
        double x = kGoalQuat[0], y = kGoalQuat[1], z = kGoalQuat[2], w = kGoalQuat[3];
        double nn = std::sqrt(x * x + y * y + z * z + w * w); x /= nn; y /= nn; z /= nn; w /= nn;
        const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                             2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
        for (int i = 0; i < 9; ++i) M.grot[i] = (float)R[i];
        for (int i = 0; i < 4; ++i) M.gquat[i] = (float)kGoalQuat[i];
        M.ghat[0] = (float)w; M.ghat[1] = (float)x; M.ghat[2] = (float)y; M.ghat[3] = (float)z;
        M.geps = (float)(1.0 - nn);
    }
    M.wfix = (float)kWFix;
    M.wten = (float)kWTen;

    // one table block per handle: [lattice tables (soft torso) | arm table], laid out as the kernels read it
    std::vector<float>& tb = out->words;
    tb.assign(TB_TOTAL, 0.f);
    build_arm_table(chain, &tb[TB_ARM], cfg.armature_scale);
    for (int i = 0; i < NJ; ++i) M.armature[i] = chain.link[i].joint ? (float)(cfg.armature_scale * 5.0 / (i + 1)) : 0.f;
    // contact regulariser scale: translational inverse weight of the probe at init_qpos + element (MuJoCo body_invweight0 analogue)
    M.invw = (float)(usim_host::site_inverse_weight(chain, cfg.armature_scale) + (1.0 / 0.01 + 2.0 / (270 * 0.01)) / 3.0);
    // ---- torso lattice: top face (iy = 3) of the 9 x 4 x 11 shell, shell ids in creation order ----
    out->n_el = (cfg.torso == USIM_TORSO_TOP) ? N_TOP : (cfg.torso == USIM_TORSO_FULL ? NSH : 0);
    if (out->n_el == 0) return USIM_OK;
    if (cfg.torso == USIM_TORSO_FULL) return build_full_tables(shape, tb);
    // top face (iy = 3): element e = 11 ix + iz; its side-face neighbour below the rim, if any, is pinned (a tendon, no lattice unknown)
    std::vector<double> L((size_t)N_TOP * N_TOP, 0.0);
    const std::vector<ShellElement> sh = torso_shell(shape);
    for (int id = 0; id < NSH; ++id) {
        const ShellElement& el = sh[id];
        if (el.b != 3) continue;
        const int e = el.a * 11 + el.c;
        std::memcpy(&tb[TB_SHELL + e], &id, sizeof(int));
        for (int k = 0; k < 3; ++k) { tb[TB_POS + e * 3 + k] = el.pos[k]; tb[TB_AXIS + e * 3 + k] = el.axis[k]; }
        for (int d : {0, 1, 4, 5}) if (el.nbr[d] >= 0) L[(size_t)e * N_TOP + sh[el.nbr[d]].a * 11 + sh[el.nbr[d]].c] = -kWTen;
        L[(size_t)e * N_TOP + e] = lattice_diag(el.nn);
    }
    std::vector<double> Li = invert(L, N_TOP);
    // lattice part: laid out exactly as the kernels' workgroup-resident LDS copy
    for (int i = 0; i < N_TOP; ++i) for (int j = 0; j < N_TOP; ++j) tb[TB_LINV + (size_t)i * LROW + j] = (float)Li[(size_t)i * N_TOP + j];
    return USIM_OK;
}

// usim_config -> DevCfg, with the derived constants of the probe (probe_sdf, collide_cull) and of the torso shape
inline DevCfg translate_config(const usim_config& cfg) {
    DevCfg C{};
    C.mode = cfg.mode; C.horizon = cfg.horizon; C.early_term = cfg.early_termination; C.det_traj = cfg.deterministic_trajectory;
    C.rand_solref = cfg.torso_solref_randomization; C.rand_pos = cfg.initial_probe_pos_randomization; C.rand_fric = cfg.friction_randomization;
    C.torso_drop = cfg.torso_drop; C.pgs_iters = cfg.pgs_iters; C.ik_iters = cfg.ik_iters; C.env_offset = cfg.env_offset; C.adim = (cfg.mode == USIM_MODE_VARIABLE_Z) ? 7 : 6;
    C.key0 = (uint32_t)cfg.seed; C.key1 = (uint32_t)(cfg.seed >> 32);
    C.substeps = cfg.substeps > 1 ? cfg.substeps : 1;
    C.frictionloss = (float)cfg.joint_frictionloss;
    C.dt_ctrl = (float)cfg.control_dt; C.dt = (float)(cfg.control_dt / C.substeps); C.kp_fixed = (float)cfg.kp_fixed; C.damping_ratio = (float)cfg.damping_ratio; C.kp_min = (float)cfg.kp_min;
    C.kp_max = (float)cfg.kp_max; C.out_pos = (float)cfg.out_max_pos; C.out_ori = (float)cfg.out_max_ori; C.stiffness = (float)cfg.stiffness;
    C.damping = (float)cfg.damping; C.elem_fric = (float)cfg.elem_friction; C.probe_fric = (float)cfg.probe_friction;
    C.probe_geoms = cfg.probe_geoms == 2 ? 2 : 1; C.probe_fric2 = (float)cfg.probe_friction2;
    C.pair = (C.probe_geoms == 2 && cfg.pair_model != 0) ? 1 : 0; C.rn_scale = (C.probe_geoms == 2 && !C.pair) ? 0.5f : 1.0f;
    C.probe_r = (float)cfg.probe_radius; C.probe_hl = (float)cfg.probe_halflen; C.probe_hw = (float)cfg.probe_halfwidth; C.probe_tip = (float)cfg.probe_tip;
    {
        const double cb = (cfg.probe_radius - cfg.probe_radius2) / cfg.probe_height, ca = std::sqrt(1.0 - cb * cb);
        C.probe_r2 = (float)cfg.probe_radius2; C.probe_h = (float)cfg.probe_height; C.probe_ca = (float)ca; C.probe_cb = (float)cb;
        C.probe_cah = C.probe_ca * C.probe_h;
        { const double cr = cfg.probe_radius + cfg.probe_height + cfg.probe_halfwidth + 0.025 + 0.0075 + 1e-4; C.probe_cull2 = (float)(cr * cr); }    // (sideways sweep: triangle inequality)
        // element as a capsule, probe inside a ball of radius rp about the centre c of its upper axis: touching needs dist(c, element axis segment) <= rp + ELEM_R (DevCfg::probe_cull2c)
        {
            const double hh = std::hypot(cfg.probe_halflen, cfg.probe_halfwidth);
            const double rp = std::max(std::hypot(hh, cfg.probe_height) + cfg.probe_radius, hh + cfg.probe_radius2), cr = rp + 0.0075 + 1e-4;
            C.probe_cull2c = (float)(cr * cr);
        }
        C.probe_deep0 = (float)(cfg.probe_radius * (2.0 / 3.0)); C.probe_inv_band = (float)(1.0 / (cfg.probe_radius * (0.96 - 2.0 / 3.0)));
    }
    {
        const int shape = cfg.torso_shape ? 1 : 0;
        C.top_off = (float)kTopOff[shape]; C.y_range = (float)kYRange[shape]; C.drop = (float)(kTorsoZ[shape] - 0.0525 - 0.8);
        // usim_config.torso_drop: 0 the base stays at the spawn height (it stands on the caps of its tilted rim capsules; default since round 4), 1 free fall over the
        // spawn gap then rest (rounds 1-3), 2 at rest one gap lower from the start.  The kernels know "fall" (torso_drop) and the rest offset (drop).
        if (cfg.torso_drop == 0) C.drop = 0.f;
        C.torso_drop = cfg.torso_drop == 1 ? 1 : 0;
    }
    return C;
}

}  // namespace usim
