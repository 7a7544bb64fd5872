// usim_api.hip -- host side of the C ABI declared in include/usim.h (libusim.so).
//
// Builds the model constants in double precision (link-7 composite inertia, torso lattice tables, the inverse
// of the lattice normal matrix), owns the SoA state block in HBM and enqueues the kernels of
// usim_kernels.hip (and of usim_full.h, usim_step16.h, which it includes) on the caller's HIP stream.  No torch types, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <new>
#include <atomic>

#include "../../include/usim.h"
#include "usim_device.h"
#include "usim_robot.h"
#include "usim_kernels.hip"      // single translation unit: kernels + host launcher (no relocatable device code)
#include "usim_snapshot.h"       // usim_save_envs / usim_load_envs (behind the step kernels)


using namespace usim;

// Kernel mapping of a handle: the kernels of its step launches (MODE 0) and of its reset / refill launches (MODE 1);
// M = io.nsub > 1 || C.substeps > 1 (several physics steps per launch: every mapping but FULL).
//   mapping     handle                                                step launch                      reset / refill launch
//   FULL        full torso (lanes_per_env 0, 16, 32 or 64: ignored)   usim_step_kernel<2, 64, 0>       usim_step_kernel<2, 64, 1>
//   RIGID16     rigid torso, lanes 0 or 16 (waves_per_simd ignored)   usim_step16_kernel<0, 2, 0, M>   usim_step16_kernel<0, 2, 1, false>
//   SOFT16_W1   soft torso, lanes 16, 1 wave per SIMD                 usim_step16_kernel<1, 1, 0, M>   usim_step16_kernel<1, 2, 1, false> (not register-critical)
//   SOFT16_W2   soft torso, lanes 16, 2 waves per SIMD                usim_step16_kernel<1, 2, 0, M>   same
//   SPLIT16     soft torso, lanes 32 (split kernel, 16-lane groups)   usim_step32_kernel<M, 16>        same
//   SPLIT8      soft torso, lanes 64 (split kernel, 8-lane groups)    usim_step32_kernel<M, 8>         same
// Soft torso, lanes 0: waves_per_simd 0 the split kernel -- up to 4096 envs/GPU lanes 32 (two waves per quad of environments, 16 environments per workgroup
// = one workgroup per CU), beyond lanes 64 (two environments per DPP row, 32 per workgroup: 8192 envs still one workgroup per CU, 23.8 vs 29.3 us/step;
// profiles/r03/bench_matrix.txt) --, a nonzero waves_per_simd (a register budget) lanes 16.  Waves per SIMD: the value given, else 1 up to 4096 envs, 2 beyond.
// Refused: waves_per_simd outside 0 .. 2, any other lanes_per_env; usim_set_mapping also refuses lanes 0 and rigid / full-torso handles.
// usim_config.warm_start on a soft-torso handle: the step launch of its mapping is the instantiation with the warm start (last template argument true); the
// reset / refill launch likewise (it empties the warm rows of the environments it resets).  Rigid and full torso: no effect.
enum class Mapping : int { FULL, RIGID16, SOFT16_W1, SOFT16_W2, SPLIT16, SPLIT8 };
static bool resolve_mapping(int torso, int lanes_per_env, int waves_per_simd, int n_envs, Mapping* m) {
    if (waves_per_simd < 0 || waves_per_simd > 2) return false;
    if (torso == USIM_TORSO_NONE) { *m = Mapping::RIGID16; return lanes_per_env == 0 || lanes_per_env == 16; }
    if (lanes_per_env != 0 && lanes_per_env != 16 && lanes_per_env != 32 && lanes_per_env != 64) return false;
    const int lanes = lanes_per_env ? lanes_per_env : (waves_per_simd ? 16 : (n_envs <= 4096 ? 32 : 64));
    const int waves = waves_per_simd ? waves_per_simd : (n_envs <= 4096 ? 1 : 2);
    *m = torso == USIM_TORSO_FULL ? Mapping::FULL : lanes == 32 ? Mapping::SPLIT16 : lanes == 64 ? Mapping::SPLIT8 : (waves == 1 ? Mapping::SOFT16_W1 : Mapping::SOFT16_W2);
    return true;
}
static bool soft_torso(Mapping m) { return m != Mapping::FULL && m != Mapping::RIGID16; }
static bool multi_step(Mapping m) { return m != Mapping::FULL; }           // several control steps per launch (usim_rollout_random)

// one kernel of the table with its launch geometry (environments and threads per workgroup, dynamic LDS words; the 16-lane kernels: + the arm table behind
// everything else); model and configuration by value, or through pointers for the split kernels
struct Kernel { void (*step)(const DevModel, const DevCfg, float*, int, int, const DevIO, int, long long); void (*split)(const DevModel*, const DevCfg*, float*, int, int, const DevIO, int, long long);
                int epb, nt, lds_words; };
// acts: the launch plays a caller's action block (usim_rollout_actions, several control steps per launch): the multi-step kernel that moves io.act on between them
static Kernel kernel_of(Mapping m, int mode, bool multi, bool warm, bool acts = false) {
    if (mode != 0 && soft_torso(m)) m = Mapping::SOFT16_W2;
    const bool r = mode != 0, mu = !r && multi;
    if (mu && acts && m != Mapping::FULL) {
        Kernel k = kernel_of(m, mode, multi, warm);            // the launch geometry of the mapping's multi-step kernel
        const bool w = warm && soft_torso(m);
        switch (m) {
            case Mapping::RIGID16: k.step = usim_step16_acts_kernel<0, 2>; break;
            case Mapping::SOFT16_W1: k.step = w ? usim_step16_acts_kernel<1, 1, true> : usim_step16_acts_kernel<1, 1>; break;
            case Mapping::SOFT16_W2: k.step = w ? usim_step16_acts_kernel<1, 2, true> : usim_step16_acts_kernel<1, 2>; break;
            case Mapping::SPLIT16: k.split = w ? usim_step32_acts_kernel<16, true> : usim_step32_acts_kernel<16>; break;
            default: k.split = w ? usim_step32_acts_kernel<8, true> : usim_step32_acts_kernel<8>; break;
        }
        return k;
    }
    if (warm && soft_torso(m)) {
        constexpr int L16 = arm_lds_base<1, 0, 16>() + ARM_LDS_WORDS;
        if (r) return {usim_step16_kernel<1, 2, 1, false, true>, nullptr, 16, 256, L16};
        switch (m) {
            case Mapping::SOFT16_W1: return {mu ? usim_step16_kernel<1, 1, 0, true, true> : usim_step16_kernel<1, 1, 0, false, true>, nullptr, 16, 256, L16};
            case Mapping::SOFT16_W2: return {mu ? usim_step16_kernel<1, 2, 0, true, true> : usim_step16_kernel<1, 2, 0, false, true>, nullptr, 16, 256, L16};
            case Mapping::SPLIT16: return {nullptr, mu ? usim_step32_kernel<true, 16, true> : usim_step32_kernel<false, 16, true>, 4 * wpr<16>(), 128 * wpr<16>(), arm_lds_base<1, 1, 16>() + ARM_LDS_WORDS};
            default: return {nullptr, mu ? usim_step32_kernel<true, 8, true> : usim_step32_kernel<false, 8, true>, 8 * wpr<8>(), 128 * wpr<8>(), arm_lds_base<1, 1, 8>() + ARM_LDS_WORDS};
        }
    }
    constexpr int L16 = arm_lds_base<1, 0, 16>() + ARM_LDS_WORDS;
    switch (m) {
        case Mapping::FULL: return {r ? usim_step_kernel<2, 64, 1> : usim_step_kernel<2, 64, 0>, nullptr, FULL_EPB, FULL_NT, FULL_LDS_WORDS};
        case Mapping::RIGID16: return {r ? usim_step16_kernel<0, 2, 1, false> : mu ? usim_step16_kernel<0, 2, 0, true> : usim_step16_kernel<0, 2, 0, false>, nullptr, 16, 256, arm_lds_base<0, 0, 16>() + ARM_LDS_WORDS};
        case Mapping::SOFT16_W1: return {mu ? usim_step16_kernel<1, 1, 0, true> : usim_step16_kernel<1, 1, 0, false>, nullptr, 16, 256, L16};
        case Mapping::SOFT16_W2: return {r ? usim_step16_kernel<1, 2, 1, false> : mu ? usim_step16_kernel<1, 2, 0, true> : usim_step16_kernel<1, 2, 0, false>, nullptr, 16, 256, L16};
        case Mapping::SPLIT16: return {nullptr, mu ? usim_step32_kernel<true, 16> : usim_step32_kernel<false, 16>, 4 * wpr<16>(), 128 * wpr<16>(), arm_lds_base<1, 1, 16>() + ARM_LDS_WORDS};
        case Mapping::SPLIT8: return {nullptr, mu ? usim_step32_kernel<true, 8> : usim_step32_kernel<false, 8>, 8 * wpr<8>(), 128 * wpr<8>(), arm_lds_base<1, 1, 8>() + ARM_LDS_WORDS};
    }
    return {};
}

struct usim_handle {
    usim_config cfg;
    Mapping map = Mapping::RIGID16;   // resolved by usim_create (resolve_mapping)
    int n = 0, npad = 0, device = 0, adim = 6, n_el = 0, nfields = 0;
    DevModel M;
    DevCfg C;
    float* state = nullptr;
    float* d_tables = nullptr;        // lattice table block of this handle (DevModel::tables)
    void* d_consts = nullptr;         // device copy of M and C (the split kernels read them through pointers: scalar loads instead of ~110 kernel-argument dwords)
    const DevModel* d_M = nullptr; const DevCfg* d_C = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // device time of the reset-bank refill launches (usim_refill_time): a ring of event pairs, read lazily
    static constexpr int RF_RING = 8;
    hipEvent_t rf0[RF_RING] = {}, rf1[RF_RING] = {};
    bool rf_live[RF_RING] = {};
    int rf_next = 0;
    double rf_total_ms = 0.0;
    long long rf_count = 0;
    // reset bank machinery
    int2* d_items = nullptr;          // refill work list, capacity 2 * n * BANK_DEPTH
    int* d_count = nullptr;           // [0] items, [1] finished workgroups of the running refill
    long long steps_since_refill = 0;
    int steps_per_launch = 256;      // usim_rollout_random: consecutive steps per launch of the 16-lane kernels (USIM_STEPS_PER_LAUNCH overrides, 1 .. MAX_STEPS_PER_LAUNCH)
    int bank_row0 = 0;
    bool warm = false;                // warm start of the top-face contact solve: warm rows behind the reset bank, the step / reset kernels that use them (kernel_of)
    std::string hip_err;
};

// every entry point runs on the handle's device and restores the caller's current device afterwards
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess); }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

#define HIPCHK(h, call)                                                                                     \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            (h)->hip_err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
            return USIM_ERR_HIP;                                                                            \
        }                                                                                                   \
    } while (0)

// ---------------------------------------------------------------------------------------------------------
// model data (the Panda chain constants themselves live in usim_kernels.hip)
// ---------------------------------------------------------------------------------------------------------
namespace {
const double kPi = 3.14159265358979323846;
const double kGoalQuat[4] = {-0.69192486, 0.72186726, -0.00514253, -0.01100909};   // ultrasound.py:174 (x,y,z,w)
const double kBase[3] = {-0.56, 0.0, 0.913};                                         // ultrasound.py:279-280 + mount height
// torso spawn height = table 0.8 + z_offset 0.005 - bottom_site z (ultrasound.py:146,313): box -0.0522 (soft_box.xml:14), cylinder
// -0.05 (soft_human_torso.xml:14); trajectory height / waypoint grid width per shape (ultrasound.py:184,186)
const double kTorsoZ[2] = {0.8 + 0.005 + 0.0522, 0.8 + 0.005 + 0.05};
const double kTopOff[2] = {0.039, 0.041}, kYRange[2] = {0.09, 0.05};
const double kProbePos[3] = {-0.004, -0.063, 0.128};                                 // ultrasound_probe_gripper.xml:6
const double kProbeCom[3] = {0.0013, 0.021, -0.043};                                 // stand-in (mesh missing from the snapshot)
const double kProbeI[3] = {1.6e-3, 1.6e-3, 2.0e-4};

void pack_sym(const double I[3][3], float* o) { o[0] = (float)I[0][0]; o[1] = (float)I[0][1]; o[2] = (float)I[0][2]; o[3] = (float)I[1][1]; o[4] = (float)I[1][2]; o[5] = (float)I[2][2]; }

bool on_shell(int a, int b, int c) {
    if (a < 0 || a >= 9 || b < 0 || b >= 4 || c < 0 || c >= 11) return false;
    return a == 0 || a == 8 || b == 0 || b == 3 || c == 0 || c == 10;
}

// soft equality constraints of the lattice (composite solrefsmooth, d_max 0.95): weight of the pin to the rest position and of a tendon to a neighbour
const double kDMax = 0.95, kWFix = kDMax / (1 - kDMax), kWTen = 0.5 * kDMax / (1 - kDMax);
double lattice_diag(int nn) { return 1.0 + kWFix + kWTen * nn; }      // diagonal of the lattice Laplacian: an element with nn tendons

// one element of the 9 x 4 x 11 torso shell (soft_box.xml:9): lattice cell, world-axes position and slide axis (float, as uploaded), the shell ids
// of its 6-neighbourhood (x-, x+, y-, y+, z-, z+; -1 off the shell) and their number
struct ShellElement { int a, b, c; float pos[3], axis[3]; int nbr[6], nn; };

// the 270 shell elements in creation order (ix outer, iy, iz inner: the index is the shell id)
std::vector<ShellElement> torso_shell(int shape) {
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
std::vector<double> invert(std::vector<double> a, int n) {
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
}  // namespace

// per-handle copy of the table block (synchronous: complete before usim_create returns, so no stream of the caller can race with it)
static int upload_tables(usim_handle* h, const std::vector<float>& tb) {
    HIPCHK(h, hipMalloc(&h->d_tables, tb.size() * sizeof(float)));
    HIPCHK(h, hipMemcpy(h->d_tables, tb.data(), tb.size() * sizeof(float), hipMemcpyHostToDevice));
    h->M.tables = h->d_tables;
    return USIM_OK;
}

// Arm table of the 16-lane kernels (usim_device.h ArmTable) from the z-aligned chain: lanes 0 .. 6 the links (padding links of a shorter
// chain: identity transform, no mass, no joint), lane 7 the end-effector site as a fixed child of the last link.
static void build_arm_table(const usim_host::Chain& c, float* tb, const double armature_scale) {
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
static int build_full_tables(usim_handle* h, int shape) {
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
    return upload_tables(h, tb);
}

static int build_model(usim_handle* h) {
    DevModel& M = h->M;
    std::memset(&M, 0, sizeof M);
    // robot chain (z-aligned, end effector folded into the last link): arm table + the end-effector constants of the kernels
    const usim_host::RobotDesc desc = (h->cfg.robot == USIM_ROBOT_UR5E) ? usim_host::ur5e_desc() : usim_host::panda_desc();
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
    const int shape = h->cfg.torso_shape ? 1 : 0;
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
    std::vector<float> tb(TB_TOTAL, 0.f);
    build_arm_table(chain, &tb[TB_ARM], h->cfg.armature_scale);
    for (int i = 0; i < NJ; ++i) M.armature[i] = chain.link[i].joint ? (float)(h->cfg.armature_scale * 5.0 / (i + 1)) : 0.f;
    // contact regulariser scale: translational inverse weight of the probe at init_qpos + element (MuJoCo body_invweight0 analogue)
    M.invw = (float)(usim_host::site_inverse_weight(chain, h->cfg.armature_scale) + (1.0 / 0.01 + 2.0 / (270 * 0.01)) / 3.0);
    // ---- torso lattice: top face (iy = 3) of the 9 x 4 x 11 shell, shell ids in creation order ----
    h->n_el = (h->cfg.torso == USIM_TORSO_TOP) ? N_TOP : (h->cfg.torso == USIM_TORSO_FULL ? NSH : 0);
    if (h->n_el == 0) return upload_tables(h, tb);
    if (h->cfg.torso == USIM_TORSO_FULL) return build_full_tables(h, shape);
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
    return upload_tables(h, tb);
}

// dynamic LDS limit of every kernel the handle can launch: those of its mapping, for a soft-torso handle those of every soft-torso mapping (usim_set_mapping)
static int set_lds_limits(usim_handle* h) {
    for (int m = 0; m <= (int)Mapping::SPLIT8; ++m)
        if ((Mapping)m == h->map || (soft_torso((Mapping)m) && soft_torso(h->map)))
            for (int i = 0; i < 5; ++i) {                        // (step, reset) x (single, multi-step), then the multi-step kernel of usim_rollout_actions
                const Kernel k = i < 4 ? kernel_of((Mapping)m, i & 1, i >> 1, h->warm) : kernel_of((Mapping)m, 0, true, h->warm, true);
                HIPCHK(h, hipFuncSetAttribute(k.step ? (const void*)k.step : (const void*)k.split, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_words * (int)sizeof(float)));
            }
    return USIM_OK;
}

// every environment's warm rows to "nothing kept" (synchronous)
static int warm_rows_reset(usim_handle* h) {
    std::vector<float> w((size_t)WARM_WORDS * h->npad, 0.f);
    const int none = -1;
    for (int i = 0; i < h->npad; ++i) for (int k = 0; k < MAXC; ++k) std::memcpy(&w[(size_t)i * WARM_WORDS + WARM_EL + k], &none, 4);
    HIPCHK(h, hipMemcpy(h->state + warm_index(h->bank_row0, h->npad, 0), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    return USIM_OK;
}

template <int MODE>
static int launch(usim_handle* h, DevIO io, int flags, long long rstep, hipStream_t s) {
    io.bank_row0 = h->bank_row0;
    const Kernel k = kernel_of(h->map, MODE, io.nsub > 1 || h->C.substeps > 1, h->warm, io.nsub > 1 && io.act);
    const dim3 grid((h->n + k.epb - 1) / k.epb), block(k.nt);
    const size_t lds = (size_t)k.lds_words * sizeof(float);
    if (k.step) hipLaunchKernelGGL(k.step, grid, block, lds, s, h->M, h->C, h->state, h->n, h->npad, io, flags, rstep);
    else hipLaunchKernelGGL(k.split, grid, block, lds, s, h->d_M, h->d_C, h->state, h->n, h->npad, io, flags, rstep);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->hip_err = std::string("usim_step_kernel launch: ") + hipGetErrorString(e); return USIM_ERR_HIP; }
    return USIM_OK;
}

extern "C" {

int usim_default_config(usim_config* c) {
    if (!c || c->struct_size != (int32_t)sizeof(usim_config)) return USIM_ERR_INVALID;   // nothing is written to a struct of another layout
    std::memset(c, 0, sizeof *c);
    c->mode = USIM_MODE_TRACKING; c->torso = USIM_TORSO_TOP; c->horizon = 1000; c->early_termination = 1;
    c->deterministic_trajectory = 0; c->torso_solref_randomization = 1; c->initial_probe_pos_randomization = 1;
    c->friction_randomization = 0; c->torso_drop = 0; c->pgs_iters = 24; c->ik_iters = 5; c->env_offset = 0; c->lanes_per_env = 0; c->torso_shape = 0; c->waves_per_simd = 0; c->robot = 0; c->seed = 3;
    c->control_dt = 0.002; c->substeps = 1; c->kp_fixed = 300; c->damping_ratio = 1; c->kp_min = 0; c->kp_max = 500; c->out_max_pos = 0.05; c->out_max_ori = 0.5;
    c->stiffness = 1324.17; c->damping = 17.59; c->elem_friction = 0.01; c->probe_friction = 1e-4; c->probe_friction2 = 1.0; c->probe_geoms = 2; c->probe_radius = 0.021; c->probe_halflen = 0.0065;
    c->pair_model = 1; c->probe_radius2 = 0.035; c->probe_height = 0.020; c->probe_halfwidth = 0.0; c->probe_tip = -0.0005;      // round-4 fit, kept in round 5 (oracle: PROBE_*; profiles/r04/probe_fit.txt, profiles/r05/probe_fit.txt)
    c->armature_scale = 1.0; c->joint_frictionloss = 0.1;                 // robosuite's defaults for robot joints (include/usim.h)
    c->struct_size = (int32_t)sizeof(usim_config);
    return USIM_OK;
}

int usim_create(const usim_config* cfg, int n_envs, int device, usim_handle** out) {
    if (!cfg || !out || n_envs <= 0) return USIM_ERR_INVALID;
    if (cfg->struct_size != (int32_t)sizeof(usim_config)) return USIM_ERR_INVALID;     // built against another layout of include/usim.h
    if (cfg->probe_radius2 <= 0 || !(cfg->probe_height > std::fabs(cfg->probe_radius2 - cfg->probe_radius))) return USIM_ERR_INVALID;
    if (!(cfg->probe_halfwidth >= 0) || !(std::fabs(cfg->probe_tip) <= 0.02) || cfg->torso_drop < 0 || cfg->torso_drop > 2) return USIM_ERR_INVALID;
    if (cfg->mode < 0 || cfg->mode > 3 || cfg->torso < 0 || cfg->torso > 2 || !(cfg->armature_scale >= 0) || !(cfg->joint_frictionloss >= 0) || cfg->horizon <= 0 || cfg->control_dt <= 0 ||
        cfg->probe_halflen < 1e-4 || cfg->probe_radius <= 0 || cfg->pgs_iters < 0 || cfg->ik_iters < 0 || cfg->torso_shape < 0 ||
        cfg->torso_shape > 1 || cfg->waves_per_simd < 0 || cfg->waves_per_simd > 2 || cfg->robot < 0 || cfg->robot > 1 || cfg->warm_start < 0 || cfg->warm_start > 1) return USIM_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return USIM_ERR_NO_DEVICE;
    usim_handle* h = new (std::nothrow) usim_handle();
    if (!h) return USIM_ERR_ALLOC;
    *out = h;                       // returned even on failure so that usim_last_hip_error can be read; caller destroys
    h->cfg = *cfg; h->n = n_envs; h->npad = (n_envs + WG - 1) / WG * WG; h->device = device;
    h->adim = (cfg->mode == USIM_MODE_VARIABLE_Z) ? 7 : 6;
    DeviceGuard guard(device);
    int rc = build_model(h);
    if (rc != USIM_OK) return rc;
    DevCfg& C = h->C;
    C.mode = cfg->mode; C.horizon = cfg->horizon; C.early_term = cfg->early_termination; C.det_traj = cfg->deterministic_trajectory;
    C.rand_solref = cfg->torso_solref_randomization; C.rand_pos = cfg->initial_probe_pos_randomization; C.rand_fric = cfg->friction_randomization;
    C.torso_drop = cfg->torso_drop; C.pgs_iters = cfg->pgs_iters; C.ik_iters = cfg->ik_iters; C.env_offset = cfg->env_offset; C.adim = h->adim;
    C.key0 = (uint32_t)cfg->seed; C.key1 = (uint32_t)(cfg->seed >> 32);
    C.substeps = cfg->substeps > 1 ? cfg->substeps : 1;
    C.frictionloss = (float)cfg->joint_frictionloss;
    // warm start of the top-face contact solve (the rigid torso has no contact solve, the full torso is always warm: accepted, no effect).  USIM_WARM_START = 0 / 1
    // replaces the field, so that a fixed command line (bench.py) can time both; the handle's recorded configuration follows it
    if (const char* ws = std::getenv("USIM_WARM_START")) { if ((ws[0] == '0' || ws[0] == '1') && ws[1] == 0) h->cfg.warm_start = ws[0] - '0'; }
    h->warm = h->cfg.warm_start != 0 && cfg->torso == USIM_TORSO_TOP;
    C.dt_ctrl = (float)cfg->control_dt; C.dt = (float)(cfg->control_dt / C.substeps); C.kp_fixed = (float)cfg->kp_fixed; C.damping_ratio = (float)cfg->damping_ratio; C.kp_min = (float)cfg->kp_min;
    C.kp_max = (float)cfg->kp_max; C.out_pos = (float)cfg->out_max_pos; C.out_ori = (float)cfg->out_max_ori; C.stiffness = (float)cfg->stiffness;
    C.damping = (float)cfg->damping; C.elem_fric = (float)cfg->elem_friction; C.probe_fric = (float)cfg->probe_friction;
    C.probe_geoms = cfg->probe_geoms == 2 ? 2 : 1; C.probe_fric2 = (float)cfg->probe_friction2;
    C.pair = (C.probe_geoms == 2 && cfg->pair_model != 0) ? 1 : 0; C.rn_scale = (C.probe_geoms == 2 && !C.pair) ? 0.5f : 1.0f;
    C.probe_r = (float)cfg->probe_radius; C.probe_hl = (float)cfg->probe_halflen; C.probe_hw = (float)cfg->probe_halfwidth; C.probe_tip = (float)cfg->probe_tip;
    {
        const double cb = (cfg->probe_radius - cfg->probe_radius2) / cfg->probe_height, ca = std::sqrt(1.0 - cb * cb);
        C.probe_r2 = (float)cfg->probe_radius2; C.probe_h = (float)cfg->probe_height; C.probe_ca = (float)ca; C.probe_cb = (float)cb;
        C.probe_cah = C.probe_ca * C.probe_h;
        { const double cr = cfg->probe_radius + cfg->probe_height + cfg->probe_halfwidth + 0.025 + 0.0075 + 1e-4; C.probe_cull2 = (float)(cr * cr); }    // (sideways sweep: triangle inequality)
        C.probe_deep0 = (float)(cfg->probe_radius * (2.0 / 3.0)); C.probe_inv_band = (float)(1.0 / (cfg->probe_radius * (0.96 - 2.0 / 3.0)));
    }
    {
        const int shape = cfg->torso_shape ? 1 : 0;
        C.top_off = (float)kTopOff[shape]; C.y_range = (float)kYRange[shape]; C.drop = (float)(kTorsoZ[shape] - 0.0525 - 0.8);
        // usim_config.torso_drop: 0 the base stays at the spawn height (it stands on the caps of its tilted rim capsules; default since round 4), 1 free fall over the
        // spawn gap then rest (rounds 1-3), 2 at rest one gap lower from the start.  The kernels know "fall" (torso_drop) and the rest offset (drop).
        if (cfg->torso_drop == 0) C.drop = 0.f;
        C.torso_drop = cfg->torso_drop == 1 ? 1 : 0;
    }
    {
        // device copy of the model and the configuration (both final here; build_model has set M.tables)
        const size_t offC = (sizeof(DevModel) + 255) / 256 * 256;
        HIPCHK(h, hipMalloc(&h->d_consts, offC + sizeof(DevCfg)));
        HIPCHK(h, hipMemcpy(h->d_consts, &h->M, sizeof(DevModel), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(static_cast<char*>(h->d_consts) + offC, &h->C, sizeof(DevCfg), hipMemcpyHostToDevice));
        h->d_M = static_cast<const DevModel*>(h->d_consts); h->d_C = reinterpret_cast<const DevCfg*>(static_cast<const char*>(h->d_consts) + offC);
    }
    if (const char* spl = std::getenv("USIM_STEPS_PER_LAUNCH")) { const int v = std::atoi(spl); if (v >= 1 && v <= MAX_STEPS_PER_LAUNCH) h->steps_per_launch = v; }
    h->nfields = (cfg->torso == USIM_TORSO_FULL) ? F_TOTAL_FULL : (h->n_el ? F_TOTAL_TOP : F_NSCALAR);
    h->bank_row0 = h->nfields;                                  // two reset-bank slots follow the live state rows
    size_t bytes = (size_t)(h->nfields + BANK_ROWS) * h->npad * sizeof(float);
    const size_t warm_bytes = h->warm ? (size_t)WARM_WORDS * h->npad * sizeof(float) : 0;      // warm rows behind the bank (usim_device.h warm_index)
    HIPCHK(h, hipMalloc(&h->state, bytes + warm_bytes));
    HIPCHK(h, hipMemset(h->state, 0, bytes + warm_bytes));
    if (h->warm) { int rc2 = warm_rows_reset(h); if (rc2) return rc2; }
    HIPCHK(h, hipMalloc(&h->d_items, 2 * (size_t)h->n * BANK_DEPTH * sizeof(int2)));
    HIPCHK(h, hipMalloc(&h->d_count, 2 * sizeof(int)));
    HIPCHK(h, hipMemset(h->d_count, 0, 2 * sizeof(int)));
    HIPCHK(h, hipEventCreate(&h->ev0));
    HIPCHK(h, hipEventCreate(&h->ev1));
    for (int i = 0; i < usim_handle::RF_RING; ++i) { HIPCHK(h, hipEventCreate(&h->rf0[i])); HIPCHK(h, hipEventCreate(&h->rf1[i])); }
    if (!resolve_mapping(cfg->torso, cfg->lanes_per_env, cfg->waves_per_simd, n_envs, &h->map)) return USIM_ERR_INVALID;
    // the full torso runs one mapping: a wave per environment, the Panda's constants, one physics step per control step, one step per launch
    if (h->map == Mapping::FULL && (cfg->robot != USIM_ROBOT_PANDA || C.substeps > 1)) { h->hip_err = "torso = USIM_TORSO_FULL: Panda, substeps = 1"; return USIM_ERR_UNSUPPORTED; }
    return set_lds_limits(h);
}

void usim_destroy(usim_handle* h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    if (h->state) (void)hipFree(h->state);
    if (h->d_tables) (void)hipFree(h->d_tables);
    if (h->d_consts) (void)hipFree(h->d_consts);
    if (h->d_items) (void)hipFree(h->d_items);
    if (h->d_count) (void)hipFree(h->d_count);

    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (int i = 0; i < usim_handle::RF_RING; ++i) { if (h->rf0[i]) (void)hipEventDestroy(h->rf0[i]); if (h->rf1[i]) (void)hipEventDestroy(h->rf1[i]); }
    delete h;
}

int usim_set_mapping(usim_handle* h, int lanes_per_env, int waves_per_simd) {
    if (!h || !soft_torso(h->map) || lanes_per_env == 0) return USIM_ERR_INVALID;
    return resolve_mapping(h->cfg.torso, lanes_per_env, waves_per_simd, h->n, &h->map) ? USIM_OK : USIM_ERR_INVALID;
}

int usim_set_steps_per_launch(usim_handle* h, int steps) {
    if (!h || steps < 1 || steps > MAX_STEPS_PER_LAUNCH) return USIM_ERR_INVALID;
    h->steps_per_launch = steps;
    return USIM_OK;
}

int usim_get_steps_per_launch(const usim_handle* h) { return h ? h->steps_per_launch : USIM_ERR_INVALID; }

static void refill_collect(usim_handle* h, int slot);

int usim_refill_time(usim_handle* h, double* total_ms, long long* launches) {
    if (!h || !total_ms || !launches) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    for (int i = 0; i < usim_handle::RF_RING; ++i) refill_collect(h, i);         // blocks until the recorded refill launches have finished
    *total_ms = h->rf_total_ms; *launches = h->rf_count;
    return USIM_OK;
}

int usim_num_envs(const usim_handle* h) { return h ? h->n : USIM_ERR_INVALID; }
int usim_action_dim(const usim_handle* h) { return h ? h->adim : USIM_ERR_INVALID; }
int usim_num_elements(const usim_handle* h) { return h ? h->n_el : USIM_ERR_INVALID; }
int usim_has_warm_start(const usim_handle* h) { return h ? (h->warm ? 1 : 0) : USIM_ERR_INVALID; }

// compute every episode on the refill work list into the reset bank (grid-stride over the list, one launch)
static void refill_collect(usim_handle* h, int slot) {
    if (!h->rf_live[slot]) return;
    float ms = 0.f;
    if (hipEventSynchronize(h->rf1[slot]) == hipSuccess && hipEventElapsedTime(&ms, h->rf0[slot], h->rf1[slot]) == hipSuccess) { h->rf_total_ms += ms; h->rf_count += 1; }
    h->rf_live[slot] = false;
}
static int bank_refill(usim_handle* h, hipStream_t s) {
    DevIO b{}; b.items = h->d_items; b.count = h->d_count; b.refill = 1;
    h->steps_since_refill = 0;
    // a stream that is being captured into a graph (policy.GraphedCollector: the whole rollout loop as one hipGraph) takes the launch only: no
    // event bookkeeping, no synchronising call
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return launch<1>(h, b, 0, 0, s);
    const int slot = h->rf_next;
    h->rf_next = (slot + 1) % usim_handle::RF_RING;
    refill_collect(h, slot);                          // (a pair that is reused was recorded RF_RING refills = 512 steps ago: long finished)
    const bool timed = h->rf0[slot] && h->rf1[slot] && hipEventRecord(h->rf0[slot], s) == hipSuccess;
    const int rc = launch<1>(h, b, 0, 0, s);
    if (timed && rc == USIM_OK && hipEventRecord(h->rf1[slot], s) == hipSuccess) h->rf_live[slot] = true;
    return rc;
}

// order episodes +1..+BANK_DEPTH for the selected environments and compute them
static int bank_fill(usim_handle* h, const uint8_t* mask_dev, hipStream_t s) {
    const int total = h->n * BANK_DEPTH;
    hipLaunchKernelGGL(usim_bank_items_kernel, dim3((total + 255) / 256), dim3(256), 0, s, h->state, h->n, mask_dev, h->d_items, h->d_count);
    HIPCHK(h, hipGetLastError());
    return bank_refill(h, s);
}

// direct reset of the selected environments followed by the fill of their bank rings, all on `stream`
static int reset_common(usim_handle* h, const uint8_t* mask_dev, const float* params_dev, float* obs_dev, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    DevIO io{}; io.mask = mask_dev; io.obs = obs_dev; io.reset_params = params_dev; io.refill = 0;
    int rc = launch<1>(h, io, 0, 0, s);
    if (rc) return rc;
    return bank_fill(h, mask_dev, s);
}

int usim_reset(usim_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream) {
    if (!h) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    return reset_common(h, mask_dev, nullptr, obs_dev, stream);
}

int usim_reset_explicit(usim_handle* h, const uint8_t* mask_dev, const float* params_dev, float* obs_dev, void* stream) {
    if (!h || !params_dev) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    return reset_common(h, mask_dev, params_dev, obs_dev, stream);
}

static int fill_io(const usim_step_io* s, DevIO& io, bool need_act) {
    if (!s || !s->obs_dev || !s->rew_dev || !s->done_dev || (need_act && !s->act_dev)) return USIM_ERR_INVALID;
    io = DevIO{};
    io.act = s->act_dev; io.obs = s->obs_dev; io.rew = s->rew_dev; io.done = s->done_dev; io.term_obs = s->term_obs_dev;
    io.contacts = s->contacts_dev; io.ep_ret = s->ep_return_dev; io.ep_len = s->ep_length_dev; io.act_out = s->act_out_dev; io.log = s->log_dev; io.status_out = s->status_dev;
    return USIM_OK;
}

// One step on `stream`.  A finished environment adopts its next episode from the reset bank inside the step kernel (a copy
// of 38 words) and orders the episode that will reuse the slot.  An environment consumes at most one slot per step, so a
// refill launch every BANK_DEPTH steps keeps every ring valid by construction; in that launch the initial-pose IK and the
// zero-torque forward pass of all environments that finished during the period run side by side.
static int step_common(usim_handle* h, DevIO io, int flags, long long rstep, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & LF_AUTO_RESET)) return launch<0>(h, io, flags, rstep, s);
    io.items = h->d_items; io.count = h->d_count;
    int rc = launch<0>(h, io, flags, rstep, s);
    if (rc) return rc;
    if (++h->steps_since_refill >= BANK_DEPTH) rc = bank_refill(h, s);
    return rc;
}

int usim_step(usim_handle* h, const usim_step_io* s, int auto_reset, void* stream) {
    if (!h) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    DevIO io; int rc = fill_io(s, io, true);
    if (rc) return rc;
    return step_common(h, io, auto_reset ? LF_AUTO_RESET : 0, 0, stream);
}

int usim_refill_bank(usim_handle* h, void* stream) {
    if (!h) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    return bank_refill(h, (hipStream_t)stream);
}

int usim_random_actions(usim_handle* h, int64_t step, float* act_dev, void* stream) {
    if (!h || !act_dev) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    hipLaunchKernelGGL(usim_random_actions_kernel, dim3((h->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->C, h->n, (long long)step, act_dev);
    HIPCHK(h, hipGetLastError());
    return USIM_OK;
}

// nsteps consecutive auto-reset steps in multi-step launches (usim_rollout_random, usim_rollout_actions; `flags` and io.act are all that differs between them).
// The 16-lane kernels run up to h->steps_per_launch consecutive steps per launch (usim_step16.h step16_body); a launch never crosses the refill period of the
// reset bank (an environment consumes at most one ring slot per step).  io.act, where there is one, is an action block [nsteps][n][A]: inside a launch the kernel
// moves it on from control step to control step (kernel_of acts), between launches this loop does -- whether or not the outputs are blocks (block_advance).
static int rollout_common(usim_handle* h, DevIO io, int flags, long long first_step, int nsteps, int block_advance, void* stream) {
    const int kmax = multi_step(h->map) ? h->steps_per_launch : 1;
    for (int k = 0; k < nsteps;) {
        int kk = nsteps - k < kmax ? nsteps - k : kmax;
        if (kk > BANK_DEPTH - (int)h->steps_since_refill) kk = BANK_DEPTH - (int)h->steps_since_refill;
        io.nsub = kk; io.block = block_advance ? 1 : 0;
        h->steps_since_refill += kk - 1;                      // (step_common counts the launch as one step)
        const int rc = step_common(h, io, flags, first_step + k, stream);
        if (rc) return rc;
        k += kk;
        if (block_advance) advance_rollout_block(io, (size_t)h->n * kk, h->adim);
        if (io.act) io.act += (size_t)h->n * kk * h->adim;
    }
    return USIM_OK;
}

int usim_rollout_random(usim_handle* h, int64_t first_step, int nsteps, const usim_step_io* s, int block_advance, void* stream) {
    if (!h || nsteps < 0) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    DevIO io; int rc = fill_io(s, io, false);
    if (rc) return rc;
    io.act = nullptr;
    return rollout_common(h, io, LF_AUTO_RESET | LF_RANDOM_ACT, (long long)first_step, nsteps, block_advance, stream);
}

int usim_rollout_actions(usim_handle* h, int nsteps, const usim_step_io* s, int block_advance, void* stream) {
    if (!h || nsteps < 0) return USIM_ERR_INVALID;
    DevIO io; int rc = fill_io(s, io, true);                  // (io->act_dev required; nothing is enqueued on a refusal)
    if (rc) return rc;
    if (nsteps == 0) return USIM_OK;
    DeviceGuard guard(h->device);
    io.act_out = nullptr;                                     // nothing is drawn: the block's own action entry, if any, is not written
    return rollout_common(h, io, LF_AUTO_RESET, 0, nsteps, block_advance, stream);
}

int usim_time_steps(usim_handle* h, int64_t first_step, int nsteps, const usim_step_io* s, int block_advance, void* stream, float* elapsed_ms) {
    if (!h || !elapsed_ms) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(h, hipEventRecord(h->ev0, st));
    int rc = usim_rollout_random(h, first_step, nsteps, s, block_advance, stream);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev1, st));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return USIM_OK;
}

static inline size_t lat_words(const usim_handle* h) { return h->cfg.torso == USIM_TORSO_FULL ? LATF_ENV_WORDS : LAT_ENV_WORDS; }
static inline size_t lat_s(const usim_handle* h) { return h->cfg.torso == USIM_TORSO_FULL ? LATF_S : LAT_S; }
static inline size_t lat_sd(const usim_handle* h) { return h->cfg.torso == USIM_TORSO_FULL ? LATF_SD : LAT_SD; }

// full torso: per environment USIM_FULL_BODY_WORDS float64 -- pose and velocity of the free body (13: position (world), quaternion w x y z, linear velocity (world), angular
// velocity (body frame)), then the warm start of the contact solve (LATF_WARM_WORDS: every element's table-contact force and multiplier, the probe slots' elements as numbers and
// forces).  float64 because the device holds the position relative to the robot base in float32: base + position is exact in float64, so get -> set restores the bits.
constexpr int FULL_BODY_WORDS = 13 + LATF_WARM_WORDS;
static_assert(FULL_BODY_WORDS == USIM_FULL_BODY_WORDS, "include/usim.h");
int usim_get_body_state(usim_handle* h, double* body) {
    if (!h || !body || h->cfg.torso != USIM_TORSO_FULL) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<float> buf((size_t)LATF_ENV_WORDS * h->npad);
    HIPCHK(h, hipMemcpy(buf.data(), h->state + (size_t)F_LAT * h->npad, buf.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->n; ++i) {
        const float* e = &buf[(size_t)i * LATF_ENV_WORDS];
        double* o = body + (size_t)i * FULL_BODY_WORDS;
        for (int a = 0; a < 13; ++a) o[a] = (double)e[LATF_BODY + a] + (a < 3 ? (double)h->M.base[a] : 0.0);
        for (int w = 0; w < LATF_WARM_WORDS; ++w) {
            if (w >= 4 * NSH && w < 4 * NSH + 8) { int v; std::memcpy(&v, &e[LATF_WTAB + w], 4); o[13 + w] = (double)v; }      // element numbers of the probe slots
            else o[13 + w] = (double)e[LATF_WTAB + w];
        }
    }
    return USIM_OK;
}
int usim_set_body_state(usim_handle* h, const double* body) {
    if (!h || !body || h->cfg.torso != USIM_TORSO_FULL) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<float> bw(13 + LATF_WARM_WORDS);
    for (int i = 0; i < h->n; ++i) {
        const double* o = body + (size_t)i * FULL_BODY_WORDS;
        for (int a = 0; a < 13; ++a) bw[a] = (float)(o[a] - (a < 3 ? (double)h->M.base[a] : 0.0));
        for (int w = 0; w < LATF_WARM_WORDS; ++w) {
            if (w >= 4 * NSH && w < 4 * NSH + 8) { const int v = (int)o[13 + w]; std::memcpy(&bw[13 + w], &v, 4); }
            else bw[13 + w] = (float)o[13 + w];
        }
        float* dst = h->state + (size_t)F_LAT * h->npad + (size_t)i * LATF_ENV_WORDS;
        HIPCHK(h, hipMemcpy(dst + LATF_BODY, bw.data(), 13 * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(dst + LATF_WTAB, bw.data() + 13, (size_t)LATF_WARM_WORDS * sizeof(float), hipMemcpyHostToDevice));
    }
    return USIM_OK;
}

// soft top-face torso with usim_config.warm_start: the kept contact list of the solver, [n][USIM_WARM_WORDS] float32 (the device's warm rows with the elements as numbers)
static_assert(WARM_WORDS == USIM_WARM_WORDS, "include/usim.h");
int usim_get_warm_start(usim_handle* h, float* w) {
    if (!h || !w || !h->warm) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(w, h->state + warm_index(h->bank_row0, h->npad, 0), (size_t)WARM_WORDS * h->n * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->n; ++i) for (int k = 0; k < MAXC; ++k) {
        float* p = &w[(size_t)i * WARM_WORDS + WARM_EL + k];
        int v; std::memcpy(&v, p, 4); *p = (float)v;
    }
    return USIM_OK;
}
int usim_set_warm_start(usim_handle* h, const float* w) {
    if (!h || !w || !h->warm) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<float> buf(w, w + (size_t)WARM_WORDS * h->n);
    for (int i = 0; i < h->n; ++i) for (int k = 0; k < MAXC; ++k) {
        float* p = &buf[(size_t)i * WARM_WORDS + WARM_EL + k];
        const int v = (*p >= 0.f && *p < (float)N_TOP) ? (int)*p : -1;       // (an element number the kernels can compare; anything else: empty slot)
        std::memcpy(p, &v, 4);
    }
    HIPCHK(h, hipMemcpy(h->state + warm_index(h->bank_row0, h->npad, 0), buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
    return USIM_OK;
}

int usim_get_state(usim_handle* h, float* scalars, float* lattice) {
    if (!h || !scalars) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<float> buf((size_t)h->nfields * h->npad);
    HIPCHK(h, hipMemcpy(buf.data(), h->state, buf.size() * sizeof(float), hipMemcpyDeviceToHost));
    const int int_fields[4] = {F_T, F_TOUCH, F_EPISODE, F_STATUS};
    for (int i = 0; i < h->n; ++i) {
        for (int f = 0; f < F_NSCALAR; ++f) scalars[(size_t)i * USIM_NSCALAR + f] = buf[scalar_index(f, i)];
        for (int j = 0; j < NJ; ++j) scalars[(size_t)i * USIM_NSCALAR + F_Q + j] = buf[scalar_index(F_Q0 + j, i)] + buf[scalar_index(F_Q + j, i)];   // device holds dq = q - q0
        for (int k = 0; k < 4; ++k) {
            int v; std::memcpy(&v, &buf[scalar_index(int_fields[k], i)], 4);
            scalars[(size_t)i * USIM_NSCALAR + int_fields[k]] = (float)v;
        }
        if (lattice && h->n_el)
            for (int e = 0; e < h->n_el; ++e) {
                lattice[((size_t)i * h->n_el + e) * 2] = buf[(size_t)F_LAT * h->npad + (size_t)i * lat_words(h) + lat_s(h) + e];
                lattice[((size_t)i * h->n_el + e) * 2 + 1] = buf[(size_t)F_LAT * h->npad + (size_t)i * lat_words(h) + lat_sd(h) + e];
            }
    }
    return USIM_OK;
}

int usim_set_state(usim_handle* h, const float* scalars, const float* lattice) {
    if (!h || !scalars) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<float> buf((size_t)h->nfields * h->npad);
    HIPCHK(h, hipMemcpy(buf.data(), h->state, buf.size() * sizeof(float), hipMemcpyDeviceToHost));
    const int int_fields[4] = {F_T, F_TOUCH, F_EPISODE, F_STATUS};
    for (int i = 0; i < h->n; ++i) {
        for (int f = 0; f < F_NSCALAR; ++f) buf[scalar_index(f, i)] = scalars[(size_t)i * USIM_NSCALAR + f];
        for (int j = 0; j < NJ; ++j) buf[scalar_index(F_Q + j, i)] = scalars[(size_t)i * USIM_NSCALAR + F_Q + j] - scalars[(size_t)i * USIM_NSCALAR + F_Q0 + j];   // device holds dq = q - q0
        for (int k = 0; k < 4; ++k) {
            int v = (int)scalars[(size_t)i * USIM_NSCALAR + int_fields[k]];
            std::memcpy(&buf[scalar_index(int_fields[k], i)], &v, 4);
        }
        if (lattice && h->n_el)
            for (int e = 0; e < h->n_el; ++e) {
                buf[(size_t)F_LAT * h->npad + (size_t)i * lat_words(h) + lat_s(h) + e] = lattice[((size_t)i * h->n_el + e) * 2];
                buf[(size_t)F_LAT * h->npad + (size_t)i * lat_words(h) + lat_sd(h) + e] = lattice[((size_t)i * h->n_el + e) * 2 + 1];
            }
    }
    HIPCHK(h, hipMemcpy(h->state, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
    if (h->warm) { int rc = warm_rows_reset(h); if (rc) return rc; }          // a state set from outside starts cold (usim_set_warm_start after this call restores the list)
    // the bank is a pure function of (seed, env, episode): rebuild every ring for the restored episode counters
    HIPCHK(h, hipMemset(h->d_count, 0, 2 * sizeof(int)));
    {
        int rc = bank_fill(h, nullptr, nullptr);
        if (rc) return rc;
    }
    HIPCHK(h, hipDeviceSynchronize());
    return USIM_OK;
}

// ---- snapshots: whole environments copied between the state block and a caller-owned device buffer of rows (usim_snapshot.h), one launch on the caller's stream and
// nothing else -- no synchronisation, no event, no allocation, no host counter: capture-safe like usim_refill_bank
static_assert(USIM_SNAPSHOT_WORDS_RIGID == F_NSCALAR && USIM_SNAPSHOT_WORDS_TOP == F_NSCALAR + LAT_ENV_WORDS && USIM_SNAPSHOT_WORDS_TOP_WARM == F_NSCALAR + LAT_ENV_WORDS + WARM_WORDS &&
              USIM_SNAPSHOT_WORDS_FULL == F_NSCALAR + LATF_ENV_WORDS, "include/usim.h");
static SnapLayout snap_layout(const usim_handle* h) {
    return {h->cfg.torso == USIM_TORSO_FULL ? LATF_ENV_WORDS : (h->n_el ? LAT_ENV_WORDS : 0), h->warm ? WARM_WORDS : 0, h->bank_row0};
}
static unsigned snap_grid(int rows, int lanes) { return (unsigned)(((size_t)rows * lanes + SNAP_WG - 1) / SNAP_WG); }

int usim_snapshot_words(const usim_handle* h) { return h ? snap_row_words(snap_layout(h)) : USIM_ERR_INVALID; }

int usim_save_envs(usim_handle* h, const int32_t* env_index_dev, int m, float* snap_dev, void* stream) {
    if (!h || !snap_dev || m <= 0 || (reinterpret_cast<uintptr_t>(snap_dev) & 15) || (!env_index_dev && m > h->n)) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    const SnapLayout L = snap_layout(h);
    hipStream_t s = (hipStream_t)stream;
    if (h->map == Mapping::FULL) hipLaunchKernelGGL(usim_save_envs_kernel<64>, dim3(snap_grid(m, 64)), dim3(SNAP_WG), 0, s, h->state, h->n, h->npad, L, env_index_dev, m, snap_dev);
    else hipLaunchKernelGGL(usim_save_envs_kernel<16>, dim3(snap_grid(m, 16)), dim3(SNAP_WG), 0, s, h->state, h->n, h->npad, L, env_index_dev, m, snap_dev);
    HIPCHK(h, hipGetLastError());
    return USIM_OK;
}

int usim_load_envs(usim_handle* h, const float* snap_dev, int m, const int32_t* row_of_env_dev, void* stream) {
    if (!h || !snap_dev || !row_of_env_dev || m <= 0 || (reinterpret_cast<uintptr_t>(snap_dev) & 15)) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    const SnapLayout L = snap_layout(h);
    hipStream_t s = (hipStream_t)stream;
    if (h->map == Mapping::FULL) hipLaunchKernelGGL(usim_load_envs_kernel<64>, dim3(snap_grid(h->n, 64)), dim3(SNAP_WG), 0, s, h->state, h->n, h->npad, L, snap_dev, m, row_of_env_dev);
    else hipLaunchKernelGGL(usim_load_envs_kernel<16>, dim3(snap_grid(h->n, 16)), dim3(SNAP_WG), 0, s, h->state, h->n, h->npad, L, snap_dev, m, row_of_env_dev);
    HIPCHK(h, hipGetLastError());
    return USIM_OK;
}

int usim_profile_step(usim_handle* h, const usim_step_io* s, int64_t step, uint64_t* ticks, int max_ticks) {
    if (!h || !ticks || max_ticks < 17) return USIM_ERR_INVALID;
#if !defined(USIM_TSTAMP) && !defined(USIM_TSTAMP_NOWAIT)
    h->hip_err = "usim_profile_step needs the profiling build (make -C csrc prof -> libusim_prof.so)";
    return USIM_ERR_UNSUPPORTED;
#endif
    DeviceGuard guard(h->device);
    DevIO io; int rc = fill_io(s, io, false);
    if (rc) return rc;
    io.act = nullptr;
    unsigned long long* d = nullptr;
    HIPCHK(h, hipMalloc(&d, 64 * sizeof(unsigned long long)));
    HIPCHK(h, hipMemset(d, 0, 64 * sizeof(unsigned long long)));
    io.dbg = d; io.items = h->d_items; io.count = h->d_count;
    // USIM_PROFILE_NSUB = k: the stamps of the LAST of k consecutive steps of one launch (multi-step kernels; never across a refill period)
    if (const char* ns = std::getenv("USIM_PROFILE_NSUB")) { const int v = std::atoi(ns); if (v > 1 && v <= BANK_DEPTH - h->steps_since_refill) { io.nsub = v; h->steps_since_refill += v - 1; } }
    rc = launch<0>(h, io, LF_AUTO_RESET | LF_RANDOM_ACT, (long long)step, nullptr);
    if (rc == USIM_OK && ++h->steps_since_refill >= BANK_DEPTH) rc = bank_refill(h, nullptr);
    HIPCHK(h, hipDeviceSynchronize());
    unsigned long long host[64];
    HIPCHK(h, hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost));
    HIPCHK(h, hipFree(d));
    for (int i = 0; i < (max_ticks < 64 ? max_ticks : 64); ++i) ticks[i] = host[i];      // 0-16: phases of the single-wave kernels; 20-29 / 30-39: arm / lattice side of the split kernel
    return rc;
}

const char* usim_strerror(int status) {
    switch (status) {
        case USIM_OK: return "ok";
        case USIM_ERR_INVALID: return "invalid argument or configuration";
        case USIM_ERR_NO_DEVICE: return "no usable HIP device";
        case USIM_ERR_HIP: return "HIP runtime error (see usim_last_hip_error)";
        case USIM_ERR_ALLOC: return "allocation failed";
        case USIM_ERR_UNSUPPORTED: return "unsupported configuration";
        default: return "unknown usim status";
    }
}
const char* usim_last_hip_error(const usim_handle* h) { return h ? h->hip_err.c_str() : ""; }
#ifndef USIM_SRC_HASH
#define USIM_SRC_HASH "unhashed"
#endif
const char* usim_version(void) { return "usim 0.5 (gfx950) src " USIM_SRC_HASH; }

}  // extern "C"

#include "usim_policy.hip"
