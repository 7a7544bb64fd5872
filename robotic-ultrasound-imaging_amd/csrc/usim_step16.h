// usim_step16.h -- step kernel with the arm mathematics of an environment DISTRIBUTED over the 16 lanes of its group (one DPP row).
//
// The first step kernel (round 1, since removed) replicated the 7-DoF arm mathematics in all lanes of a group: at 4096 envs/GPU every SIMD held
// one wave, the kernel was bound by VALU issue slots, and 4.1 k of its 7 k instructions per wave-step were that replicated stream.  Here a lane
// owns one link (joint space, lanes 0 .. nj-1) and / or one task-space row (lanes 0-2 position, 4-6 orientation); lane 7 owns the
// end-effector site frame.  Lanes exchange data with DPP row operations only (row_newbcast, row_shr / row_shl, quad_perm) plus two 8 x 8
// transposes through LDS:
//   * kinematics: the world frame of every link is a prefix SCAN over the composition of the local link transforms (three shifted steps);
//   * Newton-Euler bias forces: angular velocity / acceleration and origin acceleration are prefix SUMS of per-link terms, the force and
//     moment accumulation is a suffix sum;
//   * mass matrix (composite rigid body): suffix sums of the link inertias about the base origin; lane i forms row i from the axes of
//     lanes j <= i (row broadcasts), the upper triangle comes back through the LDS transpose;
//   * M^-1 by an in-place Gauss-Jordan sweep with row i in lane i (no pivoting: M is symmetric positive definite);
//   * operational space: lane j keeps column j of the site Jacobian, task lane a keeps row a (LDS transpose), Lambda^-1 = J M^-1 J^T row a
//     in task lane a; the two 3 x 3 solves of the uncoupled controller run inside the quads, the 6 x 6 nullspace solve across the six task
//     lanes (Gauss-Jordan on [A | b] again);
//   * every M^-1 / J / J^T product afterwards is "own row times broadcast vector".
// The algorithm is modelled lane by lane in tests/arm_lanes_model.py and checked there against the serial chain.  The robot is a table
// (DevModel::tables + TB_ARM, usim_device.h ArmTable): per lane the fixed transform to the parent link frame, a joint about the local z axis,
// inertial parameters in the link frame -- the kernel is the same for every chain of up to seven joints.
//
// Lattice / contact phases (soft torso) are the ones of usim_kernels.hip and usim_contact.h (lattice_rhs, lattice_solve, collide_*; contact_solve): the G = 16 mapping is unchanged there.
// A pass of a step kernel is step16_one (single-wave kernels; arm wave of the split kernel) or lattice_pass (lattice / contact wave of the split kernel); step16_body loops over
// the passes of a launch.
#pragma once
#include <type_traits>

namespace usim {

template <int N, class F>
DI void static_for(F&& f) {
    if constexpr (N > 0) { static_for<N - 1>(f); f(std::integral_constant<int, N - 1>{}); }
}

// ---- DPP row primitives.  A DPP row is 16 lanes.  G = 16: the row is the group of one environment.  G = 8 (split kernel beyond 4096 envs/GPU):
// a row holds the groups of TWO environments, lanes 0-7 and 8-15 -- the arm mathematics only ever used lanes 0-7 of a group (seven links + the
// site frame; task rows in lanes 0-2 / 4-6), so the second environment takes the lanes that idled.  A broadcast then needs one instruction per
// half (bank_mask 0x3 / 0xc select lanes 0-7 / 8-15 of every row), a shift one select that keeps lane 8 .. from reading across the fence. ----
template <int CTRL>
DI float dpp0(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true)); }
template <int G> DI int glane() { return (int)(threadIdx.x & (G - 1)); }
template <int G, int K> DI float rbc(float v) {                                        // value of lane K of the group, in every lane of the group
    if constexpr (G == 16) return dpp0<0x150 + K>(v);
    else {
        const int iv = __float_as_int(v);
        const int t = __builtin_amdgcn_update_dpp(iv, iv, 0x150 + K, 0xf, 0x3, false);
        return __int_as_float(__builtin_amdgcn_update_dpp(t, iv, 0x150 + 8 + K, 0xf, 0xc, false));
    }
}
template <int G, int D> DI float rshr0(float v) {                                      // value of lane l - D of the group (0 for l < D)
    const float t = dpp0<0x110 + D>(v);
    if constexpr (G == 16) return t; else return (glane<G>() < D) ? 0.f : t;
}
template <int G, int D> DI float rshl0(float v) {                                      // value of lane l + D of the group (0 beyond it)
    const float t = dpp0<0x100 + D>(v);
    if constexpr (G == 16) return t; else return (glane<G>() >= G - D) ? 0.f : t;
}
template <int G, int D> DI float rshr(float v, float fill) {                           // value of lane l - D of the group (`fill` for l < D)
    const float t = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x110 + D, 0xf, 0xf, false));
    if constexpr (G == 16) return t; else return (glane<G>() < D) ? fill : t;
}
template <int K> DI float qbc(float v) { return dpp0<K * 0x55>(v); }                  // value of lane K of the quad
template <int G, int K> DI f3 rbc3(f3 v) { return mk(rbc<G, K>(v.x), rbc<G, K>(v.y), rbc<G, K>(v.z)); }
template <int G> DI float prefix_sum(float v) { v += rshr0<G, 1>(v); v += rshr0<G, 2>(v); v += rshr0<G, 4>(v); return v; }     // inclusive, over lanes l-7 .. l of the group
template <int G> DI float suffix_sum(float v) { v += rshl0<G, 1>(v); v += rshl0<G, 2>(v); v += rshl0<G, 4>(v); return v; }     // inclusive, over lanes l .. l+7
template <int G> DI f3 prefix_sum(f3 v) { return mk(prefix_sum<G>(v.x), prefix_sum<G>(v.y), prefix_sum<G>(v.z)); }
template <int G> DI f3 suffix_sum(f3 v) { return mk(suffix_sum<G>(v.x), suffix_sum<G>(v.y), suffix_sum<G>(v.z)); }

constexpr int TASK_LANE[6] = {0, 1, 2, 4, 5, 6};      // lane that owns task-space row a: position rows in quad 0, orientation rows in quad 1

// ---- fused DPP arithmetic.  The compiler folds a row shift into v_add_f32_dpp by itself but keeps a broadcast feeding a multiply-add as
// v_mov_b32_dpp + v_fmac_f32 (the accumulator of v_fmac is tied to the destination, which its DPP combiner does not model), so the
// "own row times broadcast vector" products are written out: one v_fmac_f32_dpp per term (G = 8: one per term and half of the row).  A DPP
// source written by the VALU instruction right before needs two wait states, and the hazard recogniser does not look inside inline assembly:
// every block opens with s_nop 1. ----
#define USIM_DPP_BC(K) " row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t"
#define USIM_DPP_LO(K) " row_newbcast:" #K " row_mask:0xf bank_mask:0x3\n\t"
// (the second environment of a row reads lane K + 8: the operand is spelled out per call site)
// sum_j A[j] * (value of v in lane j), j = 0 .. 6: own row times a vector that lives one component per joint lane
DI float row_times_joint7(const float* A, float v) {
    float s;
    asm("s_nop 1\n\t"
        "v_mul_f32_dpp %0, %1, %2" USIM_DPP_BC(0) "v_fmac_f32_dpp %0, %1, %3" USIM_DPP_BC(1) "v_fmac_f32_dpp %0, %1, %4" USIM_DPP_BC(2)
        "v_fmac_f32_dpp %0, %1, %5" USIM_DPP_BC(3) "v_fmac_f32_dpp %0, %1, %6" USIM_DPP_BC(4) "v_fmac_f32_dpp %0, %1, %7" USIM_DPP_BC(5)
        "v_fmac_f32_dpp %0, %1, %8" USIM_DPP_BC(6)
        : "=&v"(s) : "v"(v), "v"(A[0]), "v"(A[1]), "v"(A[2]), "v"(A[3]), "v"(A[4]), "v"(A[5]), "v"(A[6]));
    return s;
}
// the same for the two 8-lane groups of a row: lanes 0-7 read lanes 0-6, lanes 8-15 read lanes 8-14
DI float row_times_joint7_g8(const float* A, float v) {
    float s;
    asm("s_nop 1\n\t"
        "v_mul_f32_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"  "v_mul_f32_dpp %0, %1, %2 row_newbcast:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_fmac_f32_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %3 row_newbcast:9 row_mask:0xf bank_mask:0xc\n\t"
        "v_fmac_f32_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %4 row_newbcast:10 row_mask:0xf bank_mask:0xc\n\t"
        "v_fmac_f32_dpp %0, %1, %5 row_newbcast:3 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %5 row_newbcast:11 row_mask:0xf bank_mask:0xc\n\t"
        "v_fmac_f32_dpp %0, %1, %6 row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %6 row_newbcast:12 row_mask:0xf bank_mask:0xc\n\t"
        "v_fmac_f32_dpp %0, %1, %7 row_newbcast:5 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %7 row_newbcast:13 row_mask:0xf bank_mask:0xc\n\t"
        "v_fmac_f32_dpp %0, %1, %8 row_newbcast:6 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %8 row_newbcast:14 row_mask:0xf bank_mask:0xc"
        : "=&v"(s) : "v"(v), "v"(A[0]), "v"(A[1]), "v"(A[2]), "v"(A[3]), "v"(A[4]), "v"(A[5]), "v"(A[6]));
    return s;
}
template <int G, int NJ_>
DI float row_times_joint(const float* A, float v) {
    static_assert(NJ_ == 7, "seven joint lanes");
    if constexpr (G == 16) return row_times_joint7(A, v); else return row_times_joint7_g8(A, v);
}
// sum_a A[a] * (value of t in task lane a), task lanes 0 1 2 4 5 6
template <int G>
DI float col_times_task(const float* A, float t) {
    float s;
    if constexpr (G == 16) {
        asm("s_nop 1\n\t"
            "v_mul_f32_dpp %0, %1, %2" USIM_DPP_BC(0) "v_fmac_f32_dpp %0, %1, %3" USIM_DPP_BC(1) "v_fmac_f32_dpp %0, %1, %4" USIM_DPP_BC(2)
            "v_fmac_f32_dpp %0, %1, %5" USIM_DPP_BC(4) "v_fmac_f32_dpp %0, %1, %6" USIM_DPP_BC(5) "v_fmac_f32_dpp %0, %1, %7" USIM_DPP_BC(6)
            : "=&v"(s) : "v"(t), "v"(A[0]), "v"(A[1]), "v"(A[2]), "v"(A[3]), "v"(A[4]), "v"(A[5]));
    } else {
        asm("s_nop 1\n\t"
            "v_mul_f32_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"  "v_mul_f32_dpp %0, %1, %2 row_newbcast:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %3 row_newbcast:9 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %4 row_newbcast:10 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %1, %5 row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %5 row_newbcast:12 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %1, %6 row_newbcast:5 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %6 row_newbcast:13 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %1, %7 row_newbcast:6 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %1, %7 row_newbcast:14 row_mask:0xf bank_mask:0xc"
            : "=&v"(s) : "v"(t), "v"(A[0]), "v"(A[1]), "v"(A[2]), "v"(A[3]), "v"(A[4]), "v"(A[5]));
    }
    return s;
}
// A[c] += (value of A[c] in lane K) * f  for the seven entries of a row (Gauss-Jordan row update: the pivot row is lane K's)
template <int G, int K>
DI void row_axpy_bc7(float* A, float f) {
    if constexpr (G == 16) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %0, %7 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %1, %1, %7 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %2, %2, %7 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %3, %3, %7 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %4, %4, %7 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %5, %5, %7 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %6, %6, %7 row_newbcast:%8 row_mask:0xf bank_mask:0xf"
            : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(A[4]), "+v"(A[5]), "+v"(A[6]) : "v"(f), "n"(K));
    } else {
        // the pivot row's own entries must be read before they are overwritten: lanes 0-7 and 8-15 are updated by separate instructions, and the
        // pivot lanes K / K + 8 update themselves with f = (1 - pivot) / pivot - ... exactly as in the 16-lane form (same arithmetic per lane)
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %0, %7 row_newbcast:%8 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %0, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %1, %1, %7 row_newbcast:%8 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %1, %1, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %2, %2, %7 row_newbcast:%8 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %2, %2, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %3, %3, %7 row_newbcast:%8 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %3, %3, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %4, %4, %7 row_newbcast:%8 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %4, %4, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %5, %5, %7 row_newbcast:%8 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %5, %5, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %6, %6, %7 row_newbcast:%8 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %6, %6, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xc"
            : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(A[4]), "+v"(A[5]), "+v"(A[6]) : "v"(f), "n"(K), "n"(K + 8));
    }
}
// z . n + vo . f with (z, vo) taken from lane K: entry K of this lane's row of the mass matrix
template <int G, int K>
DI float spatial_dot_bc(f3 z, f3 vo, f3 n, f3 f) {
    float s;
    if constexpr (G == 16) {
        asm("s_nop 1\n\t"
            "v_mul_f32_dpp %0, %1, %7 row_newbcast:%13 row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %0, %2, %8 row_newbcast:%13 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_newbcast:%13 row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %0, %4, %10 row_newbcast:%13 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f32_dpp %0, %5, %11 row_newbcast:%13 row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %0, %6, %12 row_newbcast:%13 row_mask:0xf bank_mask:0xf"
            : "=&v"(s) : "v"(z.x), "v"(z.y), "v"(z.z), "v"(vo.x), "v"(vo.y), "v"(vo.z), "v"(n.x), "v"(n.y), "v"(n.z), "v"(f.x), "v"(f.y), "v"(f.z), "n"(K));
    } else {
        asm("s_nop 1\n\t"
            "v_mul_f32_dpp %0, %1, %7 row_newbcast:%13 row_mask:0xf bank_mask:0x3\n\t"   "v_mul_f32_dpp %0, %1, %7 row_newbcast:%14 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %2, %8 row_newbcast:%13 row_mask:0xf bank_mask:0x3\n\t"  "v_fmac_f32_dpp %0, %2, %8 row_newbcast:%14 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_newbcast:%13 row_mask:0xf bank_mask:0x3\n\t"  "v_fmac_f32_dpp %0, %3, %9 row_newbcast:%14 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_newbcast:%13 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %4, %10 row_newbcast:%14 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %5, %11 row_newbcast:%13 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %5, %11 row_newbcast:%14 row_mask:0xf bank_mask:0xc\n\t"
            "v_fmac_f32_dpp %0, %6, %12 row_newbcast:%13 row_mask:0xf bank_mask:0x3\n\t" "v_fmac_f32_dpp %0, %6, %12 row_newbcast:%14 row_mask:0xf bank_mask:0xc"
            : "=&v"(s) : "v"(z.x), "v"(z.y), "v"(z.z), "v"(vo.x), "v"(vo.y), "v"(vo.z), "v"(n.x), "v"(n.y), "v"(n.z), "v"(f.x), "v"(f.y), "v"(f.z), "n"(K), "n"(K + 8));
    }
    return s;
}

// world frame of every link: local transform of this lane's link (fixed rotation, joint about the local z axis), then the scan
// T_l <- T_(l-d) o T_l for d = 1, 2, 4.  X, Y, Z: rotation columns, P: origin.  Lanes without a joint carry q = 0 (sin 0 = 0, cos 0 = 1 exactly).
template <int G>
DI void fk16(const float* at, const float q, f3& X, f3& Y, f3& Z, f3& P) {
    float s, c;
    sincos_(q, s, c);
    const f3 f0 = mk(at[AT_RFIX], at[AT_RFIX + 1], at[AT_RFIX + 2]), f1 = mk(at[AT_RFIX + 3], at[AT_RFIX + 4], at[AT_RFIX + 5]);
    X = f0 * c + f1 * s; Y = f1 * c - f0 * s; Z = mk(at[AT_RFIX + 6], at[AT_RFIX + 7], at[AT_RFIX + 8]);
    P = mk(at[AT_LPOS], at[AT_LPOS + 1], at[AT_LPOS + 2]);
    static_for<3>([&](auto Dc) {
        constexpr int D = 1 << decltype(Dc)::value;
        // lanes l < D read the identity (fill values of the shift): their frame is already complete
        const f3 LX = mk(rshr<G, D>(X.x, 1.f), rshr<G, D>(X.y, 0.f), rshr<G, D>(X.z, 0.f));
        const f3 LY = mk(rshr<G, D>(Y.x, 0.f), rshr<G, D>(Y.y, 1.f), rshr<G, D>(Y.z, 0.f));
        const f3 LZ = mk(rshr<G, D>(Z.x, 0.f), rshr<G, D>(Z.y, 0.f), rshr<G, D>(Z.z, 1.f));
        const f3 LP = mk(rshr0<G, D>(P.x), rshr0<G, D>(P.y), rshr0<G, D>(P.z));
        const f3 nX = LX * X.x + LY * X.y + LZ * X.z, nY = LX * Y.x + LY * Y.y + LZ * Y.z, nZ = LX * Z.x + LY * Z.y + LZ * Z.z;
        P = LP + LX * P.x + LY * P.y + LZ * P.z;
        X = nX; Y = nY; Z = nZ;
    });
}

// column l of the site Jacobian in joint lane l -> row a in task lane a, through the 8 x 8 LDS scratch of the environment
DI void jacobian_rows(float* xl, const int gl, const float* Jc, float* Jr) {
    if (gl < 8) {
#pragma unroll
        for (int a = 0; a < 6; ++a) xl[a * 8 + gl] = Jc[a];
    }
    group_sync();
    int arow = (gl & 7) - ((gl & 4) ? 1 : 0);
    arow = arow > 5 ? 5 : arow;
    const float4 j0 = *reinterpret_cast<const float4*>(&xl[arow * 8]), j1 = *reinterpret_cast<const float4*>(&xl[arow * 8 + 4]);
    Jr[0] = j0.x; Jr[1] = j0.y; Jr[2] = j0.z; Jr[3] = j0.w; Jr[4] = j1.x; Jr[5] = j1.y; Jr[6] = j1.z; Jr[7] = j1.w;
}

// solution of the 6 x 6 system whose row a (A[0..5] | b) lives in task lane a: Gauss-Jordan across the six task lanes, no pivoting (the
// matrices are symmetric positive definite).  Lanes without a task row must pass zero rows: they are never pivots.
template <int G>
DI float solve6_task(float* A, float b, const int gl) {
    static_for<6>([&](auto Kc) {
        constexpr int k = decltype(Kc)::value;
        constexpr int lk = TASK_LANE[k];
        const float g = (A[k] - (gl == lk ? 1.f : 0.f)) * rcp_(rbc<G, lk>(A[k]));
#pragma unroll
        for (int c = k + 1; c < 6; ++c) A[c] = fmaf(-g, rbc<G, lk>(A[c]), A[c]);
        b = fmaf(-g, rbc<G, lk>(b), b);
    });
    return b;
}

// per-environment LDS scratch of the two transposes: 8 x 8 words
constexpr int X16_WORDS = 64;
constexpr int X16_RIGID_STRIDE = 84;                  // rigid-torso launches: one block per environment: 64 words transpose scratch + 12 words `fixed`-mode goal (84 mod 32 = 20)

// OCC = waves per SIMD the register allocation aims at.  1: the whole register file for one wave (no spills; the choice up to 4096 envs/GPU,
// where every SIMD holds one wave anyway).  2: 256 registers per lane (the soft-torso kernel then keeps ~27 values in scratch): beyond 4096
// envs/GPU two waves share a SIMD and fill each other's stalls (8192 envs: 28.6 us/step against 37.4 us in two rounds of one wave).
// MODE 0: one env.step() per environment; a finished environment takes its next initial state from the reset bank.
// MODE 1: reset computation (draws, initial-pose IK, zero-torque forward pass) for the environments selected by the mask (written to the
//         live state) or for the (env, episode) items of the refill work list (written to the reset bank).
//
// ROLE (usim_step32_kernel): the soft-torso step of four environments split over TWO waves that share a SIMD -- ROLE 1 runs the arm side
// (kinematics ... controller, then acceleration, sensors, reward, bookkeeping), ROLE 2 the lattice / contact side (staging, right-hand side,
// matrix-core solve, collision, contact solve, element integration).  They meet at workgroup barriers and hand over through per-environment
// LDS mailboxes: site pose (1 -> 2), Lambda^-1 / alpha / vs (1 -> 2), contact wrench and contact list (2 -> 1).  ROLE 0 = one wave does both.
// Two functions state a pass: step16_one for ROLE 0 and ROLE 1, lattice_pass for ROLE 2; step16_body calls the one or the other.
//
// waves per role in a workgroup of the split kernel: one 512-thread workgroup per CU (two 256-thread workgroups per CU, with barrier domains of their own, measured slower
// for both group sizes: DESIGN.md section 4.8)
constexpr int SPLIT_WPR = 4;
// Split kernel: behind the per-environment blocks (16 with 16-lane groups, 32 with 8-lane groups) every environment has a mailbox block, one layout for both
// group sizes (word offsets):
constexpr int MB_POSE = X16_WORDS;                    // (before it: the 8 x 8 transpose scratch of the arm wave)  site pose 9 words; word 10: length of the broad-phase queue
constexpr int MB_OP = MB_POSE + 12;                   // op-space quantities: 6 x 8 Lambda^-1, alpha 6, vs 6
constexpr int MB_W = MB_OP + 64;                      // contact wrench 6, contact count, overflow flag, the contacts' element ids 8 (between the steps of a resident launch: the new episode's parameters)
constexpr int MB_Q = MB_W + 16;                       // broad-phase queue (element ids; the spare last word takes the non-candidates' stores)
constexpr int MB_GOAL = MB_Q + 100;                   // `fixed` mode with physics substeps: the goal anchored at the policy step (12 words)
// Action drawn ahead (split kernel, resident launches of usim_rollout_random; AHEAD of step16_one): the arm wave draws the NEXT pass's random action in its idle window
// between precompute() and hand-off (3) and keeps the seven words in its own mailbox block (written and read by the same wave), so that the Philox rounds leave the
// chain behind hand-off (1).
constexpr int MB_ACT = MB_GOAL + 12;                  // the action of the running control step / of the next one (7 words + 1)
// Report written late (split kernel, 16-lane groups, resident launches; arm_report_late below): what the arm wave needs to write the report of pass k during pass k + 1
// is parked here.  Only the arm wave touches the area, and every word is written and read by lanes of the environment's own group: no hand-off involved.
constexpr int MB_REP = MB_ACT + 8;
constexpr int REP_LINK = 0;                           // lane NJ - 1's words of the probe torque sensor: al, ao, s_xso, s_rc, s_wwrc, s_nw, s_arm, X, Y, Z (30 words + 2)   -- parked in the wait
constexpr int REP_SITE = 32;                          // site frame sx, sy, sz (9 words), obs[9 .. 18] (10 words) + 1                                                       -- parked in the wait
constexpr int REP_W = 52;                             // contact wrench (6), hand velocity (3), reward, episode return, t, status, done | need << 1, contact count + 1 pad    -- parked behind the state part
constexpr int REP_SHELL = 68;                         // shell ids of the contacts (launches that report contacts)                                                            -- parked behind the state part
constexpr int REP_AQ = 76;                            // site acceleration of the constrained arm, component a from task lane a (6 words + 2)                                  -- parked behind the state part
constexpr int REP_WORDS = 84;
// which split kernels those are: G lanes per environment, RES = resident (multi-step) launch
template <int G, bool RES> constexpr bool report_late() { return G == 16 && RES; }
// words of an environment's mailbox block: the kernels that write the report late (REP) have the area behind MB_ACT, the others keep the block they had
template <bool REP> constexpr int x2_stride() { return MB_REP + (REP ? REP_WORDS : 0); }
template <int G> constexpr int x2_base() { return TB_WORDS + (64 * SPLIT_WPR / G) * GE_STRIDE; }
static_assert(x2_base<16>() % 4 == 0 && x2_base<8>() % 4 == 0 && x2_stride<false>() % 4 == 0 && x2_stride<true>() % 4 == 0 && MB_OP % 4 == 0 && MB_W % 4 == 0 && MB_ACT % 4 == 0
              && MB_REP % 4 == 0 && REP_SITE % 4 == 0 && REP_W % 4 == 0 && REP_SHELL % 4 == 0 && REP_AQ % 4 == 0 && REP_WORDS % 4 == 0, "mailbox block: 16-byte accesses");
static_assert((x2_base<8>() + 32 * x2_stride<false>()) * 4 <= 160 * 1024, "split kernel with 8-lane groups: LDS of a CU");
static_assert(OBS_DIM == 19 && MAXC == 8 && REP_AQ + 8 == REP_WORDS, "layout of the report area");
// Collision in the split kernel: the broad phase (collide_cull) leaves the ids of the elements that can touch the probe (ascending) in the environment's queue, and the
// lattice side evaluates the whole queue after hand-off (1) (collide_queue), typically in one pass of its lanes.  Who culls:
//   8-lane groups:  the arm side, which has the site pose first, runs 7 of the 13 rounds before hand-off (1), while the lattice side still stages its right-hand side and
//                   solves; the lattice side appends the other 6 after the hand-off.
//   16-lane groups: the lattice side runs all 7 rounds after the hand-off; the arm side, the longer one on both sides of hand-off (1), runs none and never needs the
//                   integrated element positions (which is what lets the lattice wave run ahead, below).
// (7 / 5 / 3 / 0 arm-side rounds of 16-lane groups measured: profiles/handoff_balance/ab.txt.  Giving the arm side a share of the NARROW phase measured slower for every
// share and both group sizes -- DESIGN.md section 4.6 -- and was removed.)
template <int G> constexpr int arm_cull_rounds() { return G == 16 ? 0 : 7; }
// LA, the lattice solve ahead (split kernel, 16-lane groups, resident launches): lattice_rhs and lattice_solve need nothing from the arm side but "this episode ended", which
// happens once per episode.  The lattice wave therefore goes straight from integrating pass k into the right-hand side and the solve of pass k + 1 on the state in its
// registers and meets the arm wave only at hand-off (1) of pass k + 1; hand-off (4) and the barrier between the passes exist on the last pass of a launch only.  After
// hand-off (1) it reads the arm wave's new-episode word; if an environment of the wave has one it adopts it and runs the two phases again for the wave (same instructions on
// the same inputs for the environments that went on: same bits).  The lattice wave then owns EB(GE_S) and carries kst / kdmp / mu / t, the lattice and the warm record
// between the passes.  The hand-offs and what each hazard rests on: BARRIER INVARIANT at usim_step32_kernel.
// Such a lattice wave runs at s_setprio 1 from hand-off (2) to hand-off (1) of the next pass, where it is the longer one of the pair, and at 0 between (1) and (2), where the
// arm wave is (the two share the VALU issue of their SIMD, the older one -- the arm wave -- first; the other windows measured: profiles/lattice_ahead/ab.txt).
template <int ROLE, int G, bool RES> constexpr bool lattice_ahead() { return ROLE != 0 && G == 16 && RES; }

// workgroup barrier of the step kernels; the profiling build counts them per role (BARRIER INVARIANT at usim_step32_kernel)
#if defined(USIM_TSTAMP) || defined(USIM_TSTAMP_NOWAIT)
#define USIM_BAR() do { __syncthreads(); ++nbar; } while (0)
#else
#define USIM_BAR() __syncthreads()
#endif


// State of an environment that stays in the registers of its lanes from one step of a multi-step launch to the next (RES): its joint words, the
// scalar words (held by every lane of the group) and its elements of the lattice.  Every step still STORES the state (and its slice of the
// transition block); what a resident launch saves is waiting for the words it stored itself to come back.  The arm table (28 words per lane,
// needed at the top of every step) is parked in LDS behind everything else during the first step and read from there afterwards: kept in
// registers it would be live across the whole step (the split kernel spills at 256 registers).
// Who carries what: a single wave (ROLE 0) all of it; the arm wave of the split kernel (ROLE 1) the joint words and `ep`, and of `s` -- 8-lane groups only -- a copy it
// refreshes from LDS every pass to cull on; the lattice wave (lattice_pass) kst, kdmp, mu and t of `ep`, s, sd and wr, and nothing else.
constexpr int ARM_LDS_WORDS = A16_LANES * AT_STRIDE;
template <int TORSO, int ROLE, int G, bool RES = false> constexpr int arm_lds_base();
template <int NE, class WR = NoWarm>
struct Carry {
    float dqj, qdj, q0j;
    Episode ep;
    float s[NE], sd[NE];
    WR wr;                                                               // kept contact list of the lane (warm start; NoWarm: nothing)
};

template <int TORSO, int ROLE, int G, bool RES> constexpr int arm_lds_base() {                    // (RES: the split kernels' mailbox blocks depend on it, x2_stride)
    return ROLE != 0 ? x2_base<G>() + (64 * SPLIT_WPR / G) * x2_stride<report_late<G, RES>()>() : (TORSO ? SOFT16_LDS_WORDS : 16 * X16_RIGID_STRIDE);
}
static_assert((arm_lds_base<1, 1, 8>() + ARM_LDS_WORDS) * 4 <= 160 * 1024 && arm_lds_base<1, 1, 8>() % 4 == 0 && arm_lds_base<1, 1, 16>() % 4 == 0 && arm_lds_base<1, 0, 16>() % 4 == 0
              && arm_lds_base<0, 0, 16>() % 4 == 0 && arm_lds_base<1, 1, 16, true>() % 4 == 0 && arm_lds_base<1, 1, 8, true>() == arm_lds_base<1, 1, 8>()
              && (arm_lds_base<1, 1, 16, true>() + ARM_LDS_WORDS) * 4 <= 160 * 1024, "arm table behind the LDS blocks of every 16-lane kernel");

// One pass of the lattice / contact wave of the split kernel (ROLE 2; its partner, the arm wave, runs step16_one<1, 0, 1, ...>): the soft-torso step (TORSO 1, MODE 0) of the
// wave's environments from staging the right-hand side to the integrated lattice.  Per environment it
//   reads from HBM (first pass of a launch)   kst, kdmp, mu, t; its elements' s and sd; its warm record (WR = WarmRec)
//   carries between the passes (RES)          the same, in `cy` (and nothing else of it)
//   takes from the arm wave                   site pose and, with 8-lane groups, the queue's first part and EB(GE_S) -- behind (1); Lambda^-1, alpha, vs -- behind (2);
//                                             the new-episode word in MB_W -- 8-lane groups: at the top of a pass, 16-lane resident launches (LA): behind (1)
//   hands to the arm wave                     contact wrench, count, overflow flag and the contacts' elements in MB_W -- before (3)
//   writes to HBM                             s and sd of its elements and the warm record -- before (4)
// and meets the arm wave at the table copy and at hand-offs (1)-(4): BARRIER INVARIANT at usim_step32_kernel.  `more` = another pass of this launch follows this one.
template <int NT, int G, bool RES, class WR>
DI void lattice_pass(float* lds, const DevModel& M, const DevCfg& C, float* __restrict__ st, const int n, const int npad, const DevIO& io,
                     const bool first_pass, const int sub, const bool more, int& nbar, Carry<(N_TOP + G - 1) / G, WR>& cy) {
    constexpr bool WARM = !std::is_same<WR, NoWarm>::value;             // this wave solves the contacts: it loads, keeps and stores the lane's record of the kept list
    constexpr int WPR = SPLIT_WPR, EPW = 64 / G, EPB = WPR * EPW;       // environments per wave / per workgroup (WPR waves per role)
    constexpr unsigned GMASK = (G == 16) ? 0xffffu : 0xffu;
    constexpr int NE = (N_TOP + G - 1) / G;
    constexpr bool LA = lattice_ahead<2, G, RES>();
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & (WPR - 1);      // wave within its role = quad of environments
    const bool fresh = !RES || first_pass;                              // the state comes from HBM (first step of a launch; every single-step launch)
    const int gl = lane & (G - 1), ge = lane / G;
    const int gbase = lane - gl;
    const int eb = wave * EPW + ge;
    unsigned long long* const dbg = io.dbg;
    const int env = blockIdx.x * EPB + eb;
    const bool valid = env < n;
    const bool store = valid && gl == 0;                                // [b], below
    const int ei = valid ? env : n - 1;                                 // clamp so that every lane has something to read; stores are guarded
#define LAT(w) st[(size_t)F_LAT * npad + (size_t)ei * LAT_ENV_WORDS + (w)]
#define EB(off) lds[TB_WORDS + eb * GE_STRIDE + (off)]
    float* const warm_rows = st + warm_index(io.bank_row0, npad, (size_t)ei);      // (dereferenced by handles with warm rows only)
    int mbo = x2_base<G>() + eb * x2_stride<report_late<G, RES>()>();                            // the environment's mailbox block, its offset opaque: one address register (step16_one)
    asm volatile("" : "+v"(mbo));

    // ---------------- load: the environment's contact parameters and step count, this lane's elements and warm record ----------------
    // BALLAST, marked [b]: statements of the arm wave that this prologue had while it was step16_one's.  Nothing in this function reads what they compute and the compiler
    // deletes every one of them, but each, taken out of the source, changes the register allocation and the schedule of the twelve split kernels, and the prologue without
    // them (one 16-byte load of kst, kdmp, mu, t; no arm table, joint words or other scalar words) measured 0.2 - 0.3 % slower with 8-lane groups at 8192 environments in two
    // sessions (profiles/lattice_pass/ab.txt).  They stay, in their order, for a change that measures these kernels anyway to remove.
    float* const xl = &lds[mbo];                                        // [b]
    float* const goal_lds = xl + MB_GOAL;                               // [b]
    float at[AT_STRIDE];                                                // [b] down to `jl`
    {
        constexpr int ARM_LDS = arm_lds_base<1, 2, G, RES>();
        const float4* ap = fresh ? reinterpret_cast<const float4*>(M.tables + TB_ARM + gl * AT_STRIDE) : reinterpret_cast<const float4*>(lds + ARM_LDS + gl * AT_STRIDE);
        if (fresh) {
#pragma unroll
            for (int v = 0; v < AT_STRIDE / 4; ++v) { const float4 x = ap[v]; at[4 * v] = x.x; at[4 * v + 1] = x.y; at[4 * v + 2] = x.z; at[4 * v + 3] = x.w; }
        } else {
            const float4* lp = reinterpret_cast<const float4*>(lds + ARM_LDS + gl * AT_STRIDE);
#pragma unroll
            for (int v = 0; v < AT_STRIDE / 4; ++v) { const float4 x = lp[v]; at[4 * v] = x.x; at[4 * v + 1] = x.y; at[4 * v + 2] = x.z; at[4 * v + 3] = x.w; }
        }
    }
    const float* const sp = st + scalar_index(0, (size_t)ei);
    const bool jlane = at[AT_JOINT] != 0.f;
    const int jl = jlane ? gl : NJ - 1;
    float &dqj = cy.dqj, &qdj = cy.qdj, &q0j = cy.q0j;                  // [b]
    Episode& E = cy.ep;
    f3 &ts = E.ts, &te = E.te;                                          // [b]
    float &u0 = E.u0, &vbar = E.vbar, &fzbar = E.fzbar, &fzprev = E.fzprev, &dfz = E.dfz, &kst = E.kst, &kdmp = E.kdmp, &mu = E.mu, &epret = E.epret;      // [b] but kst, kdmp, mu
    int &t = E.t, &touched = E.touched, &episode = E.episode, &status = E.status;                                                                            // [b] but t
    float (&s_pre)[NE] = cy.s, (&sd_pre)[NE] = cy.sd;
    // resident launches: the arm side reports a new episode through the mailbox (MB_W: kst, kdmp, mu, 1): the lattice at rest, the episode's parameters, t = 0
    auto adopt = [&](const float4 nx) {
        kst = nx.x; kdmp = nx.y; mu = nx.z; t = 0;
#pragma unroll
        for (int i = 0; i < NE; ++i) { s_pre[i] = 0.f; sd_pre[i] = 0.f; }
        warm_clear(cy.wr);                                               // an episode starts cold
    };
    if (fresh) {
        dqj = sp[F_Q + jl]; qdj = sp[F_QD + jl]; q0j = sp[F_Q0 + jl];     // [b]
        float sv[20];                                              // scalar words 20 .. 39: this wave reads kst, kdmp, mu and t of them
        {
            const float4* s4 = reinterpret_cast<const float4*>(sp + 20);
#pragma unroll
            for (int v = 0; v < 5; ++v) { const float4 x = s4[v]; sv[4 * v] = x.x; sv[4 * v + 1] = x.y; sv[4 * v + 2] = x.z; sv[4 * v + 3] = x.w; }
        }
#define SV(f) sv[(f) - 20]
        ts = mk(SV(F_TS), SV(F_TS + 1), SV(F_TS + 2)); te = mk(SV(F_TE), SV(F_TE + 1), SV(F_TE + 2));                                  // [b]
        u0 = SV(F_U0); vbar = SV(F_VBAR); fzbar = SV(F_FZBAR); fzprev = SV(F_FZPREV); dfz = SV(F_DFZ);                                 // [b]
        kst = SV(F_KST); kdmp = SV(F_KDMP); mu = SV(F_MU); epret = SV(F_EPRET);                                                         // (epret: [b])
        t = __float_as_int(SV(F_T)); touched = __float_as_int(SV(F_TOUCH)); episode = __float_as_int(SV(F_EPISODE)); status = __float_as_int(SV(F_STATUS));      // (all but t: [b])
#undef SV
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int e = gl + i * G;
            s_pre[i] = 0.f; sd_pre[i] = 0.f;
            if (e < N_TOP) { s_pre[i] = LAT(LAT_S + e); sd_pre[i] = LAT(LAT_SD + e); }
        }
        if constexpr (WARM) warm_load(warm_rows, gl, cy.wr);
    } else if constexpr (RES && !LA) {
        // resident launch, 8-lane groups: the word is read here (16-lane groups, LA: behind hand-off (1), below)
        const float4 nx = *reinterpret_cast<const float4*>(&lds[mbo + MB_W]);
        if (nx.w != 0.f) adopt(nx);
    }
    if (!jlane) { dqj = 0.f; qdj = 0.f; q0j = 0.f; }                    // [b]
    float qj = q0j + dqj;                                               // [b]
    if (first_pass) {
        // workgroup-resident copy of the lattice tables, this role's half of it (as in step16_one)
        const float4* src = reinterpret_cast<const float4*>(M.tables);
        float4* dst = reinterpret_cast<float4*>(lds);
        constexpr int NV = TB_WORDS / 4, PER = (NV + NT - 1) / NT;
        float4 tmp[PER];
        int tix = threadIdx.x;
        asm volatile("" : "+v"(tix));                                   // (keeps the copy's addresses from being formed ahead of the step loop and carried, spilled, through every step)
#pragma unroll
        for (int i = 0; i < PER; ++i) { int idx = tix + i * NT; tmp[i] = (idx < NV) ? src[idx] : make_float4(0, 0, 0, 0); }
#pragma unroll
        for (int i = 0; i < PER; ++i) { int idx = tix + i * NT; if (idx < NV) dst[idx] = tmp[i]; }
        USIM_BAR();
    }
    // (`sub`, the physics substep of this pass: step16_one)
    if (sub == 0) t += 1;
    const int tphys = (t - 1) * C.substeps + sub;                       // physics steps since the episode began (prescribed torso drop)
    const float dt = C.dt;
#if defined(USIM_TSTAMP) || defined(USIM_TSTAMP_NOWAIT)
#define RSTAMP(k) do { if (dbg && blockIdx.x == 0 && (threadIdx.x & (64 * WPR - 1)) == 0) dbg[30 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define RSTAMP(k) do { } while (0)
#endif
#define XSTAMP(k) RSTAMP(20 + (k))                                  /* dbg[50 ..] */
    RSTAMP(0);
    if constexpr (LA) __builtin_amdgcn_s_setprio(1);                   // (first pass; later ones come here with it raised)
    float* const mb = &lds[mbo];
    float dz, vz, az;
    torso_motion(C, tphys, dz, vz, az);
    if constexpr (LA) {
        // this side owns EB(GE_S): from the state it loaded (first pass), from every integration, and zeros when it adopts a new episode
        if (first_pass) {
#pragma unroll
            for (int i = 0; i < NE; ++i) { const int e = gl + i * G; if (e < N_TOP) EB(GE_S + e) = s_pre[i]; }
        }
    }
    // (LA, not the first pass: this wave comes here straight from integrating the previous pass -- the arm wave may still be in its finish -- and assumes that no
    //  episode of the wave ended)
    lattice_rhs<G, NE>(lds, eb, gl, M, az, kst, kdmp, true, s_pre, sd_pre);
    // The matrix-core solve a~ = Linv rhs needs nothing from the arm side: it runs here, where this wave used to wait for the site pose (hand-off (1)
    // comes when the arm side has finished its kinematics and the broad phase), and leaves only the narrow phase for after the hand-off: one box,
    // 14.38 -> 13.65 us/step at 4096 envs, 20.8 -> 20.2 at 8192 (8-lane groups).  Splitting the product around the hand-off so that both sides reach
    // hand-offs (1) and (2) together (18 / 14 / 21 of the 25 k chunks before it, accumulators live across the barrier) is slower: 13.9 / 14.1 / 13.85,
    // and with 8-lane groups the accumulators of both column sets spill (44 us).
    lattice_solve<G>(lds, eb, gl, gbase);
    RSTAMP(1);
    USIM_BAR();                                                 // (1) the arm side has published the site pose
    RSTAMP(2);
    if constexpr (LA) {
        __builtin_amdgcn_s_setprio(0);
        if (!first_pass) {
            // the arm side's word of the previous pass (written behind its reads of the wrench, read here before this pass's wrench is written): a new episode starts
            // with the lattice at rest, its own parameters and t = 0 -- adopt it (t advances as at the top of the pass: once) and run the two phases again
            const float4 nx = *reinterpret_cast<const float4*>(&mb[MB_W]);
            const bool began = nx.w != 0.f;
            if (__any(began)) {
                if (began) {
                    adopt(nx);
                    if (sub == 0) t += 1;
#pragma unroll
                    for (int i = 0; i < NE; ++i) { const int e = gl + i * G; if (e < N_TOP) EB(GE_S + e) = 0.f; }
                }
                torso_motion(C, (t - 1) * C.substeps + sub, dz, vz, az);
                lattice_rhs<G, NE>(lds, eb, gl, M, az, kst, kdmp, true, s_pre, sd_pre);
                lattice_solve<G>(lds, eb, gl, gbase);
            }
        }
    }
    const f3 xs = mk(mb[MB_POSE], mb[MB_POSE + 1], mb[MB_POSE + 2]), sy = mk(mb[MB_POSE + 3], mb[MB_POSE + 4], mb[MB_POSE + 5]),
             sz = mk(mb[MB_POSE + 6], mb[MB_POSE + 7], mb[MB_POSE + 8]);
    const f3 sxc = cross(sy, sz);
    int nq = __float_as_int(mb[MB_POSE + 10]);
    // the rest of the broad phase (elements G arm_cull_rounds<G>() ..): appended to the arm side's part of the queue
#pragma unroll
    for (int i = arm_cull_rounds<G>(); i < NE; ++i) {
        const int eraw = i * G + gl, e = eraw < N_TOP ? eraw : N_TOP - 1;
        const bool cand = (eraw < N_TOP) && collide_cull(lds, e, M, C, s_pre[i], dz, xs, sz);
        const unsigned gm = (unsigned)(__ballot(cand) >> gbase) & GMASK;
        mb[MB_Q + (cand ? nq + __popc(gm & ((1u << gl) - 1u)) : 99)] = __int_as_float(e);       // (as on the arm side: the spare last word takes the non-candidates)
        nq += __popc(gm);
    }
    group_sync();
#if defined(USIM_TSTAMP) || defined(USIM_TSTAMP_NOWAIT)
    // profiling build: queue length of every environment of the first lattice wave of workgroup 0 (dbg[54 ..]; collide_queue makes max ceil(nq / G) passes over the wave)
    if (dbg && blockIdx.x == 0 && wave == 0 && gl == 0) dbg[54 + ge] = 1ull + (unsigned long long)nq;
#endif
    // narrow phase: the whole queue, against the element positions parked in the environment's block (by the arm side; LA: by this side)
    int nc = 0;
    collide_queue<G>(lds, mb + MB_Q, nq, &EB(GE_CG), gl, gbase, M, C, &EB(GE_S), dz, xs, sxc, sy, sz, nc);
    // The contact list is complete here.  8-lane groups (EARLY) apply the slot rule and form the contact elements and the arm-independent half of every
    // contact row (frame, lever arms, lattice coupling, regulariser) before hand-off (2), while the arm side still forms Lambda^-1; 16-lane groups do it
    // after the hand-off.  One box, kernel us/step: 8-lane groups at 8192 envs 20.19 -> 19.97 (scratch 176 -> 112 bytes per lane); 16-lane groups at 4096
    // envs 13.67 -> 13.82 (same scratch; what moves ahead of the barrier lengthens the path the arm wave waits for) -- only the 8-lane kernel does it.
    constexpr bool EARLY = G == 8;
    ContactRows P;
    // (The early list lives in variables of its own and is adopted after the hand-off.  Forming it in nc / overflow / ncmax / cel directly, with the slot rule as
    //  one lambda called on either side of the barrier, reads better and cost the 8-lane multi-step kernel two more spilled registers, 8 B of scratch and 0.6 % of
    //  the 8192-environment step: DESIGN.md section 10.)
    int nc_early = nc, overflow_early = 0, ncmax_early = 0, cel_early[MAXC];
    if constexpr (EARLY) {
        contact_overflow<G>(lds, eb, gl, gbase, nc_early);
        if (nc_early > MAXC) { overflow_early = 1; nc_early = MAXC; }
        group_sync();
#pragma unroll
        for (int k = MAXC; k >= 1; --k) if (ncmax_early == 0 && __any(nc_early >= k)) ncmax_early = k;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) cel_early[k] = (k < nc_early) ? __float_as_int(EB(GE_CG + k * CG_WORDS + 6)) : 0;
        if (ncmax_early > 0) contact_rows<G>(lds, eb, gl, M, C, nc_early, cel_early, vz, P);
    }
    RSTAMP(3);
    USIM_BAR();                                                 // (2) ... and Lambda^-1, alpha = J qs, vs = J qd
    RSTAMP(4);
    if constexpr (LA) __builtin_amdgcn_s_setprio(1);
    if constexpr (!EARLY) contact_overflow<G>(lds, eb, gl, gbase, nc);
    int overflow = 0;
    if (nc > MAXC) { overflow = 1; nc = MAXC; }
    if constexpr (!EARLY) group_sync();
    XSTAMP(0);
    int ncmax = 0;
    if constexpr (EARLY) { nc = nc_early; overflow = overflow_early; ncmax = ncmax_early; }
    else {
        // the wave's largest count: nc is uniform over a group, so it is the largest of the four groups' (four lane reads and three scalar maxima in place of eight
        // votes with a branch each; the same value)
        static_assert(G == 16, "one lane read per 16-lane group of the wave");
        const int n0 = __builtin_amdgcn_readlane(nc, 0), n1 = __builtin_amdgcn_readlane(nc, 16), n2 = __builtin_amdgcn_readlane(nc, 32), n3 = __builtin_amdgcn_readlane(nc, 48);
        const int n01 = n0 > n1 ? n0 : n1, n23 = n2 > n3 ? n2 : n3;
        ncmax = n01 > n23 ? n01 : n23;
    }
    XSTAMP(1);
    float gf[MAXC], W[6] = {0, 0, 0, 0, 0, 0};
    int cel[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; ++k) { const int ek = __float_as_int(EB(GE_CG + k * CG_WORDS + 6)); gf[k] = 0.f; cel[k] = EARLY ? cel_early[k] : ((k < nc) ? ek : 0); }      // (read, then select: no branch per slot)
    if (ncmax > 0) {
        // 16-byte reads (the opaque mailbox offset hides the alignment that the static_assert at the layout guarantees): row a of Lambda^-1 is words 8 a .. 8 a + a,
        // alpha and vs are the twelve words behind the six rows -- eleven reads instead of 33 words one or two at a time
        float alpha[6], vs[6], Lp[21];
        const float4* const op = reinterpret_cast<const float4*>(&mb[MB_OP]);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const float4 lo = op[2 * a], hi = (a >= 4) ? op[2 * a + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float row[6] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y};
#pragma unroll
            for (int b = 0; b <= a; ++b) Lp[PK(a, b)] = row[b];
        }
        {
            const float4 v0 = op[12], v1 = op[13], v2 = op[14];
            alpha[0] = v0.x; alpha[1] = v0.y; alpha[2] = v0.z; alpha[3] = v0.w; alpha[4] = v1.x; alpha[5] = v1.y;
            vs[0] = v1.z; vs[1] = v1.w; vs[2] = v2.x; vs[3] = v2.y; vs[4] = v2.z; vs[5] = v2.w;
        }
        XSTAMP(2);
        contact_solve<G, EARLY, true>(lds, eb, gl, M, C, nc, ncmax, cel, Lp, alpha, vs, mu, vz, P, W, gf, dbg, cy.wr);
        XSTAMP(3);
    } else warm_clear(cy.wr);                                        // (no contact in the wave: nothing kept)
    if (gl == 0) {
        *reinterpret_cast<float4*>(&mb[MB_W]) = make_float4(W[0], W[1], W[2], W[3]);
        *reinterpret_cast<float4*>(&mb[MB_W + 4]) = make_float4(W[4], W[5], __int_as_float(nc), __int_as_float(overflow));
        // the contacts' elements as this wave holds them (0 beyond the count); the arm wave maps them to shell ids where the launch reports contacts
        static_assert(MAXC == 8, "two 16-byte stores");
        *reinterpret_cast<float4*>(&mb[MB_W + 8]) = make_float4(__int_as_float(cel[0]), __int_as_float(cel[1]), __int_as_float(cel[2]), __int_as_float(cel[3]));
        *reinterpret_cast<float4*>(&mb[MB_W + 12]) = make_float4(__int_as_float(cel[4]), __int_as_float(cel[5]), __int_as_float(cel[6]), __int_as_float(cel[7]));
    }
    RSTAMP(5);
    USIM_BAR();                                                 // (3) contact wrench and contact list published
    RSTAMP(6);
#if defined(USIM_TSTAMP) || defined(USIM_TSTAMP_NOWAIT)
    if (more && dbg && blockIdx.x == 0 && (threadIdx.x & (64 * WPR - 1)) == 0) dbg[62] = __builtin_readcyclecounter();      // hand-off (3) of the pass before the last one
#endif
    {
        float acc_e[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) { const int e = gl + i * G; acc_e[i] = (e < N_TOP) ? EB(GE_A + e) : 0.f; }
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {                              // (every slot, no test against the wave's contact count: slots beyond an environment's count carry gf = 0
                                                                     //  and element 0, and eight uniform branches cost more than the multiply-adds they skip)
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int e = (gl + i * G < N_TOP) ? gl + i * G : N_TOP - 1;
                acc_e[i] = fmaf(lds[TB_LINV + e * LROW + cel[k]], gf[k], acc_e[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int e = gl + i * G;
            if (e >= N_TOP) continue;
            const float sdn = sd_pre[i] + dt * acc_e[i];
            const float sn = s_pre[i] + dt * sdn;
            if (valid) { LAT(LAT_SD + e) = sdn; LAT(LAT_S + e) = sn; }
            if constexpr (RES) { sd_pre[i] = sdn; s_pre[i] = sn; EB(GE_S + e) = sn; }     // resident launch: the next step's state; positions for the arm side's broad phase
        }
        if constexpr (WARM) { if (valid) warm_store(warm_rows, gl, cy.wr); }
    }
    RSTAMP(7);
    if (!LA || !more) USIM_BAR();                               // (4) lattice stored: the arm side may now zero it for an episode that ended (LA: last pass of a launch only)
    RSTAMP(8);
#undef RSTAMP
#undef XSTAMP
#undef LAT
#undef EB
}

// The 16-lane step of the single-wave kernels (ROLE 0: arm and lattice sides in one wave) and of the arm wave of the split kernel (ROLE 1; its lattice / contact wave runs
// lattice_pass, above).
// AHEAD (action drawn ahead; arm side of the split kernel in resident launches that draw their actions): `more` = another pass of this launch follows this one
template <int TORSO, int MODE, int ROLE, int NT, int G = 16, bool RES = false, class WR = NoWarm, bool AHEAD = false>
DI void step16_one(float* lds, const DevModel& M, const DevCfg& C, float* __restrict__ st, const int n, const int npad, const DevIO& io, const int flags, const long long rstep,
                   const bool first_pass, const int sub, const bool more, int& nbar, Carry<TORSO ? (N_TOP + G - 1) / G : 1, WR>& cy) {
    static_assert(ROLE != 2, "the lattice / contact wave of the split kernel runs lattice_pass");
    static_assert(!AHEAD || (ROLE == 1 && RES), "action drawn ahead: the arm wave of a resident split launch");
    // warm start of the contact solve (WR = WarmRec): the side that solves the contacts loads the lane's record of the kept list with the state, hands it to
    // contact_solve and stores the new one with the lattice; the side that restarts an episode clears the environment's warm rows
    constexpr bool WARM = !std::is_same<WR, NoWarm>::value;
    // (MODE 1, the reset launch of such a handle: its zero-torque forward pass solves cold and keeps nothing; it clears the rows of the environments it resets)
    static_assert(!WARM || (TORSO == 1 && ROLE == 0) || (TORSO == 1 && MODE == 0), "warm start: the soft-torso kernels");
    constexpr int WPR = (ROLE != 0) ? SPLIT_WPR : 4;                    // (single-wave kernels: the four waves of a 256-thread workgroup)
    constexpr int EPW = 64 / G, EPB = WPR * EPW;                        // environments per wave / per workgroup (WPR waves per role)
    static_assert(!RES || MODE == 0, "resident state: step launches only");
    constexpr int X2_BASE = x2_base<G>();
    constexpr unsigned GMASK = (G == 16) ? 0xffffu : 0xffu;
    static_assert(G == 16 || (TORSO == 1 && MODE == 0 && ROLE != 0), "8-lane groups: the split soft-torso step only");
    constexpr int NE = TORSO ? (N_TOP + G - 1) / G : 1;
    static_assert(ROLE == 0 || (TORSO == 1 && MODE == 0), "the split kernel is the soft-torso step");
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & (WPR - 1);      // wave within its role = quad of environments
    // resident state (see Carry): every role of a multi-step launch.  (Before the lattice wave of 16-lane groups ran ahead it reloaded its state every pass instead.)
    constexpr bool LA = lattice_ahead<ROLE, G, RES>();
    // The report written late (arm wave of the split kernel, 16-lane groups, resident launches).  Behind hand-off (3) a pass has a STATE part -- what the next pass's
    // kinematics and the lattice wave wait for: the wrench, qacc, the Euler step, the bookkeeping scalars, reward / done / status, the adoption of a bank episode, the
    // new-episode word -- and a REPORT: the probe torque sensor, the observation row, every global store of the transition and the store of the state words.  The arm wave is
    // the late one from hand-off (3) to hand-off (2) of the next pass and idle between (2) and (3), so where another pass follows (`defer`) it parks what the report needs in
    // its own words of the mailbox block (MB_REP) and writes the report in the next pass's wait, before that pass's precompute() and action draw.  The last pass of a
    // launch writes the pending report there and its own in place, as ever; a launch of one pass is the code it was.  Same operands, same operations, same order: same bits.
    constexpr bool DEF = ROLE == 1 && report_late<G, RES>();
    const bool defer = DEF && more;
    const bool fresh = !RES || first_pass;                              // the state comes from HBM (first step of a launch; every single-step launch)
    const int gl = lane & (G - 1), ge = lane / G;
    const int gbase = lane - gl;
    const int eb = wave * EPW + ge;
    const bool auto_reset = (flags & LF_AUTO_RESET) != 0;
    unsigned long long* const dbg = io.dbg;
    // refill launches walk the work list with a grid-stride loop; every other launch runs the body once
    const bool refill = (MODE == 1) && io.refill != 0;
    const int item_cnt = refill ? io.count[0] : 1;
    const int item_first = refill ? (int)blockIdx.x * EPB : 0;
    for (int item0 = item_first; item0 < item_cnt; item0 += refill ? (int)gridDim.x * EPB : 1) {
    int env = blockIdx.x * EPB + eb;
    bool valid = env < n;
    int item_ep = 0;
    if (refill) {
        valid = item0 + eb < item_cnt;
        const int2 it = valid ? io.items[item0 + eb] : make_int2(0, 0);
        env = it.x; item_ep = it.y;
    }
    const bool store = valid && gl == 0;
    const int ei = valid ? env : (refill ? 0 : n - 1);              // clamp so that every lane has something to read; stores are guarded
#define LAT(w) st[(size_t)F_LAT * npad + (size_t)ei * LAT_ENV_WORDS + (w)]
#define EB(off) lds[TB_WORDS + eb * GE_STRIDE + (off)]
    float* const warm_rows = st + warm_index(io.bank_row0, npad, (size_t)ei);      // (dereferenced by handles with warm rows only)
    // The mailbox block sits beyond the 64 KB an LDS instruction's immediate offset reaches.  Left to itself the compiler forms one address register per mailbox WORD
    // (block + constant, hoisted out of the step loop) and spills them around the contact solve: 74 registers, two scratch round trips per step in the resident
    // kernel.  The block's offset is therefore made opaque: one address register, the words at immediate offsets from it.
    int mbo = X2_BASE + eb * x2_stride<ROLE != 0 && report_late<G, RES>()>();
    if constexpr (ROLE != 0) asm volatile("" : "+v"(mbo));
    float* const xl = (ROLE != 0) ? &lds[mbo]
                                  : (TORSO ? &lds[TB_WORDS + eb * GE_STRIDE + GE_WS] : &lds[eb * X16_RIGID_STRIDE]);   // transpose scratch of this environment
    static_assert(GE_WS + X16_WORDS <= GE_STRIDE, "transpose scratch overlays the wrench records");
    // `fixed`-mode goal held across physics substeps: split kernel -- in the mailbox block; single wave, soft torso -- the last 12 words of the environment's
    // block, behind the spare contact record; rigid torso -- behind the transpose scratch
    constexpr int GOAL_OFF = (ROLE != 0) ? MB_GOAL : (TORSO ? GE_CG + (MAXCAND + 1) * CG_WORDS - GE_WS : X16_WORDS);
    static_assert(GE_CG + (MAXCAND + 1) * CG_WORDS + 12 <= GE_STRIDE && X16_WORDS + 12 <= X16_RIGID_STRIDE, "room for the goal");
    float* const goal_lds = xl + GOAL_OFF;

    USIM_STAMP(dbg, 0);
    if constexpr (ROLE == 1) { if (dbg && blockIdx.x == 0 && threadIdx.x == 0) dbg[20] = __builtin_readcyclecounter(); }

    // ---------------- load: this lane's link record, its joint state, the environment's scalars ----------------
    float at[AT_STRIDE];
    {
        constexpr int ARM_LDS = arm_lds_base<TORSO, ROLE, G, RES>();
        const float4* ap = fresh ? reinterpret_cast<const float4*>(M.tables + TB_ARM + gl * AT_STRIDE) : reinterpret_cast<const float4*>(lds + ARM_LDS + gl * AT_STRIDE);
        if (fresh) {
#pragma unroll
            for (int v = 0; v < AT_STRIDE / 4; ++v) { const float4 x = ap[v]; at[4 * v] = x.x; at[4 * v + 1] = x.y; at[4 * v + 2] = x.z; at[4 * v + 3] = x.w; }
            if constexpr (RES) {
                // (every wave writes the same words and reads them back itself: no hand-off involved)
                if (lane < G) {
#pragma unroll
                    for (int v = 0; v < AT_STRIDE / 4; ++v) reinterpret_cast<float4*>(lds + ARM_LDS + gl * AT_STRIDE)[v] = make_float4(at[4 * v], at[4 * v + 1], at[4 * v + 2], at[4 * v + 3]);
                }
            }
        } else {
            const float4* lp = reinterpret_cast<const float4*>(lds + ARM_LDS + gl * AT_STRIDE);
#pragma unroll
            for (int v = 0; v < AT_STRIDE / 4; ++v) { const float4 x = lp[v]; at[4 * v] = x.x; at[4 * v + 1] = x.y; at[4 * v + 2] = x.z; at[4 * v + 3] = x.w; }
        }
    }
    const float* const sp = st + scalar_index(0, (size_t)ei);
    const bool jlane = at[AT_JOINT] != 0.f;                       // lanes that own a joint (a chain of fewer than seven joints pads with locked ones)
    const int jl = jlane ? gl : NJ - 1;
    // the joint words of the state hold dq = q - q0 (usim_device.h): the per-step increment dt qd is then rounded at the magnitude of the
    // excursion (~0.05 rad), not of the angle (~3 rad) -- the rounding of q would otherwise accumulate to micrometres at the probe over 200 steps
    float &dqj = cy.dqj, &qdj = cy.qdj, &q0j = cy.q0j;
    Episode& E = cy.ep;
    f3 &ts = E.ts, &te = E.te;
    float &u0 = E.u0, &vbar = E.vbar, &fzbar = E.fzbar, &fzprev = E.fzprev, &dfz = E.dfz, &kst = E.kst, &kdmp = E.kdmp, &mu = E.mu, &epret = E.epret;
    int &t = E.t, &touched = E.touched, &episode = E.episode, &status = E.status;
    float (&s_pre)[NE] = cy.s, (&sd_pre)[NE] = cy.sd;
    if (fresh) {
        dqj = sp[F_Q + jl]; qdj = sp[F_QD + jl]; q0j = sp[F_Q0 + jl];
        float sv[20];                                              // scalar words 20 .. 39
        {
            const float4* s4 = reinterpret_cast<const float4*>(sp + 20);
#pragma unroll
            for (int v = 0; v < 5; ++v) { const float4 x = s4[v]; sv[4 * v] = x.x; sv[4 * v + 1] = x.y; sv[4 * v + 2] = x.z; sv[4 * v + 3] = x.w; }
        }
#define SV(f) sv[(f) - 20]
        ts = mk(SV(F_TS), SV(F_TS + 1), SV(F_TS + 2)); te = mk(SV(F_TE), SV(F_TE + 1), SV(F_TE + 2));
        u0 = SV(F_U0); vbar = SV(F_VBAR); fzbar = SV(F_FZBAR); fzprev = SV(F_FZPREV); dfz = SV(F_DFZ);
        kst = SV(F_KST); kdmp = SV(F_KDMP); mu = SV(F_MU); epret = SV(F_EPRET);
        t = __float_as_int(SV(F_T)); touched = __float_as_int(SV(F_TOUCH)); episode = __float_as_int(SV(F_EPISODE)); status = __float_as_int(SV(F_STATUS));
#undef SV
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int e = gl + i * G;
            s_pre[i] = 0.f; sd_pre[i] = 0.f;
            if (TORSO && MODE == 0 && ROLE == 0 && e < N_TOP) { s_pre[i] = LAT(LAT_S + e); sd_pre[i] = LAT(LAT_SD + e); }
            if (TORSO && MODE == 0 && ROLE == 1 && !LA && e < N_TOP) s_pre[i] = LAT(LAT_S + e);      // the arm side parks the positions for the narrow phase and, with 8-lane groups, culls on them (LA: the lattice side does both)
        }
        if constexpr (WARM && MODE == 0 && ROLE == 0) warm_load(warm_rows, gl, cy.wr);
    } else if constexpr (RES && ROLE == 1 && !LA) {
        // resident launch, arm side of 8-lane groups (the only one that culls): the element positions the lattice side integrated (or the zeros this side left
        // for a new episode) are in the environment's LDS block
#pragma unroll
        for (int i = 0; i < NE; ++i) { const int e = gl + i * G; s_pre[i] = (e < N_TOP) ? EB(GE_S + e) : 0.f; }
    }
    if (!jlane) { dqj = 0.f; qdj = 0.f; q0j = 0.f; }
    float qj = q0j + dqj;
    if (TORSO != 0 && item0 == item_first && first_pass) {
        // workgroup-resident copy of the lattice tables: 16-byte loads, all issued before the first LDS store (and behind the state loads
        // above, whose HBM latency the copy then covers)
        const float4* src = reinterpret_cast<const float4*>(M.tables);
        float4* dst = reinterpret_cast<float4*>(lds);
        constexpr int NV = TB_WORDS / 4, PER = (NV + NT - 1) / NT;
        float4 tmp[PER];
        int tix = threadIdx.x;
        asm volatile("" : "+v"(tix));                                   // (keeps the copy's addresses from being formed ahead of the step loop and carried, spilled, through every step)
#pragma unroll
        for (int i = 0; i < PER; ++i) { int idx = tix + i * NT; tmp[i] = (idx < NV) ? src[idx] : make_float4(0, 0, 0, 0); }
#pragma unroll
        for (int i = 0; i < PER; ++i) { int idx = tix + i * NT; if (idx < NV) dst[idx] = tmp[i]; }
        USIM_BAR();
    }
    USIM_STAMP(dbg, 1);

    // robosuite MujocoEnv.step [RESTATED, SURVEY C.1]: timestep += 1 once, then int(control_timestep / model_timestep) physics substeps (controller
    // torque from the current state with the policy step's goal and gains, mj_step), then _post_action once.  `sub` is the substep of this pass
    // (multi-step kernels only; C.substeps = 1 with the shipped control_freq 500): every pass integrates and stores the state, the last one of a
    // control step evaluates reward / bookkeeping / termination and writes the transition.
    if (MODE == 0 && sub == 0) t += 1;
    const bool last_sub = sub == C.substeps - 1;
    const int tphys = (MODE == 0) ? (t - 1) * C.substeps + sub : 0;     // physics steps since the episode began (prescribed torso drop)
    const float dt = C.dt, inv_h = rcp_((float)C.horizon);
#if defined(USIM_TSTAMP) || defined(USIM_TSTAMP_NOWAIT)
#define RSTAMP(k) do { if (dbg && blockIdx.x == 0 && (threadIdx.x & (64 * WPR - 1)) == 0) dbg[20 + (k)] = __builtin_readcyclecounter(); } while (0)      /* arm wave of the split kernel (lattice_pass: dbg[30 ..]) */
#else
#define RSTAMP(k) do { } while (0)
#endif
    const int comp = gl & 3;                                             // task lanes: component of the position (quad 0) / orientation (quad 1) block
    const bool blk = (gl & 4) != 0;
    const bool is_task = (gl < 8) && comp != 3;
    auto pick = [&](f3 v) { return comp == 0 ? v.x : (comp == 1 ? v.y : v.z); };

    bool need = false;                                                   // MODE 1: environments that (re)initialise
    int ep_t = episode;                                                  // episode index the reset draws are keyed on
    if constexpr (MODE == 1) {
        need = refill ? valid : (io.mask ? io.mask[ei] != 0 : true);
        if (!__any(need)) continue;
        // ================= reset draws (ultrasound.py:416-478): the three counter blocks side by side in lanes 0, 1, 2 =================
        ep_t = refill ? item_ep : episode + 1;                           // listed bank episode, or the live reset
        if (!refill) episode = ep_t;
        const uint32_t gid = (uint32_t)(C.env_offset + ei);
        const u4 r = philox(gid, (uint32_t)ep_t, (uint32_t)(gl < 3 ? gl : 2), 0u, C.key0, C.key1);
        const float ra = __uint_as_float(r.a), rb = __uint_as_float(r.b), rc = __uint_as_float(r.c), rd = __uint_as_float(r.d);
        u4 A, B, Cc;
        A.a = __float_as_uint(rbc<G, 0>(ra)); A.b = __float_as_uint(rbc<G, 0>(rb)); A.c = __float_as_uint(rbc<G, 0>(rc)); A.d = __float_as_uint(rbc<G, 0>(rd));
        B.a = __float_as_uint(rbc<G, 1>(ra)); B.b = __float_as_uint(rbc<G, 1>(rb)); B.c = __float_as_uint(rbc<G, 1>(rc)); B.d = __float_as_uint(rbc<G, 1>(rd));
        Cc.a = __float_as_uint(rbc<G, 2>(ra)); Cc.b = __float_as_uint(rbc<G, 2>(rb)); Cc.c = __float_as_uint(rbc<G, 2>(rc)); Cc.d = __float_as_uint(rbc<G, 2>(rd));
        const float tz = M.torso[2] + M.base[2] + C.top_off;             // ultrasound.py:184,807
        f3 noise = mk(0, 0, 0);
        kst = C.stiffness; kdmp = C.damping;
        if (io.reset_params) {
            const float* p = io.reset_params + (size_t)ei * 13;
            ts = mk(p[0], p[1], p[2]); te = mk(p[3], p[4], p[5]); u0 = p[6]; noise = mk(p[7], p[8], p[9]);
            kst = p[10]; kdmp = p[11]; mu = p[12];
        } else {
            if (C.det_traj) { ts = mk(0.062f, -0.020f, 0.896f); te = mk(-0.032f, -0.075f, 0.896f); }   // ultrasound.py:763-764
            else {
                // ultrasound.py:787-788: np.linspace grids over the torso top, 50 points each
                const float tx = M.torso[0] + M.base[0], ty = M.torso[1] + M.base[1];
                const float xs0 = -0.15f + tx + 0.03f, xstep = (0.15f + tx - xs0) / 49.f;
                const float ys0 = -C.y_range + ty, ystep = 2.f * C.y_range / 49.f;
                ts = mk(xs0 + (float)urange(A.a, 50u) * xstep, ys0 + (float)urange(A.b, 50u) * ystep, tz);
                te = mk(xs0 + (float)urange(A.c, 50u) * xstep, ys0 + (float)urange(A.d, 50u) * ystep, tz);
            }
            u0 = u01(B.a);                                               // ultrasound.py:443
            if (C.rand_pos) {                                            // ultrasound.py:880-881
                const float r1 = sqrtf(-2.f * logf(u01_open(B.b))), th1 = 2.f * PI_F * u01(B.c);
                const float r2 = sqrtf(-2.f * logf(u01_open(B.d))), th2 = 2.f * PI_F * u01(Cc.a);
                noise = mk(r1 * cosf(th1) * 0.0025f, r1 * sinf(th1) * 0.0025f, r2 * cosf(th2) * 0.010f);
            }
            if (C.rand_solref) { kst = 1300.f + (float)urange(Cc.b, 300u); kdmp = 17.f + (float)urange(Cc.c, 24u); }   // ultrasound.py:293-294
            float pf = C.probe_fric;
            if (C.rand_fric) pf *= 0.5f + 1.5f * u01(Cc.d);
            mu = fmaxf(pf, C.elem_fric);
            if (C.probe_geoms == 2 && !C.pair) mu = 0.5f * (mu + fmaxf(C.probe_fric2, C.elem_fric));   // two coincident contacts per pair restated as one (usim_config.probe_geoms)
        }
        // ================= initial pose: damped-least-squares IK from init_qpos (ultrasound.py:812-844) =================
        const float uu = clampf(u0, 0.f, 1.f);
        const f3 tp0 = ts + (te - ts) * uu;
        const f3 target = mk(tp0.x + noise.x + M.ikb[0] - M.base[0], tp0.y + noise.y + M.ikb[1] - M.base[1], tp0.z + noise.z + M.ikb[2] - M.base[2]);
        const f3 gx = mk(M.grot[0], M.grot[3], M.grot[6]), gy = mk(M.grot[1], M.grot[4], M.grot[7]), gz = mk(M.grot[2], M.grot[5], M.grot[8]);
        qj = jlane ? at[AT_INITQ] : 0.f;
        for (int it = 0; it < C.ik_iters; ++it) {
            f3 X, Y, Z, P;
            fk16<G>(at, qj, X, Y, Z, P);
            const f3 sx = rbc3<G, 7>(X), sy = rbc3<G, 7>(Y), sz = rbc3<G, 7>(Z), xs = rbc3<G, 7>(P);
            const f3 eo = (cross(sx, gx) + cross(sy, gy) + cross(sz, gz)) * 0.5f;
            const f3 ep = target - xs;
            const float e = is_task ? (blk ? pick(eo) : pick(ep)) : 0.f;
            const f3 jv = cross(Z, xs - P);
            const float Jc[6] = {jlane ? jv.x : 0.f, jlane ? jv.y : 0.f, jlane ? jv.z : 0.f, jlane ? Z.x : 0.f, jlane ? Z.y : 0.f, jlane ? Z.z : 0.f};
            float Jr[8];
            jacobian_rows(xl, gl, Jc, Jr);
            // (J J^T + 1e-6 I) y = e, row a in task lane a
            float A6[6];
            static_for<6>([&](auto Bc) {
                constexpr int b = decltype(Bc)::value;
                float sacc = 0.f;
                static_for<NJ>([&](auto Jn) { constexpr int j = decltype(Jn)::value; sacc = fmaf(Jr[j], rbc<G, TASK_LANE[b]>(Jr[j]), sacc); });
                A6[b] = is_task ? sacc + ((gl == TASK_LANE[b]) ? 1e-6f : 0.f) : 0.f;
            });
            const float y = solve6_task<G>(A6, e, gl);
            const float dq = col_times_task<G>(Jc, y);
            qj = jlane ? qj + dq : 0.f;
            group_sync();                                                // the scratch is rewritten by the next iteration / the forward pass
        }
        q0j = qj; qdj = 0.f; dqj = 0.f;
        episode_begin(E, 0);
    }

    // =================================================================================================================
    // kinematics: local transform of this lane's link, then the scan  T_l <- T_(l-d) o T_l  for d = 1, 2, 4
    // =================================================================================================================
    f3 X, Y, Z, P;                                                       // world rotation columns and origin of this lane's frame
    fk16<G>(at, qj, X, Y, Z, P);
    const f3 rcm = X * at[AT_LCOM] + Y * at[AT_LCOM + 1] + Z * at[AT_LCOM + 2];      // link COM relative to the link origin
    const f3 cm_ = P + rcm;
    // site frame = lane 7's; hand origin = a fixed point of the last link
    const f3 sx = rbc3<G, 7>(X), sy = rbc3<G, 7>(Y), sz = rbc3<G, 7>(Z), xs = rbc3<G, 7>(P);
    const f3 hand = rbc3<G, NJ - 1>(P + X * M.hand7[0] + Y * M.hand7[1] + Z * M.hand7[2]);
    if constexpr (ROLE == 1) {
        {
            // broad phase of the collision (collide_cull): element ids that can touch the probe, ascending, into the queue; element positions
            // into the environment's LDS block for whoever evaluates them
            float dz_, vz_, az_;
            torso_motion(C, tphys, dz_, vz_, az_);
            int nq = 0;
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int eraw = i * G + gl, e = eraw < N_TOP ? eraw : N_TOP - 1;
                if (!LA && eraw < N_TOP) EB(GE_S + eraw) = s_pre[i];          // (8-lane groups and single-step launches; LA: the lattice side owns the area)
                if (i >= arm_cull_rounds<G>()) continue;
                const bool cand = (eraw < N_TOP) && collide_cull(lds, e, M, C, s_pre[i], dz_, xs, sz);
                const unsigned gm = (unsigned)(__ballot(cand) >> gbase) & GMASK;
                xl[MB_Q + (cand ? nq + __popc(gm & ((1u << gl) - 1u)) : 99)] = __int_as_float(e);     // (a lane without a candidate writes the queue's spare last word -- 99 elements at most are queued --: a store, not a branch)
                nq += __popc(gm);
            }
            if (gl == 0) xl[MB_POSE + 10] = __int_as_float(nq);
        }
        if (gl == 7) {                                                   // the site frame is lane 7's own
            float* mbp = xl + MB_POSE;
            mbp[0] = P.x; mbp[1] = P.y; mbp[2] = P.z; mbp[3] = Y.x; mbp[4] = Y.y; mbp[5] = Y.z; mbp[6] = Z.x; mbp[7] = Z.y; mbp[8] = Z.z;
        }
        if constexpr (ROLE == 1) RSTAMP(1);
        USIM_BAR();                                                 // (1)
        if constexpr (ROLE == 1) RSTAMP(2);
    }

    // ---------------- action (replicated: seven words) ----------------
    float act[7] = {0, 0, 0, 0, 0, 0, 0};
    // the synthetic action of control step `cs` (usim_random_actions_kernel's stream)
    auto draw_action = [&](const long long cs, float (&a7)[7]) {
        // the two counter blocks are evaluated side by side by the even and odd lanes of the group, then shared
        const uint32_t gid = (uint32_t)(C.env_offset + ei);
        const u4 r = philox(gid, (uint32_t)cs, (uint32_t)((unsigned long long)cs >> 32), 1u + (uint32_t)(gl & 1), C.key0, C.key1);
        const float ra = __uint_as_float(r.a), rb = __uint_as_float(r.b), rc = __uint_as_float(r.c), rd = __uint_as_float(r.d);
        uint32_t rr[7];
        rr[0] = __float_as_uint(rbc<G, 0>(ra)); rr[1] = __float_as_uint(rbc<G, 0>(rb)); rr[2] = __float_as_uint(rbc<G, 0>(rc)); rr[3] = __float_as_uint(rbc<G, 0>(rd));
        rr[4] = __float_as_uint(rbc<G, 1>(ra)); rr[5] = __float_as_uint(rbc<G, 1>(rb)); rr[6] = __float_as_uint(rbc<G, 1>(rc));
        // (the decoding of synthetic_action, usim_episode.h, written out: called here it changes the schedule of 7 of the 14 16-lane kernels)
#pragma unroll
        for (int a = 0; a < 7; ++a) {
            const float u = u01(rr[a]);
            const bool sgn = (C.mode == 1) || (C.mode == 3) || (C.mode == 2 && a == 6);
            a7[a] = sgn ? 2.f * u - 1.f : u;
            if (C.mode == 3) a7[a] *= WRENCH_MAX;
        }
    };
    // AHEAD: the arm wave's own words of the mailbox block hold the action of the running control step (the same lanes write and read them)
    auto keep_action = [&](const float (&a7)[7]) {
        if (gl == 0) {
            *reinterpret_cast<float4*>(&xl[MB_ACT]) = make_float4(a7[0], a7[1], a7[2], a7[3]);
            *reinterpret_cast<float4*>(&xl[MB_ACT + 4]) = make_float4(a7[4], a7[5], a7[6], 0.f);
        }
    };
    if constexpr (MODE == 0) {
    if (flags & LF_RANDOM_ACT) {
        if (AHEAD && !first_pass) {
            // drawn during the previous pass of this launch (below, before hand-off (3)), or held over the physics substeps of a control step
            const float4 a0 = *reinterpret_cast<const float4*>(&xl[MB_ACT]), a1 = *reinterpret_cast<const float4*>(&xl[MB_ACT + 4]);
            act[0] = a0.x; act[1] = a0.y; act[2] = a0.z; act[3] = a0.w; act[4] = a1.x; act[5] = a1.y; act[6] = a1.z;
        } else {
            draw_action(rstep, act);
            if constexpr (AHEAD) keep_action(act);                      // (for the later substeps of this control step)
        }
        if (io.act_out && store) {                                      // (one predicated region for the seven stores)
            if constexpr (AHEAD) {
                // adim is 6 or 7 (translate_config) and uniform: six plain stores and one scalar branch, not seven tests
                float* const ao = io.act_out + (size_t)ei * C.adim;
#pragma unroll
                for (int a = 0; a < 6; ++a) ao[a] = act[a];
                if (C.adim > 6) ao[6] = act[6];
            } else {
#pragma unroll
                for (int a = 0; a < 7; ++a) if (a < C.adim) io.act_out[(size_t)ei * C.adim + a] = act[a];
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < 7; ++a) if (a < C.adim) act[a] = finite_or_zero(io.act[(size_t)ei * C.adim + a]);
    }
    }
    // =================================================================================================================
    // dynamics: bias forces (prefix / suffix sums over the joint lanes) and mass matrix (composite inertia by suffix sums)
    // =================================================================================================================
    float bias, Mr[NJ];                                                  // this lane's bias torque and its full row of M
    f3 w, al, ao;                                                        // link angular velocity, bias angular acceleration, bias acceleration of the origin
    {
        const f3 zq = Z * qdj;
        w = prefix_sum<G>(zq);
        const f3 wp = w - zq;                                            // parent link
        const f3 dal = cross(wp, zq);
        al = prefix_sum<G>(dal);
        const f3 alp = al - dal;
        const f3 r = mk(P.x - rshr0<G, 1>(P.x), P.y - rshr0<G, 1>(P.y), P.z - rshr0<G, 1>(P.z));
        f3 da = cross(alp, r) + cross(wp, cross(wp, r));
        da.z += (gl == 0) ? GRAV : 0.f;                                  // gravity enters as the base acceleration
        ao = prefix_sum<G>(da);
        const f3 ac = ao + cross(al, rcm) + cross(w, cross(w, rcm));
        const float mass = at[AT_MASS];
        const f3 F = ac * mass;
        // world inertia Iw = R I R^T (six entries)
        const float* I = &at[AT_INERTIA];
        const f3 RI0 = mk(X.x * I[0] + Y.x * I[1] + Z.x * I[2], X.x * I[1] + Y.x * I[3] + Z.x * I[4], X.x * I[2] + Y.x * I[4] + Z.x * I[5]);   // row x of R I
        const f3 RI1 = mk(X.y * I[0] + Y.y * I[1] + Z.y * I[2], X.y * I[1] + Y.y * I[3] + Z.y * I[4], X.y * I[2] + Y.y * I[4] + Z.y * I[5]);
        const f3 RI2 = mk(X.z * I[0] + Y.z * I[1] + Z.z * I[2], X.z * I[1] + Y.z * I[3] + Z.z * I[4], X.z * I[2] + Y.z * I[4] + Z.z * I[5]);
        float Iw[6];
        Iw[0] = RI0.x * X.x + RI0.y * Y.x + RI0.z * Z.x; Iw[1] = RI0.x * X.y + RI0.y * Y.y + RI0.z * Z.y; Iw[2] = RI0.x * X.z + RI0.y * Y.z + RI0.z * Z.z;
        Iw[3] = RI1.x * X.y + RI1.y * Y.y + RI1.z * Z.y; Iw[4] = RI1.x * X.z + RI1.y * Y.z + RI1.z * Z.z; Iw[5] = RI2.x * X.z + RI2.y * Y.z + RI2.z * Z.z;
        const f3 Nc = symmul(Iw, al) + cross(w, symmul(Iw, w)) + cross(cm_, F);      // moment about the base origin
        const f3 fa = suffix_sum<G>(F), na = suffix_sum<G>(Nc);
        bias = dot(Z, na - cross(P, fa));
        // composite inertia about the base origin: mass, first moment, second moment
        const float cc = dot(cm_, cm_);
        float Io[6] = {fmaf(mass, cc - cm_.x * cm_.x, Iw[0]), fmaf(-mass, cm_.x * cm_.y, Iw[1]), fmaf(-mass, cm_.x * cm_.z, Iw[2]),
                       fmaf(mass, cc - cm_.y * cm_.y, Iw[3]), fmaf(-mass, cm_.y * cm_.z, Iw[4]), fmaf(mass, cc - cm_.z * cm_.z, Iw[5])};
        const float cmass = suffix_sum<G>(mass);
        const f3 ch = suffix_sum<G>(cm_ * mass);
#pragma unroll
        for (int k = 0; k < 6; ++k) Io[k] = suffix_sum<G>(Io[k]);
        const f3 vo = cross(P, Z);
        const f3 nn = symmul(Io, Z) + cross(ch, vo);
        const f3 ff = vo * cmass + cross(Z, ch);
        // lower triangle of row l: M[l][j] = z_j . n_l + vo_j . f_l  (j <= l)
        float Ml[8];
        static_for<NJ>([&](auto Jc) {
            constexpr int j = decltype(Jc)::value;
            Ml[j] = spatial_dot_bc<G, j>(Z, vo, nn, ff);
        });
        Ml[7] = 0.f;
        // upper triangle through LDS: every lane parks its row, then reads its column
        if (gl < 8) {
            *reinterpret_cast<float4*>(&xl[gl * 8]) = make_float4(Ml[0], Ml[1], Ml[2], Ml[3]);
            *reinterpret_cast<float4*>(&xl[gl * 8 + 4]) = make_float4(Ml[4], Ml[5], Ml[6], Ml[7]);
        }
        group_sync();
        const int gc = gl & 7;
#pragma unroll
        for (int j = 0; j < NJ; ++j) Mr[j] = ((j > gl) ? xl[j * 8 + gc] : Ml[j]) + ((j == gl) ? (jlane ? at[AT_ARMATURE] : 1.f) : 0.f);    // rotor inertia on the diagonal (usim_config.armature_scale); padding joint: unit diagonal
        group_sync();                                                    // the scratch is reused for the Jacobian below
    }
    USIM_STAMP(dbg, 2);

    // ---------------- M^-1: in-place Gauss-Jordan, row l in lane l ----------------
    float Mi[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) Mi[j] = Mr[j];
    static_for<NJ>([&](auto Kc) {
        constexpr int k = decltype(Kc)::value;
        const float mk_ = (gl == k) ? 1.f : 0.f;
        const float g = (mk_ - Mi[k]) * rcp_(rbc<G, k>(Mi[k]));           // minus the elimination factor
        Mi[k] = mk_;
        row_axpy_bc7<G, k>(Mi, g);
    });

    // ---------------- operational space: Jacobian column per joint lane, row per task lane, Lambda^-1 row per task lane ----------------
    float Jc[6], Jr[8], Li[6], Xm[6];                                    // Xm: row l of M^-1 J^T
    {
        const f3 jv = cross(Z, xs - P);
        Jc[0] = jv.x; Jc[1] = jv.y; Jc[2] = jv.z; Jc[3] = Z.x; Jc[4] = Z.y; Jc[5] = Z.z;
#pragma unroll
        for (int a = 0; a < 6; ++a) Jc[a] = jlane ? Jc[a] : 0.f;         // no column for padding / site / idle lanes
#pragma unroll
        for (int a = 0; a < 6; ++a) Xm[a] = row_times_joint<G, NJ>(Mi, Jc[a]);
        jacobian_rows(xl, gl, Jc, Jr);
#pragma unroll
        for (int b = 0; b < 6; ++b) Li[b] = row_times_joint<G, NJ>(Jr, Xm[b]);
    }
    const float v6 = row_times_joint<G, NJ>(Jr, qdj);                       // site twist component of this task lane
    USIM_STAMP(dbg, 3);

    // ---------------- OSC_POSE torque (robosuite osc.py run_controller; rl_config.yaml:33-51) ----------------
    float tau = 0.f;                                                     // reset: sim.forward() with zero ctrl
    if constexpr (MODE == 0) {
        const int arow = blk ? 3 + (comp > 2 ? 2 : comp) : (comp > 2 ? 2 : comp);
        float act_own = act[0];
#pragma unroll
        for (int a = 1; a < 6; ++a) act_own = (arow == a) ? act[a] : act_own;
        f3 gpos, gx, gy, gz;
        float kp, kd;
        const float up = clampf((float)(t - 1) * inv_h + u0, 0.f, 1.f);     // controller.traj_pos from the previous _post_action
        const f3 tpw = ts + (te - ts) * up;
        if (C.mode == 1) {
            float d[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) d[a] = clampf(act[a], -1.f, 1.f) * (a < 3 ? C.out_pos : C.out_ori);
            gpos = xs + mk(d[0], d[1], d[2]);
            const float ang = sqrt_(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
            if (ang < 1e-12f) { gx = sx; gy = sy; gz = sz; }
            else {
                const float hh = 0.5f * ang, sh = sinf(hh) * rcp_(ang), qw = cosf(hh), qx = d[3] * sh, qy = d[4] * sh, qz = d[5] * sh;
                const f3 e0 = mk(1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy + qw * qz), 2.f * (qx * qz - qw * qy));
                const f3 e1 = mk(2.f * (qx * qy - qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz + qw * qx));
                const f3 e2 = mk(2.f * (qx * qz + qw * qy), 2.f * (qy * qz - qw * qx), 1.f - 2.f * (qx * qx + qy * qy));
                gx = e0 * sx.x + e1 * sx.y + e2 * sx.z; gy = e0 * sy.x + e1 * sy.y + e2 * sy.z; gz = e0 * sz.x + e1 * sz.y + e2 * sz.z;
            }
            kp = C.kp_fixed;
            if (C.substeps > 1) {
                // SingleArm.control: `if policy_step: controller.set_goal(action)` -- the goal is anchored at the first physics substep of a control
                // step and held for the others: parked in the environment's LDS block (same lanes write and read it)
                if (sub == 0) {
                    if (gl == 0) {
                        goal_lds[0] = gpos.x; goal_lds[1] = gpos.y; goal_lds[2] = gpos.z; goal_lds[3] = gx.x; goal_lds[4] = gx.y; goal_lds[5] = gx.z;
                        goal_lds[6] = gy.x; goal_lds[7] = gy.y; goal_lds[8] = gy.z; goal_lds[9] = gz.x; goal_lds[10] = gz.y; goal_lds[11] = gz.z;
                    }
                } else {
                    gpos = mk(goal_lds[0], goal_lds[1], goal_lds[2]); gx = mk(goal_lds[3], goal_lds[4], goal_lds[5]);
                    gy = mk(goal_lds[6], goal_lds[7], goal_lds[8]); gz = mk(goal_lds[9], goal_lds[10], goal_lds[11]);
                }
            }
        } else {
            const float v = (C.mode == 3) ? 0.f : clampf(act_own, 0.f, 1.f);   // wrench mode: no impedance term
            kp = C.kp_min + v * (C.kp_max - C.kp_min);
            gpos = mk(tpw.x - M.base[0], tpw.y - M.base[1], tpw.z - M.base[2]);
            if (C.mode == 2) gpos.z += clampf(act[6], -1.f, 1.f) * C.out_pos;
            gx = mk(M.grot[0], M.grot[3], M.grot[6]); gy = mk(M.grot[1], M.grot[4], M.grot[7]); gz = mk(M.grot[2], M.grot[5], M.grot[8]);
        }
        kd = 2.f * sqrt_(kp) * C.damping_ratio;
        const f3 eo = (cross(sx, gx) + cross(sy, gy) + cross(sz, gz)) * 0.5f;
        const f3 ep = gpos - xs;
        const float e = blk ? pick(eo) : pick(ep);
        float F = e * kp - v6 * kd;
        // fork-only "wrench" baseline (utils/plot.py:267-268): the action takes the place of desired_force / desired_torque in the OSC law
        if (C.mode == 3) F = clampf(act_own, -WRENCH_MAX, WRENCH_MAX);
        // lambda_pos F, lambda_ori T (uncouple_pos_ori, rl_config.yaml:48): Gauss-Jordan on [B | F] inside the quads; lanes that own no
        // task row carry unit rows so that every quad has regular pivots
        float B[3], rhs = is_task ? F : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) B[c] = is_task ? (blk ? Li[3 + c] : Li[c]) : (comp == c ? 1.f : 0.f);
        static_for<3>([&](auto Kc) {
            constexpr int k = decltype(Kc)::value;
            const float g = (B[k] - (comp == k ? 1.f : 0.f)) * rcp_(qbc<k>(B[k]));
#pragma unroll
            for (int c = k + 1; c < 3; ++c) B[c] = fmaf(-g, qbc<k>(B[c]), B[c]);
            rhs = fmaf(-g, qbc<k>(rhs), rhs);
        });
        const float wr = rhs;
        // nullspace torque N^T M (10 (q0 - q) - 2 sqrt(10) qd) = M pt - J^T Lambda (J pt)
        const float pt = 10.f * (q0j - qj) - 6.3245553203367586f * qdj;
        float y = 0.f, jb = 0.f;
        y = row_times_joint<G, NJ>(Mr, pt); jb = row_times_joint<G, NJ>(Jr, pt);
        float A[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) A[c] = is_task ? Li[c] : 0.f;       // lanes without a task row: zero rows, never pivots
        jb = solve6_task<G>(A, is_task ? jb : 0.f, gl);
        const float tq_ = bias + y + col_times_task<G>(Jc, wr - jb);
        tau = clampf(tq_, -at[AT_TAUMAX], at[AT_TAUMAX]);
    }
    if (MODE == 0 && io.log && valid) {
        float* L = io.log + (size_t)ei * LOG_WIDTH;
        if (jlane) L[33 + gl] = tau;
        if (gl == 0) {
#pragma unroll
            for (int a = 0; a < 7; ++a) L[46 + a] = act[a];
        }
    }
    USIM_STAMP(dbg, 4);

    // ---------------- smooth acceleration, site-space acceleration of the unconstrained arm ----------------
    float qs = row_times_joint<G, NJ>(Mi, tau - bias - JOINT_DAMP * qdj);
    if (C.frictionloss > 0.f) {
        // joint dry friction (usim_devmath.h joint_friction, oracle joint_friction): joint by joint, A_ii ~ 1 / M_ii
        float mdiag = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) mdiag = (j == gl) ? Mr[j] : mdiag;
        const float tf = jlane ? clampf(-FRIC_D0 * mdiag * fmaf(FRIC_B, qdj, qs), -C.frictionloss, C.frictionloss) : 0.f;
        qs += row_times_joint<G, NJ>(Mi, tf);
    }
    const float alpha_t = row_times_joint<G, NJ>(Jr, qs);                   // site acceleration of the unconstrained arm, component of this task lane
    // ---- everything of the sensor / observation / reward that does not depend on the contact forces.  The split kernel evaluates it while
    //      the lattice side solves the contacts; the single-wave kernels evaluate it at the same place in the arithmetic, so all variants
    //      compute the same numbers ----
    f3 s_rc, s_wwrc, s_nw, s_arm, s_xso;                                 // probe sensor: COM offset, centripetal term, gyroscopic moment, lever arm, site - origin
    float qe[4], obs[OBS_DIM], pos_err_norm = 0.f, pos_rew = 0.f, ori_err = 0.f, ori_rew = 0.f, vel_rew = 0.f, force_e = 0.f, dforce_e = 0.f;
    f3 xw, tpw;
    auto rot_inertia = [&](f3 v) {
        const f3 l = mk(dot(X, v), dot(Y, v), dot(Z, v));
        const f3 tt = symmul(M.pI7, l);
        return X * tt.x + Y * tt.y + Z * tt.z;
    };
    auto precompute = [&]() {
        s_rc = X * M.pcom7[0] + Y * M.pcom7[1] + Z * M.pcom7[2];
        s_wwrc = cross(w, cross(w, s_rc));
        s_nw = cross(w, rot_inertia(w));
        s_xso = xs - P;
        s_arm = s_rc - s_xso;
        const int tprev = (MODE == 0) ? t - 1 : 0;
        const float up = clampf((float)tprev * inv_h + u0, 0.f, 1.f);
        tpw = ts + (te - ts) * up;
        xw = mk(xs.x + M.base[0], xs.y + M.base[1], xs.z + M.base[2]);
        obs[12] = xw.x - tpw.x; obs[13] = xw.y - tpw.y; obs[14] = xw.z - tpw.z;
        mat2quat_xyzw(sx, sy, sz, qe);
        difference_quat(qe, M.gquat, obs + 15);                          // xyzw arrays through the wxyz routine (ultrasound.py:390)
        if constexpr (MODE == 0) {
            float pe0 = 90.f * (xw.x - tpw.x), pe1 = 90.f * (xw.y - tpw.y);
            pe0 *= pe0; pe1 *= pe1;
            pos_err_norm = sqrt_(pe0 * pe0 + pe1 * pe1);
            pos_rew = 5.f * exp_(-pos_err_norm);
            const float qc[4] = {qe[3], qe[0], qe[1], qe[2]};
            ori_err = 0.2f * distance_quat_goal(qc, M.ghat, M.geps);
            ori_rew = exp_(-ori_err);
            float ve = 45.f * (vbar - 0.04f); ve *= ve;
            vel_rew = exp_(-ve);
            float fe = 0.7f * (fzbar - 5.f); fe *= fe;
            force_e = 3.f * exp_(-fe);
            float de = 0.01f * dfz; de *= de;
            dforce_e = 2.f * exp_(-de);
        }
    };
    float W[6] = {0, 0, 0, 0, 0, 0};
    int ncon = 0, overflow = 0, con_shell[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; ++k) con_shell[k] = -1;
    if constexpr (ROLE == 1) {
        // hand Lambda^-1 (row a from task lane a), alpha = J qs and vs = J qd to the lattice side; take the contact wrench back
        if (is_task) {
            const int arow = blk ? 3 + comp : comp;
            float* mbo = xl + MB_OP;
            *reinterpret_cast<float4*>(&mbo[arow * 8]) = make_float4(Li[0], Li[1], Li[2], Li[3]);
            mbo[arow * 8 + 4] = Li[4]; mbo[arow * 8 + 5] = Li[5];
            mbo[48 + arow] = alpha_t; mbo[54 + arow] = v6;
        }
        RSTAMP(3);
        USIM_BAR();                                                 // (2)
        RSTAMP(4);
        if constexpr (DEF) {
            if (!first_pass) {
                // ================= the report of the pass before (see DEF above), from the words it parked and the state words this wave still holds =================
                const float* const rp = xl + MB_REP;
                const bool tr = sub == 0;                                // that pass completed a control step: a transition is pending (and this pass has advanced t)
                const float4* const wk = reinterpret_cast<const float4*>(&rp[REP_W]);
                const float4 w0 = wk[0], w1 = wk[1], w2 = wk[2], w3 = wk[3];
                const int pflags = tr ? __float_as_int(w3.y) : 0;
                const bool pdone = (pflags & 1) != 0, pneed = (pflags & 2) != 0;
                if (tr) {
                    // the rows of that pass: one rollout row back where the launch writes a block (step16_body moved `io` on)
                    float* p_obs = io.obs; float* p_rew = io.rew; uint8_t* p_done = io.done; float* p_term = io.term_obs; int* p_con = io.contacts;
                    float* p_ret = io.ep_ret; int* p_len = io.ep_len;
                    if (io.block) {
                        const size_t rows = (size_t)n;
                        p_obs -= rows * OBS_DIM; p_rew -= rows; p_done -= rows;
                        if (p_term) p_term -= rows * OBS_DIM;
                        if (p_con) p_con -= rows * (1 + MAXC);
                        if (p_ret) p_ret -= rows;
                        if (p_len) p_len -= rows;
                    }
                    // probe torque sensor: the last link's lane's operands, read by every lane of the group
                    const float4* const lk = reinterpret_cast<const float4*>(&rp[REP_LINK]);
                    const float4 k0 = lk[0], k1 = lk[1], k2 = lk[2], k3 = lk[3], k4 = lk[4], k5 = lk[5], k6 = lk[6], k7 = lk[7];
                    const f3 p_al = mk(k0.x, k0.y, k0.z), p_ao = mk(k0.w, k1.x, k1.y), p_xso = mk(k1.z, k1.w, k2.x), p_rc = mk(k2.y, k2.z, k2.w), p_wwrc = mk(k3.x, k3.y, k3.z);
                    const f3 p_nw = mk(k3.w, k4.x, k4.y), p_arm = mk(k4.z, k4.w, k5.x), pX = mk(k5.y, k5.z, k5.w), pY = mk(k6.x, k6.y, k6.z), pZ = mk(k6.w, k7.x, k7.y);
                    const float4* const sk = reinterpret_cast<const float4*>(&rp[REP_SITE]);
                    const float4 s0 = sk[0], s1 = sk[1], s2 = sk[2], s3 = sk[3], s4 = sk[4];
                    const f3 p_sx = mk(s0.x, s0.y, s0.z), p_sy = mk(s0.w, s1.x, s1.y), p_sz = mk(s1.z, s1.w, s2.x);
                    const float4 q0 = *reinterpret_cast<const float4*>(&rp[REP_AQ]), q1 = *reinterpret_cast<const float4*>(&rp[REP_AQ + 4]);
                    const f3 alq = mk(q0.w, q1.x, q1.y);
                    const f3 alt = p_al + alq;
                    const f3 a7 = p_ao + mk(q0.x, q0.y, q0.z) - cross(alq, p_xso);
                    const f3 ac = a7 + cross(alt, p_rc) + p_wwrc;
                    const f3 il = mk(dot(pX, alt), dot(pY, alt), dot(pZ, alt));      // (rot_inertia on the parked frame)
                    const f3 it = symmul(M.pI7, il);
                    const f3 N = (pX * it.x + pY * it.y + pZ * it.z) + p_nw;
                    const f3 Fp = ac * PROBE_MASS;
                    const f3 tw = N + cross(p_arm, Fp) - mk(w0.w, w1.x, w1.y);
                    const float po[OBS_DIM] = {w0.x, w0.y, w0.z, dot(p_sx, tw), dot(p_sy, tw), dot(p_sz, tw), w1.z, w1.w, w2.x, s2.y, s2.z, s2.w,
                                               s3.x, s3.y, s3.z, s3.w, s4.x, s4.y, s4.z};
                    if (store) {
                        p_rew[ei] = w2.y;
                        if (io.status_out) io.status_out[ei] = __float_as_int(w3.x);
                        p_done[ei] = pdone ? 1 : 0;
                        if (p_con) {
                            const float4 h0 = *reinterpret_cast<const float4*>(&rp[REP_SHELL]), h1 = *reinterpret_cast<const float4*>(&rp[REP_SHELL + 4]);
                            const int sh[MAXC] = {__float_as_int(h0.x), __float_as_int(h0.y), __float_as_int(h0.z), __float_as_int(h0.w),
                                                  __float_as_int(h1.x), __float_as_int(h1.y), __float_as_int(h1.z), __float_as_int(h1.w)};
                            p_con[(size_t)ei * (1 + MAXC)] = __float_as_int(w3.z);
#pragma unroll
                            for (int k = 0; k < MAXC; ++k) p_con[(size_t)ei * (1 + MAXC) + 1 + k] = sh[k];
                        }
                        if (pdone) {
                            if (p_term) {
#pragma unroll
                                for (int a = 0; a < OBS_DIM; ++a) p_term[(size_t)ei * OBS_DIM + a] = po[a];
                            }
                            if (p_ret) p_ret[ei] = w2.z;
                            if (p_len) p_len[ei] = __float_as_int(w2.w);
                        }
                        if (p_obs) {
                            if (!pneed) {
#pragma unroll
                                for (int a = 0; a < OBS_DIM; ++a) p_obs[(size_t)ei * OBS_DIM + a] = po[a];
                            } else {
                                // the episode ended and the bank's next one was adopted (`episode` is its index): its observation
                                const int sl = episode & (BANK_DEPTH - 1);
#pragma unroll
                                for (int a = 0; a < OBS_DIM; ++a) p_obs[(size_t)ei * OBS_DIM + a] = BK(sl, BOBS + a);
                            }
                        }
                    }
                }
                // the state words as that pass left them: nothing has touched them since but t (advanced at the top of a pass that begins a control step)
                if (valid) {
                    float* const so = st + scalar_index(0, (size_t)ei);
                    if (jlane) {
                        so[F_Q + gl] = dqj; so[F_QD + gl] = qdj;
                        if (pneed) so[F_Q0 + gl] = q0j;
                    }
                    if (gl == 0) {
                        float4* s4 = reinterpret_cast<float4*>(so);
                        if (pneed) {
                            so[F_TS] = ts.x; so[F_TS + 1] = ts.y; so[F_TS + 2] = ts.z;
                            s4[6] = make_float4(te.x, te.y, te.z, u0);
                        }
                        s4[7] = make_float4(vbar, fzbar, fzprev, dfz);
                        s4[8] = make_float4(kst, kdmp, mu, __int_as_float(tr ? t - 1 : t));
                        s4[9] = make_float4(__int_as_float(touched), __int_as_float(episode), epret, __int_as_float(status));
                    }
                }
                RSTAMP(29);                                              // dbg[49]: the late report written
            }
        }
        precompute();                                                    // ... while the lattice side solves the contacts
        if constexpr (DEF) {
            if (defer && last_sub) {
                // what this pass's report needs and the contact wrench does not change: parked here, where it costs the chain nothing
                float* const rp = xl + MB_REP;
                if (gl == NJ - 1) {
                    float4* const lk = reinterpret_cast<float4*>(&rp[REP_LINK]);
                    lk[0] = make_float4(al.x, al.y, al.z, ao.x); lk[1] = make_float4(ao.y, ao.z, s_xso.x, s_xso.y); lk[2] = make_float4(s_xso.z, s_rc.x, s_rc.y, s_rc.z);
                    lk[3] = make_float4(s_wwrc.x, s_wwrc.y, s_wwrc.z, s_nw.x); lk[4] = make_float4(s_nw.y, s_nw.z, s_arm.x, s_arm.y); lk[5] = make_float4(s_arm.z, X.x, X.y, X.z);
                    lk[6] = make_float4(Y.x, Y.y, Y.z, Z.x); lk[7] = make_float4(Z.y, Z.z, 0.f, 0.f);
                }
                if (gl == 0) {
                    float4* const sk = reinterpret_cast<float4*>(&rp[REP_SITE]);
                    sk[0] = make_float4(sx.x, sx.y, sx.z, sy.x); sk[1] = make_float4(sy.y, sy.z, sz.x, sz.y);
                    sk[2] = make_float4(sz.z, fzbar - 5.0f, dfz - 0.0f, vbar - 0.04f);      // obs[9 .. 11]: the bookkeeping scalars as the report finds them behind hand-off (3)
                    sk[3] = make_float4(obs[12], obs[13], obs[14], obs[15]); sk[4] = make_float4(obs[16], obs[17], obs[18], 0.f);
                }
            }
        }
        if constexpr (AHEAD) {
            // ... and, in what is left of the wait, the action of the next control step (this pass completes one and another pass of the launch follows; after a
            // substep that does not complete one the kept action stays).  Same counters and decoding as in place: every bit of `act` is what it was.
            if ((flags & LF_RANDOM_ACT) && more && last_sub) {
                float nxt[7];
                draw_action(rstep + 1, nxt);
                keep_action(nxt);
            }
        }
        RSTAMP(5);
        USIM_BAR();                                                 // (3) the lattice side has solved the contacts
        RSTAMP(6);
#if defined(USIM_TSTAMP) || defined(USIM_TSTAMP_NOWAIT)
        if (more && dbg && blockIdx.x == 0 && (threadIdx.x & (64 * WPR - 1)) == 0) dbg[63] = __builtin_readcyclecounter();      // hand-off (3) of the pass before the last one
#endif
        const float4 w0 = *reinterpret_cast<const float4*>(&xl[MB_W]), w1 = *reinterpret_cast<const float4*>(&xl[MB_W + 4]);
        W[0] = w0.x; W[1] = w0.y; W[2] = w0.z; W[3] = w0.w; W[4] = w1.x; W[5] = w1.y;
        ncon = __float_as_int(w1.z); overflow = __float_as_int(w1.w);
        if (io.contacts) {
            // the contact list is reported: the elements the lattice side left behind the wrench (0 beyond the count: in range) -> shell ids (one uniform branch; rollout
            // blocks report none and skip the reads and the look-ups)
            const int* tb_shell = reinterpret_cast<const int*>(lds + TB_SHELL);
            const float4 e0 = *reinterpret_cast<const float4*>(&xl[MB_W + 8]), e1 = *reinterpret_cast<const float4*>(&xl[MB_W + 12]);
            const int el[MAXC] = {__float_as_int(e0.x), __float_as_int(e0.y), __float_as_int(e0.z), __float_as_int(e0.w),
                                  __float_as_int(e1.x), __float_as_int(e1.y), __float_as_int(e1.z), __float_as_int(e1.w)};
#pragma unroll
            for (int k = 0; k < MAXC; ++k) { const int sh = tb_shell[el[k]]; con_shell[k] = (k < ncon) ? sh : -1; }
        }
    } else if constexpr (TORSO != 0) {
        const int* tb_shell = reinterpret_cast<const int*>(lds + TB_SHELL);
        float dz, vz, az;
        torso_motion(C, tphys, dz, vz, az);
        lattice_rhs<G, NE>(lds, eb, gl, M, az, kst, kdmp, MODE == 0, s_pre, sd_pre);
        USIM_STAMP(dbg, 5);
        // (collision before the solve: its queue overlays the area the solve's result is stored to)
        int nc = collide_all<G, NE>(lds, eb, gl, gbase, M, C, MODE == 0, s_pre, dz, xs, sy, sz);
        lattice_solve<G>(lds, eb, gl, gbase);
        contact_overflow<G>(lds, eb, gl, gbase, nc);
        USIM_STAMP(dbg, 7);
        if (nc > MAXC) { overflow = 1; nc = MAXC; }
        ncon = nc;
        group_sync();
        int ncmax = 0;
#pragma unroll
        for (int k = MAXC; k >= 1; --k) if (ncmax == 0 && __any(nc >= k)) ncmax = k;
        float gf[MAXC];
        int cel[MAXC];
#pragma unroll
        for (int k = 0; k < MAXC; ++k) { gf[k] = 0.f; cel[k] = (k < nc) ? __float_as_int(EB(GE_CG + k * CG_WORDS + 6)) : 0; }
        if (ncmax > 0) {
            // every contact lane needs Lambda^-1, alpha = J qs and vs = J qd in full: broadcasts from the task lanes
            float alpha[6], vs[6], Lp[21];
            static_for<6>([&](auto Ac) {
                constexpr int a = decltype(Ac)::value;
                alpha[a] = rbc<G, TASK_LANE[a]>(alpha_t); vs[a] = rbc<G, TASK_LANE[a]>(v6);
#pragma unroll
                for (int b = 0; b <= a; ++b) Lp[PK(a, b)] = rbc<G, TASK_LANE[a]>(Li[b]);
            });
            USIM_STAMP(dbg, 8);
            if constexpr (MODE == 0) contact_solve<G, false, false>(lds, eb, gl, M, C, nc, ncmax, cel, Lp, alpha, vs, mu, vz, ContactRows{}, W, gf, dbg, cy.wr);
            else { NoWarm cold; contact_solve<G, false, false>(lds, eb, gl, M, C, nc, ncmax, cel, Lp, alpha, vs, mu, vz, ContactRows{}, W, gf, dbg, cold); }
        } else warm_clear(cy.wr);                                        // (no contact in the wave: nothing kept)
        USIM_STAMP(dbg, 11);
        // ---- element accelerations a = a~ + Linv[:, e_c] gf_c, semi-implicit Euler, write back (a reset leaves the lattice at rest) ----
        if constexpr (MODE == 1) {
            if (valid && need && !refill) {
                for (int e = gl; e < N_TOP; e += G) { LAT(LAT_S + e) = 0.f; LAT(LAT_SD + e) = 0.f; }
                if constexpr (WARM) warm_rows_clear<G>(warm_rows, gl);    // an episode starts cold
            }
        } else {
            float acc_e[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) { const int e = gl + i * G; acc_e[i] = (e < N_TOP) ? EB(GE_A + e) : 0.f; }
#pragma unroll
            for (int k = 0; k < MAXC; ++k) {
                if (k < ncmax) {
#pragma unroll
                    for (int i = 0; i < NE; ++i) {
                        const int e = (gl + i * G < N_TOP) ? gl + i * G : N_TOP - 1;
                        acc_e[i] = fmaf(lds[TB_LINV + e * LROW + cel[k]], gf[k], acc_e[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int e = gl + i * G;
                if (e >= N_TOP) continue;
                const float sdn = sd_pre[i] + dt * acc_e[i];
                const float sn = s_pre[i] + dt * sdn;
                if (valid) { LAT(LAT_SD + e) = sdn; LAT(LAT_S + e) = sn; }
                if constexpr (RES) { sd_pre[i] = sdn; s_pre[i] = sn; }
            }
            if constexpr (WARM) { if (valid) warm_store(warm_rows, gl, cy.wr); }
        }
#pragma unroll
        for (int k = 0; k < MAXC; ++k) con_shell[k] = (k < nc) ? tb_shell[cel[k]] : -1;
    }
    USIM_STAMP(dbg, 12);

    // ---------------- constrained arm acceleration, probe torque sensor, Euler step, hand velocity ----------------
    if constexpr (ROLE != 1) precompute();
    float tq[3];
    f3 hv;
    {
        // qacc = qs + M^-1 J^T W and the site acceleration J qacc = alpha + Lambda^-1 W through the operators that are already there
        float qacc = qs, aq_t = alpha_t;
        if (TORSO) {
#pragma unroll
            for (int a = 0; a < 6; ++a) { qacc = fmaf(Xm[a], W[a], qacc); aq_t = fmaf(Li[a], W[a], aq_t); }
        }
        // link accelerations from the site Jacobian: alpha = alpha_bias + Jw qacc, a(o) = a_bias + Jv qacc - (Jw qacc) x (x - o).  Every lane
        // evaluates the sensor on its own link's registers; the last link's lane holds the probe's.
        if (!defer) {
        float aq[6];
        static_for<6>([&](auto Ac) { constexpr int a = decltype(Ac)::value; aq[a] = rbc<G, TASK_LANE[a]>(aq_t); });
        const f3 alq = mk(aq[3], aq[4], aq[5]);
        const f3 alt = al + alq;
        const f3 a7 = ao + mk(aq[0], aq[1], aq[2]) - cross(alq, s_xso);
        const f3 ac = a7 + cross(alt, s_rc) + s_wwrc;
        const f3 N = rot_inertia(alt) + s_nw;
        const f3 Fp = ac * PROBE_MASS;
        const f3 tw = N + cross(s_arm, Fp) - mk(W[3], W[4], W[5]);
        tq[0] = rbc<G, NJ - 1>(dot(sx, tw)); tq[1] = rbc<G, NJ - 1>(dot(sy, tw)); tq[2] = rbc<G, NJ - 1>(dot(sz, tw));
        } else {
            // report written late: the sensor is evaluated there, from task lane a's component a of the site acceleration
            tq[0] = 0.f; tq[1] = 0.f; tq[2] = 0.f;
            if (is_task) xl[MB_REP + REP_AQ + (blk ? 3 + comp : comp)] = aq_t;
        }
        USIM_STAMP(dbg, 13);
        hv = mk(0, 0, 0);
        if constexpr (MODE == 0) {
            // mj_Euler with implicit joint damping: (M + h D) x = M qacc, one fixed-point step on M^-1
            const float xk = row_times_joint<G, NJ>(Mi, qacc);
            const float rhs = fmaf(-dt * JOINT_DAMP, xk, qacc);
            qdj = fmaf(dt, rhs, qdj); dqj = fmaf(dt, qdj, dqj);
            if (!jlane) { qdj = 0.f; dqj = 0.f; }
            qj = q0j + dqj;
            // hand velocity: Jacobian from before the integration, qvel from after (mj_step data semantics)
            const float v2_t = row_times_joint<G, NJ>(Jr, qdj);
            float v2[6];
            static_for<6>([&](auto Ac) { constexpr int a = decltype(Ac)::value; v2[a] = rbc<G, TASK_LANE[a]>(v2_t); });
            hv = mk(v2[0], v2[1], v2[2]) + cross(mk(v2[3], v2[4], v2[5]), hand - xs);
        }
    }
    USIM_STAMP(dbg, 14);

    // ---------------- observation (ultrasound.py:363-401), reward (:230-269), bookkeeping (:528-546), termination (:635-670) ----------------
    bool done = false;
    {
        if (MODE == 1) fzbar = W[2];                                     // ultrasound.py:477
        obs[0] = W[0]; obs[1] = W[1]; obs[2] = W[2];
        obs[3] = tq[0]; obs[4] = tq[1]; obs[5] = tq[2];
        obs[6] = hv.x; obs[7] = hv.y; obs[8] = hv.z;
        obs[9] = fzbar - 5.0f; obs[10] = dfz - 0.0f; obs[11] = vbar - 0.04f;
        if constexpr (MODE == 1) {
            if (overflow) status |= 1;
            if (refill) {
                // reset computed ahead of time: park it in the bank slot of episode ep_t
                if (valid && need) {
                    const int sl = ep_t & (BANK_DEPTH - 1);
                    if (jlane) BK(sl, BQ0 + gl) = qj;
                    if (gl == 0) {
                        BK(sl, BTS) = ts.x; BK(sl, BTS + 1) = ts.y; BK(sl, BTS + 2) = ts.z; BK(sl, BTE) = te.x; BK(sl, BTE + 1) = te.y; BK(sl, BTE + 2) = te.z;
                        BK(sl, BU0) = u0; BK(sl, BKST) = kst; BK(sl, BKDMP) = kdmp; BK(sl, BMU) = mu; BK(sl, BFZ) = fzbar;
#pragma unroll
                        for (int a = 0; a < OBS_DIM; ++a) BK(sl, BOBS + a) = obs[a];
                        BKI(sl, BSTATUS) = overflow ? 1 : 0;
                    }
                }
            } else if (store && io.obs && need) {
#pragma unroll
                for (int a = 0; a < OBS_DIM; ++a) io.obs[(size_t)ei * OBS_DIM + a] = obs[a];
            }
        } else if (last_sub) {
        const bool contact = ncon > 0;
        if (contact) touched = 1;
        const float force_rew = contact ? force_e : 0.f, dforce_rew = contact ? dforce_e : 0.f;
        float reward = pos_rew + ori_rew + vel_rew + force_rew + dforce_rew;
        done = t >= C.horizon;
        const float hvn = sqrt_(dot(hv, hv));
        vbar += (hvn - vbar) * rcp_((float)t);
        const float fz = W[2];
        dfz = (fz - fzprev) * rcp_(C.dt_ctrl);                             // ultrasound.py:542: self.control_timestep
        fzprev = fz;
        fzbar = 0.1f * fz + 0.9f * fzbar;
        // joint-limit margin and run-away guard are per-joint quantities: one ballot / one prefix sum over the group
        const bool jviol = (qj < at[AT_QMIN] + 0.1f) || (qj > at[AT_QMAX] - 0.1f);
        const unsigned jany = (unsigned)(__ballot(jviol) >> gbase) & GMASK;
        if (C.early_term) {
            const bool term = (jany != 0u) || (pos_err_norm > 1.0f) || (contact && ori_err > 0.10f) || (touched && !contact);
            done = done || term;
        }
        epret += reward;
        if (io.log && valid) {
            float* L = io.log + (size_t)ei * LOG_WIDTH;
            if (jlane) L[26 + gl] = qj;
            if (gl == 0) {
                const float upn = clampf((float)t * inv_h + u0, 0.f, 1.f);
                const f3 tpn = ts + (te - ts) * upn;
                L[0] = xw.x; L[1] = xw.y; L[2] = xw.z; L[3] = tpn.x; L[4] = tpn.y; L[5] = tpn.z;
                L[6] = hv.x; L[7] = hv.y; L[8] = hv.z; L[9] = 0.04f; L[10] = vbar;
                L[11] = qe[0]; L[12] = qe[1]; L[13] = qe[2]; L[14] = qe[3];
                L[15] = M.gquat[0]; L[16] = M.gquat[1]; L[17] = M.gquat[2]; L[18] = M.gquat[3];
                L[19] = ori_err * 5.0f;
                L[20] = fz; L[21] = 5.0f; L[22] = fzbar; L[23] = dfz; L[24] = 0.f; L[25] = contact ? 1.f : 0.f;
                L[40] = (float)(t - 1) * inv_h * 100.f;
                L[41] = pos_rew; L[42] = ori_rew; L[43] = vel_rew; L[44] = force_rew; L[45] = dforce_rew;
            }
        }
        if (overflow) status |= 1;
        {
            // numerical fault guard: a non-finite or run-away state ends the episode and is flagged
            const float chk = rbc<G, 7>(prefix_sum<G>(fabsf(qj) + 1e-3f * fabsf(qdj)));
            if (!(chk < 1.0e3f)) { status |= 4; done = true; epret -= reward; reward = 0.f; if (!(epret == epret)) epret = 0.f; }
        }
        if (store && !defer) {
            io.rew[ei] = reward;
            if (io.status_out) io.status_out[ei] = status;
            io.done[ei] = done ? 1 : 0;
            if (io.contacts) {
                io.contacts[(size_t)ei * (1 + MAXC)] = ncon;
#pragma unroll
                for (int k = 0; k < MAXC; ++k) io.contacts[(size_t)ei * (1 + MAXC) + 1 + k] = con_shell[k];
            }
            if (done) {
                if (io.term_obs) {
#pragma unroll
                    for (int a = 0; a < OBS_DIM; ++a) io.term_obs[(size_t)ei * OBS_DIM + a] = obs[a];
                }
                if (io.ep_ret) io.ep_ret[ei] = epret;
                if (io.ep_len) io.ep_len[ei] = t;
            }
        }
        need = done && auto_reset;
        if (store && io.obs && !need && !defer) {
#pragma unroll
            for (int a = 0; a < OBS_DIM; ++a) io.obs[(size_t)ei * OBS_DIM + a] = obs[a];
        }
        if constexpr (DEF) {
            // report written late: what depends on the contact wrench and on this pass's bookkeeping, as the stores above would have found it (before the adoption of a
            // bank episode resets the episode scalars)
            if (defer && gl == 0) {
                float4* const wk = reinterpret_cast<float4*>(&xl[MB_REP + REP_W]);
                wk[0] = make_float4(W[0], W[1], W[2], W[3]); wk[1] = make_float4(W[4], W[5], hv.x, hv.y);
                wk[2] = make_float4(hv.z, reward, epret, __int_as_float(t));
                wk[3] = make_float4(__int_as_float(status), __int_as_float((done ? 1 : 0) | (need ? 2 : 0)), __int_as_float(ncon), 0.f);
                if (io.contacts) {
                    float4* const hk = reinterpret_cast<float4*>(&xl[MB_REP + REP_SHELL]);
                    hk[0] = make_float4(__int_as_float(con_shell[0]), __int_as_float(con_shell[1]), __int_as_float(con_shell[2]), __int_as_float(con_shell[3]));
                    hk[1] = make_float4(__int_as_float(con_shell[4]), __int_as_float(con_shell[5]), __int_as_float(con_shell[6]), __int_as_float(con_shell[7]));
                }
            }
        }
        }
    }

    if constexpr (ROLE == 1) { RSTAMP(7); if (!LA || !more) USIM_BAR(); RSTAMP(8); }   // (4) the lattice side has stored the integrated lattice (LA: last pass of a launch only)
    if (MODE == 0 && need) {
        // ================= auto-reset: adopt the initial state prepared in the reset bank and queue the slot for refill =================
        episode += 1;
        const int sl = episode & (BANK_DEPTH - 1);
        qj = jlane ? BK(sl, BQ0 + jl) : 0.f; q0j = qj; qdj = 0.f; dqj = 0.f;
        ts = mk(BK(sl, BTS), BK(sl, BTS + 1), BK(sl, BTS + 2)); te = mk(BK(sl, BTE), BK(sl, BTE + 1), BK(sl, BTE + 2));
        u0 = BK(sl, BU0); kst = BK(sl, BKST); kdmp = BK(sl, BKDMP); mu = BK(sl, BMU); fzbar = BK(sl, BFZ);
        episode_begin(E, BKI(sl, BSTATUS));
        if (store && io.obs && !defer) {                                 // (report written late: the bank's row is read there)
#pragma unroll
            for (int a = 0; a < OBS_DIM; ++a) io.obs[(size_t)ei * OBS_DIM + a] = BK(sl, BOBS + a);
        }
        // (LA, another pass follows: no hand-off (4), the lattice side may still be storing -- its next integration and warm_store write every one of these words
        //  from the registers and the record it cleared when it adopted the episode)
        const bool zero_here = !LA || !more;
        if (TORSO && valid && zero_here) for (int e = gl; e < N_TOP; e += G) { LAT(LAT_S + e) = 0.f; LAT(LAT_SD + e) = 0.f; }
        if constexpr (WARM) {
            // an episode starts cold: the warm rows (after hand-off (4) in the split kernel: the lattice side has stored this step's list) and, where this wave
            // solves the contacts itself, its record (the lattice side of a resident launch learns of the new episode through the mailbox)
            if (valid && zero_here) warm_rows_clear<G>(warm_rows, gl);
            warm_clear(cy.wr);
        }
        if constexpr (RES && TORSO != 0) {
            // resident launch: the lattice of the new episode is at rest in the registers too (single wave) / in the LDS copy of the element
            // positions this side reads back at the next step (split kernel with 8-lane groups; the lattice side learns of it through the mailbox below)
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                s_pre[i] = 0.f; sd_pre[i] = 0.f;
                if (ROLE == 1 && !LA && gl + i * G < N_TOP) EB(GE_S + gl + i * G) = 0.f;       // (8-lane groups only: with LA the lattice side zeroes its own copy)
            }
        }
        if (store) order_refill(io, env, episode);
    }
    if constexpr (RES && ROLE == 1) {
        // (the wrench mailbox is free between hand-off (4) and the lattice side's next contact solve; LA: between this wave's reads behind hand-off (3) and the
        //  lattice side's read behind hand-off (1) of the next pass)
        if (gl == 0) *reinterpret_cast<float4*>(&xl[MB_W]) = make_float4(kst, kdmp, mu, (MODE == 0 && need) ? 1.f : 0.f);
    }
    USIM_STAMP(dbg, 15);
    if constexpr (DEF) { if (more) RSTAMP(28); }                         // dbg[48]: the state part of the pass before the last one done (its report is written late)

    // ---------------- store state: joint words by their lanes, the scalar quads by the group's first lane (report written late: in the next pass's wait) ----------------
    if (valid && (MODE == 0 || (need && !refill)) && !defer) {
        float* const so = st + scalar_index(0, (size_t)ei);
        if (jlane) {
            so[F_Q + gl] = dqj; so[F_QD + gl] = qdj;
            if (need) so[F_Q0 + gl] = q0j;
        }
        if (gl == 0) {
            float4* s4 = reinterpret_cast<float4*>(so);
            if (need) {
                so[F_TS] = ts.x; so[F_TS + 1] = ts.y; so[F_TS + 2] = ts.z;
                s4[6] = make_float4(te.x, te.y, te.z, u0);
            }
            s4[7] = make_float4(vbar, fzbar, fzprev, dfz);
            s4[8] = make_float4(kst, kdmp, mu, __int_as_float(t));
            s4[9] = make_float4(__int_as_float(touched), __int_as_float(episode), epret, __int_as_float(status));
        }
    }
    if (refill) group_sync();                                            // the next item reuses the per-environment LDS block
    }   // item loop
    if (MODE == 1 && refill) work_list_close(io);
    USIM_STAMP(dbg, 16);
    if constexpr (ROLE == 1) RSTAMP(9);
#undef RSTAMP
#undef LAT
#undef EB
}

// One launch = io.nsub consecutive steps (usim_rollout_random: the actions are drawn in-kernel, so step k + 1 needs nothing from the host).
// The lattice tables stay in LDS, launch latency and the kernel-argument / first-load round trip are paid once; every step still reads its
// state from HBM and writes it back together with its slice of the transition block, so the algorithmic traffic per step is unchanged.
template <int TORSO, int MODE, int ROLE, int NT, bool MULTI = false, int G = 16, class WR = NoWarm, bool ACTS = false>
DI void step16_body(float* lds, const DevModel& M, const DevCfg& C, float* __restrict__ st, const int n, const int npad, const DevIO& io0, const int flags, const long long rstep) {
    // (MULTI is a template parameter: the single-step instantiation -- usim_step, a policy in the loop -- keeps the register allocation of a
    // straight-line kernel; the loop costs it 2 us per step)
    // io0.nsub counts CONTROL steps; each is C.substeps physics passes (1 with the shipped control_freq)
    const int S = (MULTI && MODE == 0 && C.substeps > 1) ? C.substeps : 1;
    const int nsub = (MULTI && MODE == 0) ? (io0.nsub > 1 ? io0.nsub : 1) * S : 1;
    DevIO io = io0;
    int nbar = 0;                                                        // barriers executed by this wave (read by the profiling build only)
    Carry<TORSO ? (N_TOP + G - 1) / G : 1, WR> cy;                        // multi-step launches: the state stays in registers between the steps
    int sub = 0;
    long long cstep = rstep;                                             // control step: keys the in-kernel action draw
    for (int ks = 0; ks < nsub; ++ks) {
        // (the launches of usim_rollout_actions -- ACTS -- never draw: they keep the code they had)
        constexpr bool AHEAD = ROLE == 1 && MULTI && MODE == 0 && !ACTS;
        if constexpr (ROLE == 2) lattice_pass<NT, G, MULTI && MODE == 0, WR>(lds, M, C, st, n, npad, io, ks == 0, sub, ks + 1 < nsub, nbar, cy);
        else step16_one<TORSO, MODE, ROLE, NT, G, MULTI && MODE == 0, WR, AHEAD>(lds, M, C, st, n, npad, io, flags, cstep, ks == 0, sub, ks + 1 < nsub, nbar, cy);
        const bool ctrl_done = sub == S - 1;                             // this pass completed a control step
        if (ctrl_done) { sub = 0; ++cstep; } else ++sub;
        if (ks + 1 < nsub) {
            // Split kernel with 8-lane groups: the next step reads words this one left in LDS through the other wave of the pair (the element positions,
            // the new-episode word; the blocks are reused): order the stores, then meet.  (Both roles pass here once per step.)
            // A single-wave kernel keeps its state in registers and its LDS blocks to itself: its waves never meet after the table copy
            // (lanes 16 kernel 17.05 -> 16.76 us/step, rigid torso 5.12 -> 5.03).
            // Tried for the split kernel and dropped: hand-offs between the two waves of a pair only (LDS counters, s_sleep + s_wakeup) instead of
            // workgroup barriers, so that a pair with few contacts runs ahead of its neighbours over the 64 steps of a launch -- 15.4 us/step
            // against 14.8 with the barriers, whatever the sleep length (8192 envs, 8-lane groups: 23.4 against 22.7).
            // Split kernel with 16-lane groups (LA): nothing changes hands here -- the lattice side carries its state, each side owns its LDS areas and the mailbox words change hands at hand-offs
            // (1) and (3) -- so neither the fence nor the barrier: the lattice wave runs on into the next pass
            constexpr bool LA = lattice_ahead<ROLE, G, MULTI && MODE == 0>();
            if constexpr (!LA) {
                __threadfence_block();
                if constexpr (ROLE != 0) USIM_BAR();
            }
            if (io0.block && ctrl_done) advance_rollout_block(io, (size_t)n, C.adim);
            // usim_rollout_actions (ACTS): the next control step plays the next slice of the caller's action block [nsub][n][A], whether or not the outputs move --
            // a scalar add on a kernel argument, the same in both roles.  Instantiations of their own (usim_step16_acts_kernel, usim_step32_acts_kernel): in
            // the kernels of usim_rollout_random the add costs the single-wave soft-torso ones 6 - 8 more spilled VGPRs (profiles/rollout_actions/resource_usage.txt)
            if constexpr (ACTS) { if (ctrl_done) io.act += (size_t)n * C.adim; }
        }
    }
#if defined(USIM_TSTAMP) || defined(USIM_TSTAMP_NOWAIT)
    if (ROLE != 0 && io0.dbg && blockIdx.x == 0 && (threadIdx.x & (64 * SPLIT_WPR - 1)) == 0) io0.dbg[ROLE == 1 ? 46 : 47] = (unsigned long long)nbar;
#endif
}

template <int TORSO, int OCC, int MODE, bool MULTI = false, bool WARM = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void usim_step16_kernel(const DevModel M, const DevCfg C, float* __restrict__ st, int n, int npad,
                                                                                                          const DevIO io, int flags, long long rstep) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    step16_body<TORSO, MODE, 0, 256, MULTI, 16, typename std::conditional<WARM, WarmOf<16>::type, NoWarm>::type>(lds, M, C, st, n, npad, io, flags, rstep);
}

// the multi-step launch of usim_rollout_actions: step k of the launch reads slice k of io.act (step16_body ACTS); otherwise usim_step16_kernel<TORSO, OCC, 0, true, WARM>
template <int TORSO, int OCC, bool WARM = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void usim_step16_acts_kernel(const DevModel M, const DevCfg C, float* __restrict__ st, int n, int npad,
                                                                                                               const DevIO io, int flags, long long rstep) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    step16_body<TORSO, 0, 0, 256, true, 16, typename std::conditional<WARM, WarmOf<16>::type, NoWarm>::type, true>(lds, M, C, st, n, npad, io, flags, rstep);
}

// soft-torso step with two waves per quad of environments: waves 0-3 of the workgroup run the arm side, waves 4-7 the lattice / contact side
// (wave w and wave w + 4 land on the same SIMD and fill each other's stalls: at 4096 envs/GPU a single wave issues only ~55 % of its cycles)
// BARRIER INVARIANT (outside the HIP programming model; holds on gfx950 because s_barrier counts waves, not program points): the two roles
// execute __syncthreads() at DIFFERENT program points -- the arm wave's in step16_one<1, 0, 1, ...>, the lattice wave's in lattice_pass, the one between the passes, for both,
// in step16_body -- so both must execute exactly the same NUMBER of barriers on every path -- per step: the table copy (first step of a launch: at the end of either
// function's load section), hand-offs (1)-(4) (marked `// (1)` .. `// (4)` at the USIM_BAR() of either function; lattice_pass has no other barrier and no return), and
// the one between consecutive steps of a multi-step launch.  An
// early return, a barrier under a branch that is not uniform over the whole workgroup, or a fifth hand-off on one side only would hang the
// GPU instead of failing a test.  The profiling build counts the barriers of both roles (USIM_BAR: ticks[46] / ticks[47] of usim_profile_step) and
// tests/test_gpu_properties.py compares them; the split-vs-single-wave bit-exactness tests cover ragged workgroups and slot overflow.
// The lattice solve ahead (LA: 16-lane groups, multi-step launches): hand-off (4) and the barrier between the passes exist on the last pass only.  Barriers per pass, the same for
// both roles (`first_pass` and `more` are uniform over the workgroup; a launch of one pass is first and last: T (1) (2) (3) (4)):
//     pass                 arm wave                 lattice wave
//     first, more follow   T (1) (2) (3)            T (1) (2) (3)            T = table copy
//     middle               (1) (2) (3)              (1) (2) (3)
//     last                 (1) (2) (3) (4)          (1) (2) (3) (4)
//   a launch of n passes: 3 n + 2 in each role of usim_step32_kernel<true, 16, *> and usim_step32_acts_kernel<16, *>; 5 n in each role of the kernels of 8-lane groups
//   (T, then (1)-(4) and the barrier between passes n - 1 times, then (1)-(4)) and 5 in a single-step launch (the profiling build counts both roles,
//   tests/test_gpu_lattice_ahead.py compares them with this).  No fence
//   between the passes: __syncthreads() at the hand-offs orders what changes hands there, and nothing changes hands in HBM inside a launch (below).
//   What the missing barriers guarded, and what guards it now:
//   * EB(GE_S): the arm wave neither reads nor writes it (it runs no broad-phase round); the lattice wave writes it on the first pass from the state it loaded, at every
//     integration, and zeros when it adopts a new episode.  Every other word of the EB blocks was the lattice wave's already.
//   * the lattice's state between the passes: in the lattice wave's registers (s, sd, kst, kdmp, mu, t, the warm record), no longer reloaded from what the arm wave stored;
//     a new episode reaches it through MB_W behind hand-off (1), then lattice_rhs and lattice_solve run again for the wave; t advances at the top of the pass once and is
//     set to its first value again on adoption, never advanced twice.
//   * MB_W: wrench (lattice wave writes before (3), arm wave reads behind (3)), then the new-episode word (arm wave writes behind those reads, lattice wave reads behind
//     (1) of the next pass, before it writes the next wrench): every change of hands has a hand-off in between.  MB_POSE is written before (1) of pass k + 1 and was
//     read between (1) and (2) of pass k; MB_OP is written between (1) and (2) and read between (2) and (3); MB_Q belongs to the lattice wave; the transpose scratch, MB_GOAL,
//     MB_ACT and MB_REP (the report written late: parked in pass k, read in the wait of pass k + 1 by the same groups' lanes) to the arm wave: hand-off (3) of pass k lies
//     between every such pair.
//   * zeroing on reset: the arm wave zeroes the lattice and clears the warm rows in HBM behind (4), so on the last pass only; on the others the lattice wave's next
//     integration and warm_store overwrite every one of those words from the registers and the record it cleared on adoption.  What a launch leaves in HBM is unchanged.
// G = 16: 16 environments per workgroup (a quad per wave pair).  G = 8: 32 environments per workgroup (eight per wave pair; two per DPP row) -- the
// mapping for more than 4096 envs/GPU, where 16-lane groups would need a second round of workgroups.
template <bool MULTI, int G = 16, bool WARM = false>
__global__ __launch_bounds__(128 * SPLIT_WPR) __attribute__((amdgpu_waves_per_eu(2, 2))) void usim_step32_kernel(const DevModel* __restrict__ Mp, const DevCfg* __restrict__ Cp, float* __restrict__ st, int n, int npad,
                                                                                                                  const DevIO io, int flags, long long rstep) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // Model and configuration by POINTER to a constant block of the handle in HBM (usim_handle::d_consts), not by value: by value they are ~110 kernel-argument
    // dwords that the compiler loads once and keeps -- 186 of them spilled to VGPR lanes, every reload a v_readlane in the 256-step loop (round-4 review).
    // Through the pointer a field is a scalar load (SMEM, scalar cache) where it is used.
    const DevModel& M = *Mp; const DevCfg& C = *Cp;
    constexpr int NT = 128 * SPLIT_WPR;
    typedef typename std::conditional<WARM, typename WarmOf<G>::type, NoWarm>::type WR;
    if (threadIdx.x < NT / 2) step16_body<1, 0, 1, NT, MULTI, G, WR>(lds, M, C, st, n, npad, io, flags, rstep);
    else step16_body<1, 0, 2, NT, MULTI, G, WR>(lds, M, C, st, n, npad, io, flags, rstep);
}

// the multi-step launch of usim_rollout_actions with the split kernel: usim_step32_kernel<true, G, WARM> whose two roles move io.act on between control steps (step16_body
// ACTS: no barrier, no branch that differs between the roles -- the BARRIER INVARIANT above holds as it does there)
template <int G = 16, bool WARM = false>
__global__ __launch_bounds__(128 * SPLIT_WPR) __attribute__((amdgpu_waves_per_eu(2, 2))) void usim_step32_acts_kernel(const DevModel* __restrict__ Mp, const DevCfg* __restrict__ Cp, float* __restrict__ st, int n, int npad,
                                                                                                                       const DevIO io, int flags, long long rstep) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const DevModel& M = *Mp; const DevCfg& C = *Cp;
    constexpr int NT = 128 * SPLIT_WPR;
    typedef typename std::conditional<WARM, typename WarmOf<G>::type, NoWarm>::type WR;
    if (threadIdx.x < NT / 2) step16_body<1, 0, 1, NT, true, G, WR, true>(lds, M, C, st, n, npad, io, flags, rstep);
    else step16_body<1, 0, 2, NT, true, G, WR, true>(lds, M, C, st, n, npad, io, flags, rstep);
}

}  // namespace usim
