// usim_kernels.hip -- CDNA4 (gfx950) device code of the batched Ultrasound simulator's step kernels; their translation unit is usim_api.hip, which includes it
// (the policy, pack and score kernels are translation units of their own: usim_policy.hip, usim_pack.hip, usim_score.hip).
//
// This file holds
//   - the LDS layout and the group primitives (group_sync, group_bcast) of the soft torso's top face, its lattice phases (lattice_rhs, lattice_solve) and its collision
//     (collide_*, contact_overflow), which the 16-lane step kernels of usim_step16.h (rigid and soft torso, included at the end) call;
//   - usim_bank_items_kernel (refill work list of the reset / set_state paths) and usim_random_actions_kernel (the synthetic actions).
// The contact solve of the top face (contact_rows / contact_solve and its phases) is usim_contact.h, the full torso -- its physics and its step / reset kernel
// usim_step_kernel<2, 64, MODE> -- is usim_full.h, pieces of the env logic that the step kernels share are in usim_episode.h: all three included below.
// Every step kernel replaces, per environment:
//   a1 robosuite MujocoEnv.step driver            a2 OSC_POSE controller (rl_config.yaml:33-51)
//   a3 MuJoCo mj_step (forward dynamics + soft constraints + Euler)
//   a4 Ultrasound.reward  ultrasound.py:230-269   a5 sensors ultrasound.py:363-401
//   a6 _post_action / _check_terminated ultrasound.py:512-551, 635-670
//   a7 probe<->torso contact predicate ultrasound.py:673-736          a8 utils/quaternion.py
//   a10 reset ultrasound.py:416-478 (trajectory sampling, initial-pose IK, noise, solref randomisation)
// Model and algorithm are specified in DESIGN.md; this file is written independently of oracle/.
//
// Mapping.  G lanes of a wave64 form the group of one environment.
//   rigid / soft torso  G = 16 (the split kernel of the soft torso also G = 8): the kernels of usim_step16.h, which distribute the arm mathematics over
//                the group; in the lattice and contact phases below the lanes of a group split the 99-element lattice, the collision tests and the contacts:
//                  - the lattice inverse (99 x 100 fp32) and the element tables are workgroup-resident in LDS; per-environment
//                    scratch is a 548-word LDS block (548 mod 64 = 36 puts the 16-byte windows of the 16 environments on
//                    disjoint bank groups);
//                  - the lattice right-hand side is a 5-point stencil on a zero-bordered grid, the lattice solve
//                    A~ = Linv X (X = the right-hand sides of the wave's environments) runs on the matrix cores
//                    (v_mfma_f32_4x4x1) -- the one dense contraction of the path;
//                  - contacts keep ascending shell-id order through a wave ballot;
//                  - contact k lives in the registers of lane k; the dual problem is solved on 3 x 3 Delassus blocks held
//                    per lane, a Gauss-Seidel visit broadcasts three force increments with DPP row_newbcast.
//   full torso   one wave per environment: usim_step_kernel<2, 64, MODE> (usim_full.h).
// Per-environment state is read and written once per step as rows of the SoA state block in HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "usim_device.h"
#include "usim_devmath.h"

namespace usim {

// (the lattice tables' layout, LROW and TB_*: usim_device.h -- the host writes them)

// per-environment LDS block (word offsets); GE_X must stay 16-byte aligned
constexpr int GE_X = 0;                               // rhs[100] of the lattice solve
constexpr int GE_S = 100;                             // (free: element positions stay in their owners' registers)
constexpr int GE_SD = 200;                            // sdot[99]
constexpr int GE_A = 300;                             // lattice acceleration a~[99]
constexpr int GE_U = 300;                             // zero-bordered 11 x 13 grid of u = k_t s + b_t sdot; dead before a~ and the contact records land
constexpr int GE_U_WORDS = 144;                       // (LAT_NA + 2) * (LAT_NC + 2) = 143, rounded to 16 bytes
constexpr int CG_WORDS = 8;                           // contact record: n3, r3, element, distance
constexpr int GE_CG = 400;                            // contact records 8 x 8
constexpr int GE_WS = 464;                            // per-contact wrench + element impulse 8 x 8 (before that: candidate records 8..15)
constexpr int MAXCAND = 16;                           // penetrating elements recorded before the MAXC deepest are kept (+ one spare record for misses)
constexpr int GE_STRIDE = 548;                        // 548 mod 64 = 36: disjoint 16-byte bank windows for 16 environments
static_assert(GE_WS + MAXC * 8 <= GE_STRIDE && GE_CG + (MAXCAND + 1) * CG_WORDS <= GE_STRIDE && GE_U + GE_U_WORDS <= GE_STRIDE, "per-environment LDS block overflow");
static_assert((LAT_NA + 2) * (LAT_NC + 2) <= GE_U_WORDS && LAT_NA * LAT_NC == N_TOP, "padded lattice grid");

constexpr int SOFT16_LDS_WORDS = TB_WORDS + 16 * GE_STRIDE;   // the tables and the blocks of the 16 environments of a workgroup (16-lane kernels, one wave each)

DI void group_sync() {
    // the lanes of a group exchange data through LDS inside one wave: order the LDS traffic, no s_barrier needed
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// value of lane k (0..7) of every group, delivered to all lanes of the group (DPP row_newbcast, gfx90a+).  k is a
// compile-time constant after unrolling, so the switch folds to one v_mov_b32_dpp (two for G = 8).
// (__builtin_amdgcn_mov_dpp has no tied `old` operand: one v_mov_b32_dpp; update_dpp(iv, iv, ...) costs a register copy first -- three per pair and iteration of the
//  contact solve's matrix-vector product, 6 - 10 % of an iteration)
#define USIM_BCAST_CASE(K)                                                                               \
    case K:                                                                                              \
        if (G == 16) iv = __builtin_amdgcn_mov_dpp(iv, 0x150 + K, 0xf, 0xf, false);                      \
        else if (G == 8) {                                                                               \
            int t = __builtin_amdgcn_mov_dpp(iv, 0x150 + K, 0xf, 0x3, false);            /* lanes 0-7 of the row <- lane K (lanes 8-15: overwritten next) */   \
            iv = __builtin_amdgcn_update_dpp(t, iv, 0x150 + 8 + K, 0xf, 0xc, false);     /* lanes 8-15 <- lane 8 + K */          \
        }                                                                                                \
        break;
template <int G>
DI float group_bcast(float v, int k) {
    int iv = __float_as_int(v);
    switch (k) {
        USIM_BCAST_CASE(0) USIM_BCAST_CASE(1) USIM_BCAST_CASE(2) USIM_BCAST_CASE(3)
        USIM_BCAST_CASE(4) USIM_BCAST_CASE(5) USIM_BCAST_CASE(6) USIM_BCAST_CASE(7)
        default: break;
    }
    return __int_as_float(iv);
}
#undef USIM_BCAST_CASE
// 16-lane groups: lanes 0-7 of the row receive the value of lane J, lanes 8-15 that of lane 4 + J (J = 0..3, a compile-time constant after unrolling): two bank-masked
// v_mov_b32_dpp row_newbcast
DI float half_bcast(float v, int J) {
    const int iv = __float_as_int(v);
    int r = iv;
    switch (J) {
        case 0: { const int t = __builtin_amdgcn_mov_dpp(iv, 0x150 + 0, 0xf, 0x3, false); r = __builtin_amdgcn_update_dpp(t, iv, 0x150 + 4, 0xf, 0xc, false); } break;
        case 1: { const int t = __builtin_amdgcn_mov_dpp(iv, 0x150 + 1, 0xf, 0x3, false); r = __builtin_amdgcn_update_dpp(t, iv, 0x150 + 5, 0xf, 0xc, false); } break;
        case 2: { const int t = __builtin_amdgcn_mov_dpp(iv, 0x150 + 2, 0xf, 0x3, false); r = __builtin_amdgcn_update_dpp(t, iv, 0x150 + 6, 0xf, 0xc, false); } break;
        case 3: { const int t = __builtin_amdgcn_mov_dpp(iv, 0x150 + 3, 0xf, 0x3, false); r = __builtin_amdgcn_update_dpp(t, iv, 0x150 + 7, 0xf, 0xc, false); } break;
        default: break;
    }
    return __int_as_float(r);
}
// 16-lane groups, quad layout: a row whose quads 0 and 1 hold X_0..3 and whose quads 2 and 3 hold X_4..7 (quad_layout of usim_contact.h) delivers X_J to lanes 0-7 and
// X_(4 + J) to lanes 8-15 with ONE quad_perm:[J,J,J,J] (J = 0..3, a compile-time constant after unrolling) where half_bcast takes two: a row broadcast has one source lane
DI float quad_bcast(float v, int J) {
    const int iv = __float_as_int(v);
    int r = iv;
    switch (J) {
        case 0: r = __builtin_amdgcn_mov_dpp(iv, 0x00, 0xf, 0xf, true); break;
        case 1: r = __builtin_amdgcn_mov_dpp(iv, 0x55, 0xf, 0xf, true); break;
        case 2: r = __builtin_amdgcn_mov_dpp(iv, 0xAA, 0xf, 0xf, true); break;
        case 3: r = __builtin_amdgcn_mov_dpp(iv, 0xFF, 0xf, 0xf, true); break;
        default: break;
    }
    return __int_as_float(r);
}

// Phase timeline probe (diagnostics only): wave 0 of workgroup 0 stamps the shader clock when a buffer is given.  The stamps exist only in the profiling
// build (make prof -> libusim_prof.so): each one is a branch, and sixteen of them cost the production kernel 2 % (25.6 vs 25.1 us/step).  -DUSIM_TSTAMP_NOWAIT (what
// `make prof` sets) keeps the stamps from draining memory traffic; -DUSIM_TSTAMP waits for it first.
#if !defined(USIM_TSTAMP) && !defined(USIM_TSTAMP_NOWAIT)
#define USIM_STAMP(dbg, k) do { } while (0)
#elif defined(USIM_TSTAMP_NOWAIT)
#define USIM_STAMP(dbg, k) do { if ((dbg) && blockIdx.x == 0 && threadIdx.x == 0) (dbg)[k] = __builtin_readcyclecounter(); } while (0)
#else
#define USIM_STAMP(dbg, k) do { if ((dbg) && blockIdx.x == 0 && threadIdx.x == 0) { __builtin_amdgcn_s_waitcnt(0); (dbg)[k] = __builtin_readcyclecounter(); } } while (0)
#endif

// contact-solve phases of the lattice wave of the split kernel (first lattice wave of workgroup 0): dbg[40..45]
#if !defined(USIM_TSTAMP) && !defined(USIM_TSTAMP_NOWAIT)
#define USIM_CSTAMP(dbg, k) do { } while (0)
#else
#define USIM_CSTAMP(dbg, k) do { if ((dbg) && blockIdx.x == 0 && threadIdx.x == 256) (dbg)[40 + (k)] = __builtin_readcyclecounter(); } while (0)
#endif

// prescribed torso base motion (usim_config.torso_drop): none since round 4 (drop = 0: the torso stands on its rim capsules at the spawn height);
// torso_drop = 1: free fall over the 4.7 mm spawn gap of ultrasound.py:313, then rest
DI void torso_motion(const DevCfg& C, int tsim, float& dz, float& vz, float& az) {
    dz = -C.drop; vz = 0.f; az = 0.f;
    if (C.torso_drop) {
        float tt = (float)tsim * C.dt, zf = -0.5f * GRAV * tt * tt;
        if (zf > -C.drop) { dz = zf; vz = -GRAV * tt; az = -GRAV; }
    }
}

// Probe collision geometry (stand-in for the missing mesh, ultrasound_probe_gripper.xml:3,8; MuJoCo collides the convex hull of a mesh): a flared
// blade = convex hull of two parallel capsules of half-length probe_hl along the site x axis -- the tip capsule (radius probe_r, axis probe_r above
// the tip = grip_site) and an upper capsule (radius probe_r2, axis probe_h above the tip capsule's).  Signed distance of a point given in the site
// frame (site z points from the tip away from the probe body) and its gradient: the round-cone distance on the cross-section.
DI float probe_sdf(const DevCfg& C, const f3 p, f3& g) {
    // (v_rsq_f32 is a quarter-rate instruction like v_sqrt_f32 / v_rcp_f32: every length and its reciprocal come from one of them)
    // round 4: the cross-section is swept sideways by +-probe_hw as it is lengthways by +-probe_hl (a flat 2 hl x 2 hw face with edges of radius probe_r), and the
    // lowest point lies probe_tip beyond the site along its z axis
    const float py = C.probe_tip - p.z - C.probe_r, e = fmaxf(fabsf(p.x) - C.probe_hl, 0.f), el = fmaxf(fabsf(p.y) - C.probe_hw, 0.f);
    const float px2 = fmaf(el, el, e * e);
    const bool pxok = px2 > 1e-18f;
    const float ipx = pxok ? rsq_(px2) : 0.f, px = px2 * ipx;
    const float kk = fmaf(py, C.probe_ca, -(px * C.probe_cb));
    const bool low = kk < 0.f, flank = !low && !(kk > C.probe_cah);
    const float qy = py - C.probe_h;
    const float lc2 = fmaf(qy, qy, px2), ll2 = fmaf(py, py, px2);
    const bool okc = lc2 > 1e-18f, okl = ll2 > 1e-18f;
    const float ilc = okc ? rsq_(lc2) : 0.f, ill = okl ? rsq_(ll2) : 0.f;             // seen from the centre of the upper circle of the cross-section / of the tip circle
    const float cx = px * ilc, cy = qy * ilc;
    float d = low ? ll2 * ill - C.probe_r : lc2 * ilc - C.probe_r2;
    float gx = low ? px * ill : cx, gy = low ? (okl ? py * ill : -1.f) : (okc ? cy : -1.f);
    if (flank) { d = fmaf(px, C.probe_ca, fmaf(py, C.probe_cb, -C.probe_r)); gx = C.probe_ca; gy = C.probe_cb; }
    // direction field: the distance gradient is undefined on the medial axis of the body (the tip capsule's axis, probe_r below the surface, and
    // the centre plane above it); between 2/3 and 0.96 probe_r below the surface the direction turns into the one seen from the upper centre
    // (like the centre-to-centre search direction of a convex collider).  The distance stays exact.
    const float beta = okc ? clampf((-d - C.probe_deep0) * C.probe_inv_band, 0.f, 1.f) : 0.f;
    const float bx = fmaf(beta, cx - gx, gx), by = fmaf(beta, cy - gy, gy);
    const float rn = beta > 0.f ? rsq_(fmaf(bx, bx, by * by)) : 1.f;
    gx = bx * rn; gy = by * rn;
    const float gxi = gx * ipx;
    // (on the probe's axis the lateral direction is undefined: the lateral part of the direction, if any -- the blended field of the deep band -- goes to the site's y axis, so that g stays a unit vector)
    g = mk(copysignf(gxi * e, p.x), pxok ? copysignf(gxi * el, p.y) : gx, -gy);
    return d;
}

// One collision round: the probe blade against element i G + gl of this lane's environment (one element per lane); the wave ballot gives every
// hit its slot in the record area `recs` (MAXCAND records + one spare for misses), so that the list stays sorted by ascending shell id.
// Straight-line code (a miss writes its record to the spare slot): the rounds can be scheduled between the matrix instructions of the lattice
// solve.  Element = capsule (soft_box.xml:10): axis segment from the cap centre `tip` (t = 0) to the inner end (t = 1); the probe distance d(t)
// is convex along it.  With the slopes s0, s1 at the two ends, t minimises the quadratic model d0 + s0 t + (s1 - s0 + eps) t^2 / 2 on [0, 1];
// eps settles the point near the cap when the shaft lies flat against a flank of the probe (every point equally close: the plain minimiser
// would be ill-conditioned).
template <int G>
DI void collide_elem(const float* lds, float* recs, const bool valid, const int e, const int gl, const int gbase, const DevModel& M, const DevCfg& C, const float se, const float dz,
                     const f3 Kx, const f3 Ksx, const f3 Ksy, const f3 Ksz, int& nc) {
    const f3 ax = mk(lds[TB_AXIS + 3 * e], lds[TB_AXIS + 3 * e + 1], lds[TB_AXIS + 3 * e + 2]);
    const f3 tip = mk(M.torso[0] + lds[TB_POS + 3 * e], M.torso[1] + lds[TB_POS + 3 * e + 1], M.torso[2] + lds[TB_POS + 3 * e + 2] + dz) + ax * (se - ELEM_R);
    const f3 rel = tip - Kx;
    const f3 p0 = mk(dot(Ksx, rel), dot(Ksy, rel), dot(Ksz, rel));               // site frame
    const f3 us = mk(dot(Ksx, ax), dot(Ksy, ax), dot(Ksz, ax)) * (-2.f * ELEM_HL);
    f3 g0, g1, gs;
    (void)probe_sdf(C, p0, g0);
    (void)probe_sdf(C, p0 + us, g1);
    const float s0 = dot(g0, us), s1 = dot(g1, us);
    const float tt = clampf(-s0 * rcp_(fmaxf(s1 - s0, 0.f) + SHAFT_EPS), 0.f, 1.f);
    const float dist = probe_sdf(C, madd(p0, us, tt), gs) - ELEM_R;
    const bool hit = valid && (dist < 0.f);
    const f3 nn = (Ksx * gs.x + Ksy * gs.y + Ksz * gs.z) * -1.f;                 // from the element towards the probe
    const f3 rr = madd(tip, ax, -2.f * ELEM_HL * tt) + nn * (ELEM_R + 0.5f * dist) - Kx;
    const unsigned long long bal = __ballot(hit);
    const unsigned gm = (unsigned)(bal >> gbase) & ((1u << G) - 1u);
    const int slot = nc + __popc(gm & ((1u << gl) - 1u));
    const int sl = (hit && slot < MAXCAND) ? slot : MAXCAND;                      // MAXCAND = the spare record
    float4* rec = reinterpret_cast<float4*>(&recs[sl * CG_WORDS]);
    rec[0] = make_float4(nn.x, nn.y, nn.z, rr.x);
    rec[1] = make_float4(rr.y, rr.z, __int_as_float(e), dist);
    nc += __popc(gm);
}

// Broad phase (split kernel).  The probe -- convex hull of two parallel capsules whose axes are probe_h apart -- lies inside the capsule of
// radius probe_r + probe_h around its UPPER axis, a short segment (half-length probe_hl, 0.65 cm) that the test bounds by a ball around its centre.  The
// element is tested as the capsule it is: radius ELEM_R around its axis segment of half-length ELEM_HL (2.5 cm).  An element whose axis segment stays
// farther from that centre than the two radii, probe_hl and the margin allow (DevCfg::probe_cull2c states the inequality; lateral reach 4.97 cm) cannot
// touch the probe: most of the 99 elements, for 20 instructions each instead of three distance evaluations.  The survivors go, in ascending element
// order, into a queue that the lanes of the group then walk together (collide_queue): typically one pass instead of seven rounds.  The cull only filters
// what the exact narrow phase decides, so the contact lists do not depend on how tight it is.
// (History: the first form bounded the ELEMENT by a ball around its midpoint and kept the probe's upper axis as the segment -- reach 7.35 cm, DevCfg::probe_cull2.)
DI bool collide_cull(const float* lds, const int e, const DevModel& M, const DevCfg& C, const float se, const float dz, const f3 Kx, const f3 Ksz) {
    const f3 ax = mk(lds[TB_AXIS + 3 * e], lds[TB_AXIS + 3 * e + 1], lds[TB_AXIS + 3 * e + 2]);
    const f3 mid = mk(M.torso[0] + lds[TB_POS + 3 * e], M.torso[1] + lds[TB_POS + 3 * e + 1], M.torso[2] + lds[TB_POS + 3 * e + 2] + dz) + ax * (se - ELEM_R - ELEM_HL);
    const f3 d = mid - (Kx - Ksz * (C.probe_r + C.probe_h - C.probe_tip));         // from the centre of the upper axis (site z points away from the probe body)
    const f3 v = d - ax * clampf(dot(d, ax), -ELEM_HL, ELEM_HL);                   // from the centre of the upper axis to the nearest point of the element's axis segment
    return dot(v, v) < C.probe_cull2c;
}
// (The round around it -- candidate test, ballot, prefix slot, spare word 99, count -- is written out in both waves of the split kernel, step16_one and lattice_pass.  As one
//  function over a range of rounds it measured slower with 8-lane groups: config5 8192 24.67 -> 24.81 us/step, profiles/lattice_pass/ab.txt.)
template <int G>
DI void collide_queue(const float* lds, const float* queue, const int nq, float* recs, const int gl, const int gbase, const DevModel& M, const DevCfg& C,
                      const float* s_lds, const float dz, const f3 Kx, const f3 Ksx, const f3 Ksy, const f3 Ksz, int& nc) {
    for (int j0 = 0; __any(j0 < nq); j0 += G) {
        const int j = j0 + gl;
        const bool valid = j < nq;
        const int e = valid ? __float_as_int(queue[j]) : 0;
        collide_elem<G>(lds, recs, valid, e, gl, gbase, M, C, s_lds[e], dz, Kx, Ksx, Ksy, Ksz, nc);
    }
}

#define EBF(off) lds[TB_WORDS + eb * GE_STRIDE + (off)]

// More penetrating elements than contact slots (rare in a mixed batch, common right after a synchronous reset: 4 % of the environments): keep the MAXC
// deepest of the first MAXCAND candidates (ties keep the lower id), list still in ascending shell id.  The caller clamps its count to MAXC afterwards.
template <int G>
DI void contact_overflow(float* lds, const int eb, const int gl, const int gbase, const int nc) {
    if (nc > MAXC) {
        group_sync();
        if constexpr (G == 16) {
            // one candidate per lane of the group: rank by depth with sixteen row broadcasts, compact with a ballot
            const int m = nc < MAXCAND ? nc : MAXCAND;
            const bool cand = gl < m;
            const float4* rec = reinterpret_cast<const float4*>(&EBF(GE_CG + gl * CG_WORDS));
            const float4 r0 = rec[0], r1 = rec[1];
            const float d = cand ? r1.w : 1.0f;
            int rank = 0;
#define USIM_RANK_STEP(I) { const float di = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d), 0x150 + I, 0xf, 0xf, true)); \
                                rank += (di < d || (di == d && I < gl)) ? 1 : 0; }
            USIM_RANK_STEP(0) USIM_RANK_STEP(1) USIM_RANK_STEP(2) USIM_RANK_STEP(3) USIM_RANK_STEP(4) USIM_RANK_STEP(5) USIM_RANK_STEP(6) USIM_RANK_STEP(7)
            USIM_RANK_STEP(8) USIM_RANK_STEP(9) USIM_RANK_STEP(10) USIM_RANK_STEP(11) USIM_RANK_STEP(12) USIM_RANK_STEP(13) USIM_RANK_STEP(14) USIM_RANK_STEP(15)
#undef USIM_RANK_STEP
            const bool keep = cand && rank < MAXC;
            const unsigned gm = (unsigned)(__ballot(keep) >> gbase) & 0xffffu;
            const int slot = __popc(gm & ((1u << gl) - 1u));
            group_sync();                                  // every record is in registers before any slot is overwritten
            if (keep) {
                float4* dst = reinterpret_cast<float4*>(&EBF(GE_CG + slot * CG_WORDS));
                dst[0] = r0; dst[1] = r1;
            }
        } else if (gl == 0) {
            // (8 lanes per environment: one lane of the group edits the records in place)
            const int m = nc < MAXCAND ? nc : MAXCAND;
            for (int drop = m - MAXC; drop > 0; --drop) {
                int worst = 0; float wd = -1.0e30f;
                for (int j = 0; j < m; ++j) {
                    const float dj = EBF(GE_CG + j * CG_WORDS + 7);
                    if (dj < 0.f && dj >= wd) { wd = dj; worst = j; }
                }
                EBF(GE_CG + worst * CG_WORDS + 7) = 1.0f;                       // dropped
            }
            int wpos = 0;
            for (int j = 0; j < m; ++j) {
                if (EBF(GE_CG + j * CG_WORDS + 7) < 0.f) {
                    if (wpos != j)
                        for (int a = 0; a < CG_WORDS; ++a) EBF(GE_CG + wpos * CG_WORDS + a) = EBF(GE_CG + j * CG_WORDS + a);
                    ++wpos;
                }
            }
        }
    }
}

// The lattice phases of one forward pass, executed by the G lanes of a group on the group's LDS block.  Lane gl of the group owns elements gl, gl + G, ...
// (NE of them); az is the acceleration of the torso base (torso_motion), live = false puts the lattice at rest (reset computation).
//
// lattice_rhs: stage sdot and the spring-damper potential, build the right-hand side of the soft-equality system.  Needs no arm quantity.
template <int G, int NE>
DI void lattice_rhs(float* lds, const int eb, const int gl, const DevModel& M, const float az, const float kst, const float kdmp, const bool live,
                    const float* s_pre, const float* sd_pre) {
    // ---- stage sdot and the spring-damper potential u = k_t s + b_t sdot.  u goes into a zero-bordered 11 x 13 copy of the 9 x 11 grid, so that the four
    //      neighbours of an element are four unconditional reads; a pinned rim neighbour (s = 0) is a border cell.
    //      (the loads of s, sdot were issued together with the scalar state at the top of the kernel) ----
    const float kfix = 1.0f / (SI_DMAX * SR_TC * SR_TC), bfix = 2.0f / (SI_DMAX * SR_TC);
    const float kten = kst * (1.0f / SI_DMAX), bten = kdmp * (1.0f / SI_DMAX);
    {
        float4* uz = reinterpret_cast<float4*>(&EBF(GE_U));
#pragma unroll
        for (int v = gl; v < GE_U_WORDS / 4; v += G) uz[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    int up[NE];
    float u_own[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int e = gl + i * G;
        const int ix = (e * 373) >> 12, iz = e - LAT_NC * ix;            // e / 11 for e < 682
        up[i] = (ix + 1) * (LAT_NC + 2) + iz + 1;
        const float se = live ? s_pre[i] : 0.f, sde = live ? sd_pre[i] : 0.f;
        u_own[i] = fmaf(kten, se, bten * sde);
        if (e < N_TOP) { EBF(GE_SD + e) = sde; EBF(GE_U + up[i]) = u_own[i]; }     // (s itself stays in the owner's registers)
    }
    group_sync();
    // ---- lattice right-hand side: a_s + w_fix aref_fix + w_ten sum_j aref_ij
    //      = a_s - w_fix (k_fix s + b_fix sdot) - w_ten (deg u - sum of the four neighbour cells), deg = 4 (3 at the corners) ----
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int e = gl + i * G;
        if (e >= N_TOP) continue;
        const float se = live ? s_pre[i] : 0.f, sde = live ? sd_pre[i] : 0.f;
        const float* uc = &EBF(GE_U + up[i]);
        const float nb = (uc[-1] + uc[1]) + (uc[-(LAT_NC + 2)] + uc[LAT_NC + 2]);
        const bool corner = (e == 0) | (e == LAT_NC - 1) | (e == N_TOP - LAT_NC) | (e == N_TOP - 1);
        float r = -(GRAV + az) * lds[TB_AXIS + 3 * e + 2] - M.wfix * fmaf(bfix, sde, kfix * se);
        r = fmaf(-M.wten, fmaf(corner ? 3.f : 4.f, u_own[i], -nb), r);
        EBF(GE_X + e) = r;
    }
    if (gl == 0) EBF(GE_X + N_TOP) = 0.f;          // pad word read by the 16-byte row chunks
    group_sync();
}

// lattice_solve: a~ = Linv rhs into the GE_A area of every environment of the wave.  Needs no arm quantity either.
// Matrix-core form (every lane of the wave is active here): the wave's environments are the columns of one dense product
// A~[99 x EPW] = Linv[99 x 100] X[100 x EPW], issued as v_mfma_f32_4x4x1 (16 blocks of 4 rows x 4 columns per instruction).  Lane l feeds Linv row l (and
// row 64 + l) as the A operand and the rhs of environment l % 4 as the B operand; it receives rows 4 (l / 4) .. + 3 of that environment (layout:
// tools/probe/mfma_4x4x1_layout.hip).
template <int G>
DI void lattice_solve(float* lds, const int eb, const int gl, const int gbase) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    constexpr int EPW = 64 / G, NSET = (EPW >= 4 && EPW <= 8) ? EPW / 4 : 1, NCH = LROW / 4;
    const int lane = gbase + gl, ebw = eb - gbase / G, blk = lane >> 2;
    const int r1 = (64 + lane < N_TOP) ? 64 + lane : N_TOP - 1;
    const float4* la0 = reinterpret_cast<const float4*>(&lds[TB_LINV + lane * LROW]);
    const float4* la1 = reinterpret_cast<const float4*>(&lds[TB_LINV + r1 * LROW]);
    const float4* xb[NSET];
    v4f acc0[NSET], acc1[NSET];
#pragma unroll
    for (int u = 0; u < NSET; ++u) {
        xb[u] = reinterpret_cast<const float4*>(&lds[TB_WORDS + (ebw + 4 * u + (lane & 3)) * GE_STRIDE + GE_X]);
        acc0[u] = (v4f){0.f, 0.f, 0.f, 0.f}; acc1[u] = (v4f){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const float4 a0 = la0[c], a1 = la1[c];
#pragma unroll
        for (int u = 0; u < NSET; ++u) {
            const float4 b = xb[u][c];
            acc0[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.x, b.x, acc0[u], 0, 0, 0);
            acc1[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.x, b.x, acc1[u], 0, 0, 0);
            acc0[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.y, b.y, acc0[u], 0, 0, 0);
            acc1[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.y, b.y, acc1[u], 0, 0, 0);
            acc0[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.z, b.z, acc0[u], 0, 0, 0);
            acc1[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.z, b.z, acc1[u], 0, 0, 0);
            acc0[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.w, b.w, acc0[u], 0, 0, 0);
            acc1[u] = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.w, b.w, acc1[u], 0, 0, 0);
        }
    }
#pragma unroll
    for (int u = 0; u < NSET; ++u) {
        float* dst = &lds[TB_WORDS + (ebw + 4 * u + (lane & 3)) * GE_STRIDE + GE_A];
        *reinterpret_cast<float4*>(&dst[4 * blk]) = make_float4(acc0[u][0], acc0[u][1], acc0[u][2], acc0[u][3]);
        if (64 + 4 * blk < LROW)                       // rows 64..99 (word 99 is padding)
            *reinterpret_cast<float4*>(&dst[64 + 4 * blk]) = make_float4(acc1[u][0], acc1[u][1], acc1[u][2], acc1[u][3]);
    }
    group_sync();
}

// collide_all (single-wave kernels): broad phase and narrow phase in one go -- element positions into the environment's LDS block, the ids that pass
// collide_cull (ascending) into a queue, then the queue G elements at a time (collide_queue).  Same per-element arithmetic and the same ballot slots as
// walking all NE rounds.  Leaves the contact records (ascending shell id) in the GE_CG area and returns the number found (may exceed MAXC: contact_overflow).
// The queue overlays the GE_A area, which is free until lattice_solve stores its result there: collide first, then solve.
template <int G, int NE>
DI int collide_all(float* lds, const int eb, const int gl, const int gbase, const DevModel& M, const DevCfg& C, const bool live, const float* s_pre,
                   const float dz, const f3 Kx, const f3 Ksy, const f3 Ksz) {
    const f3 Ksx = cross(Ksy, Ksz);
    float* const q = &EBF(GE_A);
    int nq = 0, nc = 0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int eraw = i * G + gl, e = eraw < N_TOP ? eraw : N_TOP - 1;
        const float se = live ? s_pre[i] : 0.f;
        if (eraw < N_TOP) EBF(GE_S + eraw) = se;
        const bool cand = (eraw < N_TOP) && collide_cull(lds, e, M, C, se, dz, Kx, Ksz);
        const unsigned gm = (unsigned)(__ballot(cand) >> gbase) & ((1u << G) - 1u);
        if (cand) q[nq + __popc(gm & ((1u << gl) - 1u))] = __int_as_float(e);
        nq += __popc(gm);
    }
    group_sync();
    collide_queue<G>(lds, q, nq, &EBF(GE_CG), gl, gbase, M, C, &EBF(GE_S), dz, Kx, Ksx, Ksy, Ksz, nc);
    group_sync();                                      // the queue area is rewritten by the solve's result
    return nc;
}
#undef EBF

#include "usim_contact.h"
#include "usim_episode.h"
#include "usim_full.h"

// work items (env, episode + k), k = 1..BANK_DEPTH, for the environments selected by mask (reset / set_state paths)
__global__ void usim_bank_items_kernel(const float* __restrict__ st, int n, const uint8_t* __restrict__ mask, int2* items, int* count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * BANK_DEPTH) return;
    const int env = i / BANK_DEPTH, k = i % BANK_DEPTH + 1;
    if (mask && !mask[env]) return;
    const int episode = reinterpret_cast<const int*>(st)[scalar_index(F_EPISODE, (size_t)env)];
    items[atomicAdd(count, 1)] = make_int2(env, episode + k);
}


// synthetic actions of BASELINE.md section 4 (same stream as the in-kernel LF_RANDOM_ACT path)
__global__ void usim_random_actions_kernel(const DevCfg C, int n, long long rstep, float* __restrict__ act) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t gid = (uint32_t)(C.env_offset + i);
    u4 r1 = philox(gid, (uint32_t)rstep, (uint32_t)((unsigned long long)rstep >> 32), 1u, C.key0, C.key1);
    u4 r2 = philox(gid, (uint32_t)rstep, (uint32_t)((unsigned long long)rstep >> 32), 2u, C.key0, C.key1);
    uint32_t rr[8] = {r1.a, r1.b, r1.c, r1.d, r2.a, r2.b, r2.c, r2.d};
    for (int a = 0; a < C.adim; ++a) act[(size_t)i * C.adim + a] = synthetic_action(C, rr[a], a);
}

}  // namespace usim

#include "usim_step16.h"
