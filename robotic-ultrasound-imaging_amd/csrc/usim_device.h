// usim_device.h -- data layout shared by the HIP kernels (usim_kernels.hip) and the host side of the C ABI
// (usim_api.hip, usim_setup.h).  gfx950 only.
//
// HBM layout: one float32 block per handle (ints as bit patterns), n_pad = n rounded up to the workgroup
// width.  The per-environment state is environment-major: 40 scalar words per environment (scalar_index()), then -- soft torso --
// 200 lattice words per environment (LAT_*).  Each environment is read and written by one lane (rigid torso) or one group of lanes
// (soft torso) with 16-byte accesses off a single address.  The reset bank behind the state is environment-major as well.
#pragma once
#include <stdint.h>
#include <hip/hip_vector_types.h>      // int2 (DevIO::items); types only

namespace usim {

constexpr int NJ = 7;
constexpr int OBS_DIM = 19;
constexpr int MAXC = 8;
constexpr int N_TOP = 99;         // dynamic torso elements (top face of the 9x4x11 shell, soft_box.xml:9)
constexpr int LAT_NA = 9;         // lattice ix count (outer index of the shell order)
constexpr int LAT_NC = 11;        // lattice iz count (inner index)
constexpr int LINV_BLK = 8;       // row block of the blocked lattice inverse
constexpr int LINV_NBLK = 13;     // ceil(99 / 8)
constexpr int LOG_WIDTH = 53;      // words per environment of the optional episode record
constexpr int WG = 64;            // one wave64 per workgroup: one environment per lane

// scalar state fields (same order as usim_get_state's [n][USIM_NSCALAR] block; on the device the F_Q words hold dq = q - q0, the excursion from
// the initial pose of the episode -- usim_get_state / usim_set_state convert)
enum Field : int {
    F_Q = 0, F_QD = 7, F_Q0 = 14, F_TS = 21, F_TE = 24, F_U0 = 27, F_VBAR = 28, F_FZBAR = 29, F_FZPREV = 30,
    F_DFZ = 31, F_KST = 32, F_KDMP = 33, F_MU = 34, F_T = 35, F_TOUCH = 36, F_EPISODE = 37, F_EPRET = 38,
    F_STATUS = 39, F_NSCALAR = 40,
    F_LAT = 40,                     // first row of the lattice region (soft torso): LAT_ENV_WORDS rows of npad words, addressed
                                    // per environment: env i owns words [i * LAT_ENV_WORDS, (i + 1) * LAT_ENV_WORDS) of the region
    F_TOTAL_TOP = 40 + 200
};
// index of scalar field f of environment i inside the scalar region (the first F_NSCALAR * n_pad words of the block): environment-major,
// ten 16-byte accesses move the 40 words of an environment with one address register pair
__host__ __device__ inline size_t scalar_index(int f, size_t i) { return i * F_NSCALAR + f; }
// lattice region, environment-major (the 16 lanes of a group read 16 consecutive words): s[e] at LAT_S + e, sdot[e] at LAT_SD + e
constexpr int LAT_ENV_WORDS = 200, LAT_S = 0, LAT_SD = 100;
static_assert(F_TOTAL_TOP == F_LAT + LAT_ENV_WORDS && LAT_SD + N_TOP <= LAT_ENV_WORDS, "lattice region");

// arm table (16-lane step kernel, usim_step16.h): one record per lane of a group.  Lanes 0 .. nj-1 own the links of the chain (fixed transform
// from the parent link frame, joint about the local z axis, inertial parameters in the link frame), lane 7 owns the end-effector site frame
// (a fixed child of the last link), the other lanes carry identity transforms without mass.
constexpr int A16_LANES = 16;
enum ArmTable : int { AT_RFIX = 0 /* 9: columns x, y, z of the fixed rotation */, AT_LPOS = 9 /* 3 */, AT_LCOM = 12 /* 3 */, AT_MASS = 15,
                      AT_INERTIA = 16 /* 6: xx xy xz yy yz zz about the COM, link frame */, AT_QMIN = 22, AT_QMAX = 23, AT_TAUMAX = 24,
                      AT_INITQ = 25, AT_JOINT = 26 /* 1: the lane owns a joint, 0: padding / site / idle lane */, AT_ARMATURE = 27 /* rotor inertia on the joint's diagonal entry of the mass matrix */, AT_STRIDE = 28 };

// lattice tables, laid out exactly as their workgroup-resident LDS copy.  One device buffer per handle (DevModel::tables, built and
// uploaded by usim_create): handles with different torso shapes can live side by side on one GPU
constexpr int LROW = 100;                             // row stride of the lattice inverse (pad word zero)
constexpr int TB_LINV = 0;                            // float [99][100]
constexpr int TB_POS = N_TOP * LROW;                  // float [99][3] nominal surface point rel. torso centre (padded to 300)
constexpr int TB_AXIS = TB_POS + 300;                 // float [99][3] slide axis
constexpr int TB_SHELL = TB_AXIS + 300;               // int   [99]    shell id (contact-pair index convention)
constexpr int TB_WORDS = TB_SHELL + 100;              // 10600 words (the lattice topology itself is implicit: 9 x 11 grid stencil)
constexpr int TB_ARM = TB_WORDS;                      // behind the lattice block (not copied to LDS): the arm table of the 16-lane step kernel
constexpr int TB_TOTAL = TB_ARM + A16_LANES * AT_STRIDE;

// full torso (usim_full.h)
constexpr int NSH = 270;                      // shell elements (soft_box.xml:9 count="9 4 11")
constexpr int FE = 5;                         // elements per lane: element e = FE * lane + i  (64 * 5 = 320 >= 270; elements >= 270 do not exist: mass-less, zero everywhere)
constexpr int FNE = 64 * FE;
// table block of a full-torso handle (DevModel::tables), words
constexpr int FT_POS = 0;                     // float [270][3] element surface point, body frame
constexpr int FT_AXIS = 816;                  // float [270][3] slide axis (radial)
constexpr int FT_NBR = 1632;                  // int   [320][4] shell neighbours (FNE - 1 = a word that is always zero: no neighbour)
constexpr int FT_P = 2912;                    // float [270][3] P = L^-1 N'
constexpr int FT_DIAG = 3728;                 // float [320]    diagonal of L (1 for elements that do not exist)
constexpr int FT_CONST = 4048;                // float [32]     S^-1 (9), I_b^-1 (9), M_tot, contact regulariser scale of an element-table contact
constexpr int FT_LINV = 4080;                 // float [270][272] L^-1
constexpr int FT_LROW = 272;
constexpr int FT_WORDS = FT_LINV + NSH * FT_LROW;
// state of the lattice region of a full-torso handle (environment-major, LATF_ENV_WORDS words per environment)
constexpr int LATF_S = 0, LATF_SD = 272, LATF_BODY = 544;     // s[270], sdot[270], body: position (3, base-centred world axes), quaternion w x y z, linear velocity (world), angular velocity (body frame)
// warm start of the contact solve (the forces of the previous physics step: element-table contacts by element, probe contacts by element and geom):
constexpr int LATF_WTAB = 560;                // float [270][4] force (normal, t1, t2) and friction multiplier of the element's table contact; zeros: none
constexpr int LATF_WPROBE = LATF_WTAB + 4 * NSH;   // int [8] elements of the probe contact slots (-1: empty), then float [16][4]: contacts A of slots 0-7, contacts B
constexpr int LATF_WARM_WORDS = 4 * NSH + 8 + 64;
constexpr int LATF_ENV_WORDS = LATF_WPROBE + 8 + 64;      // 1712
static_assert(LATF_ENV_WORDS % 4 == 0 && LATF_WTAB % 4 == 0 && (LATF_WPROBE + 8) % 4 == 0, "16-byte accesses");
constexpr int F_TOTAL_FULL = F_NSCALAR + LATF_ENV_WORDS;

// model constants (host-built in fp64, narrowed once; passed to the kernels by value -> kernarg/SGPRs)
struct DevModel {
    float m7, c7[3], I7[6];         // link-7 composite (link7 + hand + probe): mass, COM, inertia about COM (xx,xy,xz,yy,yz,zz), link-7 frame
    float site7[3], hand7[3];       // eef site / right_hand origin in the link-7 frame
    float pcom7[3], pI7[6];         // probe body alone (torque sensor), link-7 frame
    float torso[3];                 // torso centre at spawn, base-centred world axes
    float grot[9];                  // rotation matrix of goal_quat (row-major)
    float gquat[4];                 // goal_quat (x,y,z,w) exactly as written at ultrasound.py:174
    float ghat[4], geps;            // unit goal quaternion (w,x,y,z) and 1 - |goal_quat|
    float base[3];                  // robot base in world coordinates
    float ikb[3];                   // systematic offset of the reference's initial-pose IK
    float invw, wfix, wten;         // contact regulariser scale, lattice soft-equality weights
    float armature[NJ];             // rotor inertia per joint (usim_config.armature_scale * 5 / (i + 1)): the full-torso kernel; the 16-lane kernels read the arm table
    const float* tables;            // this handle's lattice table block in HBM (TB_WORDS words, 16-byte aligned; soft torso only)
};

struct DevCfg {
    int mode, horizon, early_term, det_traj, rand_solref, rand_pos, rand_fric, torso_drop;
    int pgs_iters, ik_iters, env_offset, adim;
    uint32_t key0, key1;
    float dt, kp_fixed, damping_ratio, kp_min, kp_max, out_pos, out_ori;
    float stiffness, damping, elem_fric, probe_fric, probe_r, probe_hl;
    float probe_hw, probe_tip;                                   // half-width of the flat face across the blade, lowest point beyond the site (probe_sdf)
    float probe_cull2;                                           // read by no kernel; kept for the block's layout (the ball-form broad phase's (probe_r + probe_h + probe_hw + ELEM_HL + ELEM_R + margin)^2)
    float probe_deep0, probe_inv_band;                           // direction field below the surface: blend band (probe_sdf)
    float probe_r2, probe_h, probe_ca, probe_cb, probe_cah;   // flared blade (usim_kernels.hip probe_sdf): upper radius, height, flank direction (ca, cb), ca * h
    float top_off, y_range, drop;       // trajectory height above the torso centre, half width of the waypoint grid, spawn gap
    float probe_fric2, rn_scale;        // second colliding probe geom (usim_config.probe_geoms = 2): its friction; scale of the normal row's regulariser (0.5: two equal rows in parallel -- the merged contact of pair_model 0)
    int probe_geoms;
    int pair;                           // 1: the two coincident contacts of a probe-element pair are two contacts of the convex problem (usim_config.pair_model); the friction word of an
                                        // environment is then contact A's, contact B's is max(probe_fric2, elem_fric)
    int substeps;                       // physics steps (of dt) per control step: int(control_timestep / model_timestep) of robosuite MujocoEnv.step
    float dt_ctrl;                      // control timestep = substeps * dt (ultrasound.py:542)
    float frictionloss;                 // dry friction of every arm joint, N m (usim_config.joint_frictionloss)
    float probe_cull2c;                 // broad phase, the element as a capsule (collide_cull): (rp + ELEM_R + margin)^2 with
                                        //     rp = max(hypot(H, probe_h) + probe_r, H + probe_r2),  H = hypot(probe_hl, probe_hw).
                                        // c = centre of the probe's upper axis (probe_tip - probe_r - probe_h along site z), S = the element's axis segment.  A point p of the blade
                                        // (probe_sdf) is b + rho u + z with b in the rectangle |x| <= hl, |y| <= hw of the site's xy plane (|b| <= H), u a unit vector of that plane,
                                        // and (rho, py) a point of the cross-section K = hull of the discs (0, 0; r) and (0, h; r2); c is the point (0, h) of the axis.  So
                                        // |p - c|^2 = |b + rho u|^2 + (py - h)^2 <= (H + rho)^2 + (py - h)^2, the squared distance of (rho, py) from A = (-H, h).  The farthest point
                                        // of a hull of two discs from A lies on one of them, at |centre - A| + radius: hypot(H, h) + r or H + r2.  Hence |p - c| <= rp, whatever
                                        // probe_tip (it only moves c along site z) and for every probe_hw >= 0.  A point of the element lies within ELEM_R of S, so a common point
                                        // needs dist(c, S) <= rp + ELEM_R: an element with dist(c, S)^2 >= probe_cull2c cannot touch.  margin 1e-4 m: fp32 rounding of the
                                        // positions (~1e-7 m) and a clamped projection that misses the minimiser by |1 - |axis|| ELEM_HL (it can only lengthen the distance found)
};

struct DevIO {
    const float* act;               // [n][A] or nullptr (in-kernel synthetic actions)
    float* obs; float* rew; uint8_t* done;
    float* term_obs; int* contacts; float* ep_ret; int* ep_len;
    float* act_out;                 // [n][A] drawn actions (LF_RANDOM_ACT) or nullptr
    int* status_out;                // [n] status word of the step (bit 0 contact-slot overflow, bit 2 numerical fault) or nullptr
    float* log;                     // [n][LOG_WIDTH] per-step episode record (CSV dump of the reference) or nullptr
    const uint8_t* mask;            // reset mask (reset-only launches)
    const float* reset_params;      // [n][13] explicit reset draws or nullptr
    int2* items;                    // refill work list of (env, episode): appended by step kernels, consumed by refill launches
    int* count;                     // [0] number of items, [1] finished workgroups of the running refill launch
    int bank_row0;                  // first row of the reset bank inside the state block
    unsigned long long* dbg;        // phase timeline probe (diagnostics; nullptr in production launches)
    int refill;                     // reset launches: 0 = reset the live state of the masked envs, 1 = compute the listed bank episodes
    int nsub;                       // step launches of the 16-lane kernels: consecutive steps per launch (0 / 1 = one); step k draws the actions of
                                    // rstep + k and, with block != 0, writes slice k of rollout blocks [nsub][n][...]
    int block;
};

// rollout blocks [steps][n][...] (DevIO::block): move the block pointers on by `rows` = steps * n rows; adim: words per action
__host__ __device__ inline void advance_rollout_block(DevIO& io, size_t rows, int adim) {
    io.obs += rows * OBS_DIM; io.rew += rows; io.done += rows;
    if (io.term_obs) io.term_obs += rows * OBS_DIM;
    if (io.contacts) io.contacts += rows * (1 + MAXC);
    if (io.ep_ret) io.ep_ret += rows;
    if (io.ep_len) io.ep_len += rows;
    if (io.act_out) io.act_out += rows * adim;
}

enum LaunchFlags : int { LF_AUTO_RESET = 1, LF_RANDOM_ACT = 4 };

// reset bank: BANK_DEPTH ring slots per environment (slot = episode mod depth), each holding a ready-made initial state and
// the reset observation of one future episode (a pure function of seed, global env id and episode index)
enum BankField : int { BQ0 = 0, BTS = 7, BTE = 10, BU0 = 13, BKST = 14, BKDMP = 15, BMU = 16, BFZ = 17, BOBS = 18, BSTATUS = 37, BANK_WORDS = 38 };
constexpr int BANK_DEPTH = 256;                       // = the refill period in steps (an environment consumes at most one slot per step).  64 -> 256: the refill launch is a
                                                      // latency-bound pass (~40 us whatever the number of finished episodes), so a quarter as many of them: 14.27 ->
                                                      // 13.70 us per step at 4096 envs (128: 14.00), 20.7 -> 19.6 at 8192; 168 MB of bank at 4096 envs
constexpr int MAX_STEPS_PER_LAUNCH = 256;
constexpr int BANK_STRIDE = 40;                       // words per slot (BANK_WORDS rounded up to 16 bytes)
constexpr int BANK_ROWS = BANK_DEPTH * BANK_STRIDE;   // the bank is environment-major too: env i owns BANK_ROWS words, slot s at s * BANK_STRIDE

// warm rows (usim_config.warm_start, soft top-face torso; allocated only then): WARM_WORDS words per environment behind the reset bank, environment-major -- the
// kept contact list of the previous physics step in one layout for every mapping: the element of each of the MAXC contact slots (-1: empty), then force (3) and
// friction multiplier of the 2 MAXC virtual contacts, contact A of slot c at c, contact B at MAXC + c (= usim_get_warm_start's block, the elements as ints)
constexpr int WARM_EL = 0, WARM_F = MAXC, WARM_WORDS = MAXC + 2 * MAXC * 4;
__host__ __device__ inline size_t warm_index(int bank_row0, int npad, size_t i) { return (size_t)(bank_row0 + BANK_ROWS) * npad + i * WARM_WORDS; }

}  // namespace usim
