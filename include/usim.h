/*
 * usim.h -- C ABI of libusim, the MI355X-native batched Ultrasound simulator.
 *
 * This is the drop-in boundary of SURVEY.md section 8(b): one handle simulates n independent copies of the
 * reference's `Ultrasound` robosuite environment (src/my_environments/ultrasound.py:29) and one call
 * advances all of them by one env.step().  The reference has no FFI of its own (it is pure Python on top of
 * mujoco-py); each entry point below names the reference interface it replaces.  The Python host class
 * robotic-ultrasound-imaging_amd/vec_env.py binds exactly these symbols with ctypes and exposes the
 * stable-baselines3 VecEnv surface used by src/rl.py:130-143.
 *
 * Conventions
 *   - plain C, no exceptions across the boundary: every function returns 0 (USIM_OK) or a negative
 *     usim_status; usim_strerror() maps it to text.  Per-environment numerical faults never fail a call;
 *     they are reported in the status word of the environment (usim_get_state, field `status`).
 *   - all `*_dev` pointers are device (HBM) pointers owned by the caller (PyTorch-ROCm tensors);
 *     all other pointers are host pointers.  The library owns all simulator state and allocates nothing
 *     inside usim_step().
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); work is only
 *     enqueued, the call does not synchronise.  A handle is not thread-safe.
 *   - observations are float32 [n][19] row-major, actions float32 [n][A] row-major (A = 6, or 7 for
 *     variable_z), rewards float32 [n], dones uint8 [n].
 */
#ifndef USIM_H
#define USIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USIM_OBS_DIM 19   /* ultrasound.py:394-401: 3+3+3+1+1+1+7 */
#define USIM_MAXC 8       /* contact slots per environment */
#define USIM_NSCALAR 40   /* scalar state words per environment in usim_get_state/usim_set_state */
#define USIM_RESET_PARAMS 13
#define USIM_LOG_WIDTH 53

typedef enum usim_status {
    USIM_OK = 0,
    USIM_ERR_INVALID = -1,      /* bad argument / configuration */
    USIM_ERR_NO_DEVICE = -2,    /* no HIP device, or device index out of range */
    USIM_ERR_HIP = -3,          /* a HIP runtime call failed (see usim_last_hip_error) */
    USIM_ERR_ALLOC = -4,
    USIM_ERR_UNSUPPORTED = -5
} usim_status;

/* impedance_mode of the OSC_POSE controller: rl_config.yaml:41 ("tracking"), main.py:33 ("fixed"),
 * utils/plot.py:208-211,303-313 ("variable_z"), utils/plot.py:267-268 ("wrench": the action, +-10, replaces desired_force/desired_torque of the OSC law) */
enum { USIM_MODE_TRACKING = 0, USIM_MODE_FIXED = 1, USIM_MODE_VARIABLE_Z = 2, USIM_MODE_WRENCH = 3 };
/* torso model: BASELINE.json configs[1] (rigid, contact solver off) / configs[2] (soft torso) */
/* USIM_TORSO_FULL: all 270 shell elements on the free torso body of ultrasound.py:426-431, element-table contacts (soft_box.xml:9, ultrasound.py:300-314) -- one wave
 * per environment, an order of magnitude slower than the top-face model that the metric is quoted on; Panda, substeps 1, one step per launch */
enum { USIM_TORSO_NONE = 0, USIM_TORSO_TOP = 1, USIM_TORSO_FULL = 2 };
/* robots (ultrasound.py:137) */
enum { USIM_ROBOT_PANDA = 0, USIM_ROBOT_UR5E = 1 };

/* Mirrors the `robosuite:` block of src/rl_config.yaml:18-57 (the kwargs of Ultrasound.__init__,
 * ultrasound.py:99-136) plus the knobs the MJCF assets fix in the reference. */
typedef struct usim_config {
    int32_t struct_size;                       /* sizeof(usim_config) of the header the CALLER was built against.  The caller sets it before
                                                * usim_default_config(); that call and usim_create() return USIM_ERR_INVALID -- without writing
                                                * anything -- when it differs from the library's, so a binding built against another layout of
                                                * this struct fails loudly instead of passing shifted fields or being overrun */
    int32_t mode;                              /* controller_configs.impedance_mode */
    int32_t torso;                             /* USIM_TORSO_* */
    int32_t horizon;                           /* rl_config.yaml:27 */
    int32_t early_termination;                 /* rl_config.yaml:52 */
    int32_t deterministic_trajectory;          /* rl_config.yaml:54 */
    int32_t torso_solref_randomization;        /* rl_config.yaml:55 */
    int32_t initial_probe_pos_randomization;   /* rl_config.yaml:56 */
    int32_t friction_randomization;            /* BASELINE.json configs[4] */
    int32_t torso_drop;                        /* 0 (default since round 4): the torso base stays at its spawn height -- ultrasound.py:313 spawns the nominal bottom plane 4.7 mm
                                                * above the table, but the caps of the tilted rim capsules of the bottom face reach 4.9 - 5.8 mm below that plane and carry
                                                * the torso from the first step; 1: free fall over the 4.7 mm, then rest (rounds 1-3); 2: at rest 4.7 mm
                                                * lower from the start */
    int32_t pgs_iters;                         /* iterations of the contact solver per forward pass (default 24): block Jacobi with a line search on the dual of MuJoCo's
                                                * convex contact problem -- every contact solves its own 3 x 3 cone block at the same time (ray update, then the friction QCQP with
                                                * the normal fixed), the step along the joint direction is the minimiser of the quadratic with the slope taken block by block, capped at 1.  24 iterations rest
                                                * 2e-3 N (99th percentile) from the optimum, which is what MuJoCo's Newton solver converges to.
                                                * With warm_start = 1 the iterations start from the previous physics step's forces instead of zero, so a given count ends
                                                * closer to the optimum (18 warm iterations follow a converged solve's decisions as 24 cold ones do).
                                                * USIM_TORSO_FULL: sweeps of a block Gauss-Seidel over the probe and the element-table contacts, started from the forces of the
                                                * previous physics step (94 % of the environments follow a converged solve's decisions at 24) */
    int32_t ik_iters;                          /* reset inverse-kinematics iterations */
    int32_t env_offset;                        /* global index of env 0 of this handle (multi-GPU shard) */
    int32_t lanes_per_env;                     /* kernel mapping: 0 automatic; 16 lanes per environment (arm mathematics distributed over the group); 32 (soft torso: the split
                                                * kernel, arm side and lattice / contact side in two waves that share a SIMD; automatic up to 4096 envs); 64 (soft torso: the
                                                * same with 8-lane groups, 32 environments per workgroup; automatic beyond 4096 envs).  Rigid torso: 0 or 16; soft torso: 0, 16,
                                                * 32 or 64; full torso: 0, 16, 32 or 64, ignored (one wave per environment); anything else is USIM_ERR_INVALID.  The table of
                                                * mappings: resolve_mapping in csrc/usim_setup.h; of the kernels they run: the launch table of csrc/usim_api.hip */
    int32_t torso_shape;                       /* use_box_torso (rl_config.yaml:57): 0 box (soft_box.xml), 1 cylinder (soft_human_torso.xml) */
    int32_t waves_per_simd;                    /* soft torso, 16-lane step kernel: register budget for 1 or 2 waves per SIMD; 0 auto (1 up to 4096 envs, 2 beyond).  Nonzero with
                                                * lanes_per_env 0: lanes_per_env 16.  Rigid and full torso: 0, 1 or 2, ignored */
    int32_t robot;                             /* USIM_ROBOT_*: robots of ultrasound.py:137 */
    uint64_t seed;                             /* rl_config.yaml:1 */
    double control_dt;                         /* 1 / control_freq (rl_config.yaml:26) */
    double kp_fixed, damping_ratio;            /* rl_config.yaml:38-39 */
    double kp_min, kp_max;                     /* rl_config.yaml:42 */
    double out_max_pos, out_max_ori;           /* rl_config.yaml:36 */
    double stiffness, damping;                 /* soft_box.xml:9 solrefsmooth */
    double elem_friction, probe_friction;      /* soft_box.xml:10, ultrasound_probe_gripper.xml:8 */
    double probe_radius, probe_halflen;        /* stand-in for the missing probe mesh (ultrasound_probe_gripper.xml:3,8), a flared blade = convex hull of two
                                                * parallel capsules along the site x axis: tip capsule radius / half-length (its axis one radius above grip_site) ... */
    double probe_radius2, probe_height;        /* ... upper capsule: radius, height of its axis above the tip capsule's (probe_height > |probe_radius2 - probe_radius|) */
    int32_t substeps;                          /* physics steps per env.step(): int(control_timestep / model_timestep) of robosuite MujocoEnv.step, model timestep 2 ms
                                                * (1 with the shipped control_freq 500, rl_config.yaml:26; 25 with the env default 20, ultrasound.py:119).  control_dt above is
                                                * the CONTROL timestep (ultrasound.py:542); the physics step is control_dt / substeps.  substeps > 1: not with
                                                * USIM_TORSO_FULL (USIM_ERR_UNSUPPORTED) */
    int32_t probe_geoms;                       /* colliding geoms of the probe body.  2 (default): ultrasound_probe_gripper.xml:8-9 declares `probe_collision` AND `probe_visual`
                                                * on the same mesh, and the visual one carries no contype = conaffinity = 0 -- with MuJoCo's defaults it collides too, with the
                                                * default friction (1, 0.005, 0.0001): every probe-element pair has two coincident contacts.  With pair_model = 0 restated as one contact whose normal
                                                * row has half the regulariser (two equal rows in parallel), whose friction rows are those of the high-friction contact (the other
                                                * cone, mu = 0.01, saturates at once) and whose cone limit is (mu_1 + mu_2) / 2 of the total normal force.  1: a single probe geom */
    double probe_friction2;                    /* sliding friction of the second geom (MuJoCo default 1.0) */
    double probe_halfwidth;                    /* round 4: half-width of the flat part of the probe's face ACROSS the blade -- the face is a flat 2 probe_halflen x 2 probe_halfwidth
                                                * rectangle whose edges have the radius probe_radius (0: the blade of round 3, a tip capsule) */
    double probe_tip;                          /* round 4: the lowest point of the probe lies this far beyond grip_site along the site's z axis (0: the tip is the site) */
    int32_t pair_model;                        /* probe_geoms = 2 only.  1 (default since round 5): the two coincident contacts of a probe-element pair are TWO contacts of the
                                                * convex problem, as in MuJoCo -- the same three rows twice, each with a single contact's regulariser, cones
                                                * mu_A = max(probe_friction, elem_friction) (the per-environment friction word) and mu_B = max(probe_friction2, elem_friction).
                                                * 0: the merged contact of rounds 3-4 (half the normal regulariser, cone (mu_A + mu_B) / 2) */
    int32_t warm_start;                        /* USIM_TORSO_TOP: 1 = every contact solve starts from the forces of the previous physics step, as MuJoCo's solver does
                                                * (mj_step warm-starts from qacc_warmstart): an environment keeps the element of each contact slot with the force and friction
                                                * multiplier of its two virtual contacts; the next solve matches its contacts against that list by element, a matched contact
                                                * starts from the kept values (the shared residual from b + A s0), an unmatched one from zero.  Carried from substep to substep;
                                                * an episode starts cold (auto-reset, usim_reset, usim_reset_explicit, fault-guard restart), and so does a state set with
                                                * usim_set_state.  0 (default): cold start, the behaviour of earlier versions bit for bit.  Rigid and full torso: 0 or 1, no
                                                * effect (the full torso is always warm).  Anything else: USIM_ERR_INVALID.  The USIM_WARM_START environment variable (0 / 1),
                                                * read by usim_create, replaces the field's value for every handle the process creates afterwards -- a switch for timing a fixed
                                                * command line, in either direction; usim_has_warm_start says what a handle runs.  (Was reserved0: same offset, same sizeof) */
    double armature_scale;                     /* rotor inertia armature_i = armature_scale * 5 / (i + 1) kg m^2 on arm joint i (MuJoCo joint armature: added to the diagonal of the
                                                * mass matrix -- the plant's and, through sim.data.qM, the OSC controller's).  [RECALLED: robosuite >= 1.2 RobotModel.__init__ sets armature
                                                * 5 / (i + 1), frictionloss 0.1 and damping 0.1 on robot joints that do not specify them; the reference imports robosuite.utils.observables
                                                * (ultrasound.py:18), a 1.2 API; robosuite is not vendored in the snapshot.]  Default 1 since 0.5; 0 = none (earlier versions).  All three shipped
                                                * checkpoints replay closer to their MuJoCo statistics with it */
    double joint_frictionloss;                 /* dry friction of every arm joint, N m (MuJoCo joint frictionloss, 0.1 by the same robosuite default): one bounded constraint row per joint in
                                                * MuJoCo, restated joint by joint.  Default 0.1; 0 = none (earlier versions) */
} usim_config;

typedef struct usim_handle usim_handle;

/* Per-step I/O block.  Required: obs, rew, done.  `act` may be NULL only for usim_rollout_random /
 * usim_time_steps (actions are then drawn in-kernel).  Optional outputs may be NULL. */
typedef struct usim_step_io {
    const float* act_dev;      /* [n][A]   replaces the `action` argument of env.step (robosuite MujocoEnv.step) */
    float* obs_dev;            /* [n][19]  GymWrapper-flattened observation; the RESET observation where done */
    float* rew_dev;            /* [n]      Ultrasound.reward, ultrasound.py:230-269 */
    uint8_t* done_dev;         /* [n]      ultrasound.py:549-550 + horizon */
    float* term_obs_dev;       /* [n][19]  SB3 infos[i]["terminal_observation"]; written where done */
    int32_t* contacts_dev;     /* [n][1+USIM_MAXC] count, then ascending shell-element ids (ultrasound.py:673-736) */
    float* ep_return_dev;      /* [n]      SB3 Monitor infos[i]["episode"]["r"]; written where done */
    int32_t* ep_length_dev;    /* [n]      SB3 Monitor infos[i]["episode"]["l"]; written where done */
    float* act_out_dev;        /* [n][A]   usim_rollout_random only: the actions drawn in-kernel (completes the transition) */
    int32_t* status_dev;       /* [n]      per-environment status word after this step (bits stay set until the episode ends): bit 0 = more than USIM_MAXC simultaneous probe contacts, bit 1 =
                                *          (USIM_TORSO_FULL only) more element-table contacts than the kernel keeps (120), bit 2 = numerical fault (non-finite / run-away state of the
                                *          arm or -- USIM_TORSO_FULL -- of the free torso body or a slider; the episode is ended and, with auto_reset, restarted) */
    float* log_dev;            /* [n][USIM_LOG_WIDTH] per-step episode record, the channels of the reference's save_data CSV dump
                                *          (ultrasound.py:552-614): ee_pos3 goal_pos3 ee_vel3 goal_vel vbar ee_quat4 goal_quat4 quat_dist Fz goal_Fz
                                *          Fz_mean dFz goal_dFz is_contact q7 torques7 time% pos/ori/vel/force/dforce reward action7 */
} usim_step_io;

/* fills *c with the shipped configuration (src/rl_config.yaml).  c->struct_size must hold sizeof(usim_config) on entry:
 *     usim_config c = { sizeof c };  usim_default_config(&c); */
int usim_default_config(usim_config* c);

/* Replaces suite.make("Ultrasound", **options) + GymWrapper (src/rl.py:36-40) for n environments on HIP
 * device `device`.  Environments start un-reset; call usim_reset first.  Every handle owns its model tables (lattice inverse,
 * element geometry) in device memory: any number of handles, with the same or different configurations (torso_shape, torso, mode),
 * may be alive on one GPU at the same time.  The upload is complete when usim_create returns. */
int usim_create(const usim_config* cfg, int n_envs, int device, usim_handle** out);
void usim_destroy(usim_handle* h);

/* Switch the kernel mapping of a live soft-torso handle between lanes_per_env 32 or 64 (split kernel) and 16 (waves_per_simd 0 / 1 / 2 as in
 * usim_config); lanes_per_env 0 and rigid or full-torso handles are USIM_ERR_INVALID.  The mappings compute the same bits, so a rollout may change between them at any step -- e.g. the two-waves-per-SIMD
 * 16-lane build while a collective's workgroups are resident, the split kernel otherwise (bench.py, N > 1).  Takes effect with the next
 * call that enqueues work. */
int usim_set_mapping(usim_handle* h, int lanes_per_env, int waves_per_simd);

int usim_num_envs(const usim_handle* h);
int usim_action_dim(const usim_handle* h);     /* GymWrapper.action_space.shape[0] */
int usim_num_elements(const usim_handle* h);   /* dynamic torso elements per env (0, 99 or 270) */
int usim_has_warm_start(const usim_handle* h); /* 1: the handle keeps a contact list for usim_get_warm_start / usim_set_warm_start (USIM_TORSO_TOP with warm_start = 1, after
                                                * USIM_WARM_START); 0: it does not; < 0: error code */

/* Replaces env.reset() (ultrasound.py:416-478) for the envs where mask_dev[i] != 0 (NULL = all).
 * obs_dev [n][19] (may be NULL) receives the reset observation of the selected envs. */
int usim_reset(usim_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* Same, with explicit per-env draws instead of the seeded stream: params_dev [n][13] =
 * start xyz, end xyz (world), u0, position noise xyz, stiffness, damping, contact friction. */
int usim_reset_explicit(usim_handle* h, const uint8_t* mask_dev, const float* params_dev, float* obs_dev, void* stream);

/* Replaces SubprocVecEnv.step_async + step_wait over n envs (src/rl.py:130): one env.step() each, with
 * SB3 auto-reset semantics when auto_reset != 0. */
int usim_step(usim_handle* h, const usim_step_io* io, int auto_reset, void* stream);

/* Synthetic workload of BASELINE.md section 4: fills act_dev [n][A] with i.i.d. uniform actions from the
 * counter-based stream keyed (seed, global env id, step). */
int usim_random_actions(usim_handle* h, int64_t step, float* act_dev, void* stream);

/* Enqueues nsteps consecutive steps whose actions are drawn in-kernel from the same stream as
 * usim_random_actions(first_step + k) (io->act_dev ignored).  block_advance == 0: every step writes the same
 * buffers.  block_advance != 0: the non-NULL buffers of io are rollout blocks [nsteps][n][...] and step k writes
 * slice k (SB3 RolloutBuffer layout, the unit that is all-gathered across GPUs). */
int usim_rollout_random(usim_handle* h, int64_t first_step, int nsteps, const usim_step_io* io, int block_advance, void* stream);

/* Enqueues nsteps consecutive steps whose actions are the CALLER's: io->act_dev (required) is an action block [nsteps][n][A] and step k plays slice k -- a planner's
 * candidate sequences, a recorded trajectory to replay, an open-loop identification input, the zero actions of src/main.py.  Auto-reset is on.  The call equals nsteps
 * calls of usim_step(h, io_k, 1, stream) with act_dev = slice k, bit for bit: every output and the whole state afterwards, for every mapping, every steps_per_launch,
 * across the 256-step refill period of the reset bank, with warm_start, and with substeps > 1 (the action of a control step holds for all its physics substeps).  A
 * non-finite action component counts as 0, as in usim_step.  What it saves is the launch path: the steps run in the multi-step launches of usim_rollout_random (up to
 * usim_set_steps_per_launch steps each, never across the refill period; the full torso always launches step by step), which keep the state in registers and the
 * tables in LDS between steps and pay launch latency once.
 * block_advance governs the OUTPUT buffers only, exactly as in usim_rollout_random: 0 = every step writes the same buffers (they hold the last step's results
 * afterwards), != 0 = the non-NULL output buffers of io are rollout blocks [nsteps][n][...] and step k writes slice k.  The action block is indexed by step either
 * way.  act_out_dev is ignored (nothing is drawn).
 * nsteps == 0: USIM_OK, nothing enqueued.  A NULL handle, io, act_dev or required output buffer, or nsteps < 0: USIM_ERR_INVALID, nothing enqueued.  Capture: the
 * rules of usim_rollout_random and usim_step -- the refill counter lives on the host, so a recorded sequence starts and ends with usim_refill_bank. */
int usim_rollout_actions(usim_handle* h, int nsteps, const usim_step_io* io, int block_advance, void* stream);

/* Refill the reset bank now (the launch usim_step issues by itself every 256 steps: the initial states of the episodes that will reuse the ring slots
 * consumed since the last refill) and restart the 256-step period.  For callers that record a FIXED sequence of steps once and replay it -- a HIP
 * graph captured around T x usim_step (policy.GraphedCollector): the period counter lives on the host and does not advance at replay, so such a
 * sequence starts and ends with this call (every ring is then valid at every replay, whatever T).  Capture-safe: on a stream that is being captured
 * the library records kernel launches only (no events, no synchronising call).  Nothing in the reference corresponds to it (a reset there
 * recompiles the model, ultrasound.py:416-478). */
int usim_refill_bank(usim_handle* h, void* stream);

/* usim_rollout_random enqueues its steps in launches of up to `steps` consecutive steps each (1 .. 256, default 256 = the refill period of the reset
 * bank, which a launch never crosses; the 16- and 32-lane mappings -- the others always launch step by step): inside a launch the lattice tables stay in LDS and launch
 * latency is paid once, every step still writes its state and its slice of the rollout block to HBM.  A launch lasts as long as its slowest workgroup -- the one whose
 * environments had the most contacts --, so long launches also average that out: 4096 envs, us per step: 32 steps per launch 15.6, 64 14.7, 128 14.1, 256 13.6.  The
 * results do not depend on the value (bit for bit). */
int usim_set_steps_per_launch(usim_handle* h, int steps);
/* the value in force (the default, a usim_set_steps_per_launch call or the USIM_STEPS_PER_LAUNCH environment variable read by usim_create); < 0: error code */
int usim_get_steps_per_launch(const usim_handle* h);

/* Device time spent so far in the reset-bank refill launches of this handle (one every 256 steps with auto-reset: the initial-pose IK and
 * zero-torque forward pass of the episodes that will start next), from HIP events around them on their stream.  Blocks
 * until the refill launches issued so far have finished.  bench.py subtracts it from the event time of its step blocks to get the duration of
 * the step kernel alone -- the number a rocprofv3 kernel trace reports. */
int usim_refill_time(usim_handle* h, double* total_ms, long long* launches);

/* Like usim_rollout_random, bracketed by HIP events on `stream`; blocks until done and returns the elapsed
 * device time in milliseconds (bench.py roofline leg). */
int usim_time_steps(usim_handle* h, int64_t first_step, int nsteps, const usim_step_io* io, int block_advance, void* stream, float* elapsed_ms);

/* Checkpoint / inspection.  Host buffers; synchronises the device.
 * scalars [n][USIM_NSCALAR]: q[0..6] qd[7..13] q0[14..20] traj_start[21..23] traj_end[24..26] u0[27] vbar[28]
 * fzbar[29] fzprev[30] dfz[31] stiffness[32] damping[33] mu[34] t[35] has_touched[36] episode[37]
 * ep_return[38] status[39];  lattice [n][E][2] = (s, sdot) per element (may be NULL when E == 0). */
int usim_get_state(usim_handle* h, float* scalars, float* lattice);
int usim_set_state(usim_handle* h, const float* scalars, const float* lattice);
/* USIM_TORSO_FULL: host buffers [n][USIM_FULL_BODY_WORDS] of float64 -- the free torso body (MuJoCo's free joint, ultrasound.py:426-431): position (world), quaternion
 * (w x y z), linear velocity (world axes), angular velocity (body frame) = 13 words; then the warm start of the contact solve (the contact forces of the previous physics step:
 * [270][4] every element's table-contact force and friction multiplier, [8] the probe slots' elements, [16][4] their forces by geom).  float64: the device holds the position
 * relative to the robot base in float32, and base + position is exact in float64 -- what usim_get_body_state hands out restores the same bits.  usim_get_state /
 * usim_set_state carry the 270 sliders in `lattice`. */
#define USIM_FULL_BODY_WORDS (13 + 4 * 270 + 8 + 64)
int usim_get_body_state(usim_handle* h, double* body);
int usim_set_body_state(usim_handle* h, const double* body);
/* USIM_TORSO_TOP with warm_start = 1 (any other handle: USIM_ERR_INVALID): host buffers [n][USIM_WARM_WORDS] of float32 -- the kept contact list of the solver, the part of
 * the state that usim_get_state does not carry: [8] the element (0 .. 98) of each contact slot of the previous physics step, -1 for an empty slot; then [16][4] force
 * (normal, two tangents) and friction multiplier of the virtual contacts, contact A of slot c at c, contact B at 8 + c.  Synchronises the device.  usim_set_state empties the
 * list (a state set from outside starts cold); usim_set_warm_start after it restores a checkpoint exactly. */
#define USIM_WARM_WORDS (8 + 16 * 4)
int usim_get_warm_start(usim_handle* h, float* w);
int usim_set_warm_start(usim_handle* h, const float* w);

/* ---- snapshots: save, load and fork the state of environments ON THE DEVICE (robosuite's sim.get_state() / sim.set_state(), batched and indexed).  usim_get_state /
 * usim_set_state above go through the host, synchronise and rebuild every reset-bank ring: a checkpoint file.  These two stay inside a rollout loop: a shooting planner
 * that evaluates K action sequences from one state, two policies compared from identical states, a restart from stored states, a rewind after a probe step.
 *
 * A snapshot is a caller-owned device buffer snap_dev [m][W] of float32 rows, W = usim_snapshot_words(h), 16-byte aligned (every W is a multiple of 4 words; everything
 * moves as 16-byte accesses).  The library allocates nothing.  A row is an OPAQUE device format -- not usim_get_state's:
 *     words [0, 40)        the scalar state words in the order of usim_get_state's block, as the device holds them: words 0 - 6 are q - q0, the integer fields
 *                          (t, has_touched, episode, status) are int32 bit patterns
 *     words [40, 40 + L)   the lattice words: L = 0 (USIM_TORSO_NONE), 200 (USIM_TORSO_TOP: s and sdot of the 99 elements), 1712 (USIM_TORSO_FULL: the 270 sliders, the
 *                          free torso body and the warm start of its contact solve)
 *     then                 USIM_TORSO_TOP with warm_start = 1: the USIM_WARM_WORDS words of the solver's kept contact list (the elements as int32 bit patterns)
 * It is valid for the library version that wrote it, not a file format.
 *
 * usim_save_envs: row r receives the state of environment env_index_dev[r] (int32 [m]; NULL: environments 0 .. m - 1, which needs m <= n).  An index outside [0, n) leaves
 * its row as it is.  The handle is not modified.
 * usim_load_envs: environment i takes row row_of_env_dev[i] (int32 [n], required); a negative value, or one >= m, keeps the environment bit for bit.  Every word of the row is
 * written EXCEPT THE EPISODE COUNTER: the destination continues the saved episode -- trajectory, stiffness / damping / friction, t, has_touched, ep_return, status bits, lattice,
 * body, solver warm start -- under its own counter, and when that episode ends it goes on with ITS OWN next episode (counter + 1).  The reset bank of an environment is a ring
 * of the episodes that follow its own counter, and the refill orders it has outstanding name that counter; with the counter left alone both stay valid, so a load needs no bank
 * fill and touches no host counter.  (A load that restores the counter as well is usim_set_state, at the price of a reset.)  Stepping draws nothing per environment -- the only
 * per-environment streams are the reset draws, keyed (seed, env_offset + env, episode), and the synthetic actions of usim_rollout_random --, so environments that hold the same
 * row and are given the same actions compute the same bits until that episode ends.
 * Both: kernel launches on `stream` and nothing else -- no synchronisation, no event, no allocation; capture-safe like usim_refill_bank.  A NULL handle or buffer, m <= 0 or a
 * snap_dev off the 16-byte grid: USIM_ERR_INVALID, nothing enqueued.  There is no in-place fork: an environment read as a source while another launch lane writes it as a
 * destination would race; save, then load (vec_env.py fork).
 * Rows may be loaded into ANOTHER handle.  The caller's responsibility: equal usim_snapshot_words and an equal configuration -- torso, torso_shape, robot, mode, substeps, the
 * probe_* and solver fields (pgs_iters, pair_model, probe_geoms, warm_start), the physical constants.  The number of environments, env_offset, seed and the kernel mapping may differ. */
#define USIM_SNAPSHOT_WORDS_RIGID     40
#define USIM_SNAPSHOT_WORDS_TOP       240      /* 40 + 200 */
#define USIM_SNAPSHOT_WORDS_TOP_WARM  312      /* + USIM_WARM_WORDS */
#define USIM_SNAPSHOT_WORDS_FULL      1752     /* 40 + 1712 */
int usim_snapshot_words(const usim_handle* h);           /* one of the four; < 0: error code */
int usim_save_envs(usim_handle* h, const int32_t* env_index_dev, int m, float* snap_dev, void* stream);
int usim_load_envs(usim_handle* h, const float* snap_dev, int m, const int32_t* row_of_env_dev, void* stream);

/* Diagnostics: runs one step (in-kernel synthetic actions of `step`, auto-reset on) on the default stream, blocks, and returns
 * shader-clock stamps taken in workgroup 0: ticks[0..16] by wave 0 at the phase boundaries of the single-wave step
 * kernels, ticks[20..29] / ticks[30..38] by the arm wave / the lattice wave of the split kernel at their barriers (min(max_ticks, 64) words
 * are written, max_ticks >= 17).  Only the profiling build of the library (make -C csrc prof) carries the stamps; the production build
 * returns USIM_ERR_UNSUPPORTED. */
int usim_profile_step(usim_handle* h, const usim_step_io* io, int64_t step, uint64_t* ticks, int max_ticks);

/* ---- one step's results as ONE block, for callers that hand them to the host (numpy in / numpy out: the SB3 VecEnv protocol, vec_env.py step_async / step_wait).
 * Reads the buffers named in io -- obs_dev, rew_dev, done_dev required; term_obs_dev, ep_return_dev, ep_length_dev, status_dev may be NULL -- after the usim_step that
 * filled them, on the same stream, and writes packed_dev, a caller-owned device buffer of USIM_PACK_WORDS(n) 32-bit words, 16-byte aligned:
 *     word 0                      c, the number of environments whose episode ended in this step (int32 bits); words 1 - 3: zero
 *     words 4 .. 4 + 21 n         the head [n][USIM_PACK_HEAD_WORDS]: obs[19], rew, done as 0.0f / 1.0f
 *     then                        the episode list [c][USIM_PACK_EPISODE_WORDS], one row per finished environment IN ASCENDING ENVIRONMENT INDEX: env index (int32 bits),
 *                                 ep_length (int32 bits), ep_return, status (int32 bits), terminal_observation[19]; the words of a NULL buffer are zero.  Exactly c rows
 *                                 are written: rows c .. n - 1 keep what the buffer held
 * Every float is copied as its bits (a NaN stays the same NaN).  No handle, no allocation, no synchronisation: one kernel launch, capture-safe.  The block is a function
 * of the inputs alone (nothing is ordered by arrival).  n <= 0, a NULL io / required pointer / packed_dev or a packed_dev off the 16-byte grid: USIM_ERR_INVALID, nothing
 * is written.  A host that wants the results of a step copies 16 + 84 n bytes, reads c, and -- when c > 0 -- copies 92 c bytes more:
 *     float* packed_dev;  hipMalloc((void**)&packed_dev, USIM_PACK_WORDS(n) * 4);
 *     float* host = malloc(USIM_PACK_WORDS(n) * 4);  int32_t c;
 *     usim_step(h, &io, 1, stream);  usim_pack_step(&io, n, packed_dev, stream);
 *     hipMemcpyAsync(host, packed_dev, (4 + (size_t)n * USIM_PACK_HEAD_WORDS) * 4, hipMemcpyDeviceToHost, stream);  hipStreamSynchronize(stream);
 *     memcpy(&c, host, 4);                                              -- word 0
 *     const float* row_i = host + 4 + i * USIM_PACK_HEAD_WORDS;         -- row_i[0 .. 18] observation of env i, row_i[19] reward, row_i[20] != 0: episode ended
 *     if (c) hipMemcpy(host + 4 + (size_t)n * USIM_PACK_HEAD_WORDS, packed_dev + 4 + (size_t)n * USIM_PACK_HEAD_WORDS, (size_t)c * USIM_PACK_EPISODE_WORDS * 4, hipMemcpyDeviceToHost);
 *     const float* ep_k = host + 4 + (size_t)n * USIM_PACK_HEAD_WORDS + k * USIM_PACK_EPISODE_WORDS;    -- k < c: ep_k[0] env index, ep_k[1] length, ep_k[3] status (read as int32),
 *                                                                                                           ep_k[2] return, ep_k[4 .. 22] terminal observation */
#define USIM_PACK_HEAD_WORDS 21            /* obs[19], rew, done as 0.0f / 1.0f */
#define USIM_PACK_EPISODE_WORDS 23         /* env index (int32 bits), ep_length (int32 bits), ep_return, status (int32 bits; 0 when io->status_dev is NULL), terminal_observation[19] */
#define USIM_PACK_WORDS(n) (4 + (size_t)(n) * (USIM_PACK_HEAD_WORDS + USIM_PACK_EPISODE_WORDS))
int usim_pack_step(const usim_step_io* io, int n, float* packed_dev, void* stream);

/* ---- the score of a rollout block: for every environment the discounted return of its FIRST episode inside the block and that episode's length, in one launch -- the
 * scoring pass of a shooting planner after usim_rollout_actions, in place of 2 nsteps small tensor kernels (ret += rew * alive;
 * alive &= ~done).  rew_block_dev [nsteps][n] float32 and done_block_dev [nsteps][n] bytes are the rew / done blocks of a rollout.  For environment i:
 *     L = 1 + the first k with done[k][i] != 0 (any non-zero byte), or nsteps if there is none
 *     return_dev[i] = sum over k < L of gamma^k rew[k][i]          length_dev[i] = L  (int32; length_dev may be NULL)
 * Past its first done an environment of an auto-reset rollout plays an episode of its own: those words do not enter the sum (a NaN there does not reach the result).
 * The arithmetic is fixed -- float32, in step order, ret = fmaf(disc, r, ret); disc *= gamma; from ret = 0, disc = 1 --, so the result is a function of the inputs
 * alone; at gamma = 1 it is the float32 sum in step order.  No handle, no allocation, no synchronisation: one kernel launch, capture-safe.  A NULL buffer other than
 * length_dev, n <= 0 or nsteps <= 0: USIM_ERR_INVALID, nothing is written. */
int usim_score_block(const float* rew_block_dev, const uint8_t* done_block_dev, int nsteps, int n, float gamma, float* return_dev, int32_t* length_dev, void* stream);

/* ---- episode statistics on the device: SB3's Monitor + `ep_info_buffer = deque(maxlen = stats_window_size)` (the source of rollout/ep_rew_mean, the curve of
 * src/utils/plot.py:420-436; src/rl.py:39 wraps every environment in a Monitor), fed by one launch after every usim_step (csrc/usim_monitor.hip; monitor.py
 * DeviceMonitor, evaluate_policy).  usim_monitor_step reads io->done_dev, io->ep_return_dev and io->ep_length_dev of the step just taken (all three required; the
 * other members are ignored), on the same stream, and updates monitor_dev, a caller-owned device block of usim_monitor_words(window) 32-bit words, 16-byte aligned,
 * that lives across launches.  An all-zero block is an empty monitor.  The block:
 *     words 0 - 1      episodes    int64    episodes counted over the monitor's life
 *     words 2 - 3      length_sum  int64    sum of their lengths
 *     words 4 - 5      return_sum  float64  sum of their returns
 *     words 6 - 7      truncated   int64    counted episodes with ep_length >= horizon (horizon <= 0: none)
 *     words 8 - 9      launches    int64    + 1 per call
 *     words 10 - 15    zero
 *     words 16 ..      the ring: `window` rows of USIM_MONITOR_ROW_WORDS words {ep_return (its bits), ep_length (int32), environment index (int32), the low 32 bits of
 *                      `launches` as the call found it = the number of the launch, counted from 0}
 * Environment i is COUNTED in a launch iff done_dev[i] != 0 (any non-zero byte, as in usim_pack_step) and either target_dev == NULL or count_dev[i] < target_dev[i]
 * (int32 [n] each; SB3's evaluate_policy: "n episodes, at most target[i] of them from environment i"); count_dev[i] is then incremented.  The counted environments
 * are appended IN ASCENDING ENVIRONMENT INDEX, as _update_info_buffer(infos) walks them: episode number e, counted from 0 over the monitor's life, is ring row
 * e mod window, so the min(episodes, window) newest episodes are live and the oldest live one is row episodes mod window once the ring is full.  A launch that
 * counts more than `window` episodes stores only the last `window` of them (no row is stored twice in a launch).  Words of ep_return / ep_length of an environment
 * that is not counted are stale and enter nothing (a NaN there does not reach return_sum).  Floats travel as their bits into the ring.
 * One launch of one workgroup; return_sum is accumulated in float64 in an order fixed by the code (no floating-point atomics, nothing ordered by arrival): the same
 * block and the same inputs give the same block bit for bit.  No handle, no allocation, no synchronisation: capture-safe.  USIM_ERR_INVALID before anything is
 * enqueued: a NULL io, done_dev, ep_return_dev, ep_length_dev or monitor_dev, a monitor_dev off the 16-byte grid, n <= 0, a window outside 1 .. USIM_MONITOR_MAX_WINDOW,
 * target_dev without count_dev.
 *
 * usim_explained_variance: SB3's explained_variance(values, returns) = 1 - var(returns - values) / var(returns) (train/explained_variance) over `count` float32 words
 * each, to out_dev[0] as float32; NaN when var(returns) == 0.  One launch; float64 sums of the words shifted by their first element (a large mean does not cancel
 * the variance), in an order fixed by the code.  USIM_ERR_INVALID: a NULL pointer, count <= 0. */
#define USIM_MONITOR_HEADER_WORDS 16
#define USIM_MONITOR_ROW_WORDS     4
#define USIM_MONITOR_MAX_WINDOW   (1 << 20)
int usim_monitor_words(int window);   /* 16 + 4 * window 32-bit words; < 0: error code */
int usim_monitor_step(const usim_step_io* io, int n, int window, int horizon,
                      const int32_t* target_dev, int32_t* count_dev,
                      uint32_t* monitor_dev, void* stream);
int usim_explained_variance(const float* values_dev, const float* returns_dev,
                            int64_t count, float* out_dev, void* stream);

/* ---- error metrics and episode records of evaluation runs on the device (csrc/usim_metrics.hip; evaluation.py DeviceEpisodeMetrics, EpisodeRecorder,
 * evaluate_episodes).  The reference states its results as the thirteen numbers of src/utils/error.py:148-191 over the 24 CSV files that
 * ultrasound.py:552-614 dumps per episode; the step kernels emit every channel of those files for every environment (io->log_dev, [n][53] float32).  Both entry
 * points read io->log_dev and io->done_dev of the step just taken (both required; the other members are ignored) on the same stream, take no handle, allocate
 * nothing, synchronise nothing and decide nothing on the host: each call is the same launches whatever the data, and records into a HIP graph.
 *
 * usim_metrics_step updates metrics_dev, a caller-owned device block of usim_metrics_words(n, window) 32-bit words, 16-byte aligned, that lives across calls.  An
 * all-zero block is an empty one.  The block:
 *     words 0 - 1      episodes    int64    episodes counted over the block's life
 *     words 2 - 3      launches    int64    + 1 per call
 *     words 4 - 5      length_sum  int64    sum of their lengths
 *     words 6 - 7      nonfinite   int64    counted episodes with a metric that is not finite
 *     words 8 - 33     total[13]     float64  per metric, the sum over the counted episodes whose thirteen metrics are all finite
 *     words 34 - 59    total_sq[13]  float64  ... of their squares
 *     words 60 - 63    zero
 *     words 64 ..      the ring: `window` rows of USIM_METRICS_ROW_WORDS words {13 float64 metrics in the order of error_metrics.METRICS, environment index (int32),
 *                      episode length (int32), the low 32 bits of `launches` as the call found it, three zero words}
 *     words 64 + 32 window ..   the accumulators, float64 [n][13]
 * Every call, for every environment i: acc[i][m] += term_m(row i of log_dev), the summands of error_metrics.step_terms in float64 on the float32 words widened first
 * -- (a - b)^2 for x_pos (columns 0, 3), y_pos (1, 4), force (20, 21), mean_force (22, 21), der_force (23, 24), mean_velocity (10, 9); (sqrt(vx^2 + vy^2 + vz^2) -
 * goal)^2 over columns 6 - 8 and 9 for velocity; the columns 19, 41, 42, 44, 45, 43 themselves for quat_diff and the pos / ori / force / der_force / vel rewards.
 * Where done_dev[i] != 0 (any non-zero byte) the finished metrics are acc[i] / horizon (zero rows add nothing to the reference's means over `horizon` rows), the
 * episode length is t + 1 with t = rint((double)row[40] * horizon / 100) (the time channel; episode_log.EpisodeLogger's rule), and acc[i] is zeroed -- counted or not.
 * The environment is COUNTED by usim_monitor_step's rule: target_dev == NULL or count_dev[i] < target_dev[i], then count_dev[i]++ (int32 [n] each; a count array of
 * this entry point's own, not the monitor's).  Counted environments are appended IN ASCENDING ENVIRONMENT INDEX: episode e, counted from 0 over the block's life, is
 * ring row e mod window; a call that counts more than `window` stores only the last `window` of them.  total, total_sq and length_sum are added in that same order,
 * one episode after the other.  A counted episode with a non-finite metric is stored in the ring as it is, adds 1 to nonfinite and nothing to total / total_sq.
 * Two launches per call: the accumulation over a grid (coalesced reads of the record), then the ordered append in one workgroup.  No floating-point atomics, nothing
 * ordered by arrival: the same block and the same inputs give the same block bit for bit.  USIM_ERR_INVALID before anything is enqueued: a NULL io, log_dev, done_dev
 * or metrics_dev, a metrics_dev off the 16-byte grid, n <= 0, horizon <= 0, a window outside 1 .. USIM_MONITOR_MAX_WINDOW, target_dev without count_dev.
 *
 * usim_record_step keeps whole episodes of m chosen environments: record_dev is a caller-owned block of usim_record_words(m, episodes, horizon) 32-bit words, 16-byte
 * aligned, all zero = empty:
 *     filled[m] int32, lengths[m][episodes] int32, zero words up to a multiple of 4, then float32 rows[m][episodes][horizon][53]
 * For tracked row r with e = env_index_dev[r] (int32 [m], distinct): while filled[r] < episodes, row e of log_dev is copied, as its bits, into
 * rows[r][filled[r]][t], t by the rule above; where done_dev[e] != 0, lengths[r][filled[r]] = t + 1 and filled[r]++.  Rows an episode never reached stay zero, as
 * the reference's np.zeros(horizon, ...) buffers do; after `episodes` episodes a row records nothing more.  e and t come from device memory and are checked by the
 * kernel: an index outside [0, n) writes nothing at all, a t outside [0, horizon) copies no row.  One launch.  USIM_ERR_INVALID: a NULL io, log_dev, done_dev,
 * env_index_dev or record_dev, a record_dev off the 16-byte grid, n, m, episodes or horizon <= 0. */
#define USIM_METRICS               13   /* order of error_metrics.METRICS */
#define USIM_METRICS_HEADER_WORDS  64
#define USIM_METRICS_ROW_WORDS     32
int usim_metrics_words(int n, int window);   /* 64 + 32*window + 26*n 32-bit words; < 0: error code */
int usim_metrics_step(const usim_step_io* io, int n, int window, int horizon,
                      const int32_t* target_dev, int32_t* count_dev,
                      uint32_t* metrics_dev, void* stream);
int usim_record_words(int m, int episodes, int horizon);  /* 4*ceil((m + m*episodes)/4) + m*episodes*horizon*53; < 0: error */
int usim_record_step(const usim_step_io* io, int n, int horizon, const int32_t* env_index_dev,
                     int m, int episodes, float* record_dev, void* stream);

/* ---- a batched MPPI shooting planner: the sampler before usim_rollout_actions and the update after usim_score_block (csrc/usim_plan.hip; planner.py MPPIPlanner;
 * INTEGRATION.md section 4c).  `groups` = G controlled environments, `per_group` = K candidates each, n = G K simulated environments: environments [g K, (g + 1) K)
 * play the candidates of group g, and candidate k = 0 of every group is the unperturbed nominal.  Caller-owned float32 device buffers: the nominal mean [G][H][A]
 * (H = horizon, A = act_dim), the candidate block cand [H][n][A] -- the layout usim_rollout_actions consumes --, the returns ret [n].  Both calls take no handle and
 * are kernel launches on `stream` and nothing else -- no allocation, no synchronisation, no event; capture-safe like usim_score_block.  Both answer USIM_ERR_INVALID
 * before anything is enqueued for a NULL required pointer, groups / per_group / horizon <= 0 (or G K, G H beyond INT_MAX), act_dim outside 1 .. 8, smoothing outside
 * [0, 1), a temperature that is negative or not finite.
 *
 * usim_plan_sample:   cand[t][g K + k][a] = clip(m[g][t][a] + sigma[a] e[k][t][a], low[a], high[a])
 *   m is mean_dev; a non-finite word counts as 0, as an action does in usim_step.  Where restart_dev[g] != 0 (uint8 [G], may be NULL: no restart) m is taken as 0
 *   AND 0 IS WRITTEN INTO mean_dev[g]: an environment that has just started an episode starts from a fresh nominal.  Nothing else writes mean_dev.
 *   e = 0 for k = 0.  For k >= 1 the noise is first-order smoothed over the horizon: e[0] = xi[0], e[t] = smoothing e[t - 1] + sqrt(1 - smoothing^2) xi[t]
 *   (float32: fmaf(smoothing, e[t - 1], c xi[t]) with c rounded once from float64); the sample is fmaf(sigma, e, m), then the clip.
 *   xi is N(0, 1) by the Box-Muller recipe of usim_policy_step -- one Philox4x32-10 block per pair of components, u1 = ((word 0 >> 8) + 1) / 2^24, u2 = (word 1 >> 8)
 *   / 2^24, radius sqrt(-2 ln u1), cosine for even components and sine for odd ones, hardware log / sine / cosine -- keyed by the counter words
 *   (g K + k, (counter + *counter_base_dev) mod 2^32, 4 t + (a >> 1), 0x504c414e "PLAN") under the key (seed low, seed high).  counter_base_dev (may be NULL) is a device
 *   word that a recorded sequence advances between replays.  A draw depends on (seed, counter, candidate g K + k, t, a) alone -- not on G, K, H or the launch shape.
 *
 * usim_plan_update, per group g:
 *   best = the candidate with the largest FINITE return, ties to the lowest index; a candidate with a non-finite return has weight 0; if no return of the group is
 *   finite, best = 0 and the weight is 1 on candidate 0.
 *   temperature == 0 is a SELECTION, not a product: the weight is exactly 1 on best and plan[g][t] is that candidate's words bit for bit (no clip).
 *   temperature > 0: w_k = exp((ret_k - ret_best) / temperature) / sum_j exp((ret_j - ret_best) / temperature),  plan[g][t][a] = clip(sum_k w_k cand[t][g K + k][a], low, high).
 *   act[g] = plan[g][0];  next_mean[g][t] = plan[g][t + 1] for t < H - 1 and next_mean[g][H - 1] = plan[g][H - 1] (the receding horizon keeps the last action).
 *   Outputs: plan_dev [G][H][A], next_mean_dev [G][H][A], best_dev [G] int32 and weight_dev [n] may be NULL; act_dev [G][A] is required.  next_mean_dev may be the
 *   mean_dev of the next usim_plan_sample (this call does not read the nominal); the outputs must not overlap each other or the inputs.
 *   The result is a function of the inputs alone: float32 in a fixed order -- thread j of 256 takes candidates j, j + 256, ... ascending (s += term; acc = fmaf(w, cand,
 *   acc)), a butterfly over lane distances 32 .. 1 inside each wave of 64, then ((w0 + w1) + w2) + w3 over the four waves; no atomics, nothing ordered by arrival.  The
 *   result of a group does not depend on the other groups. */
int usim_plan_sample(float* mean_dev, const float* sigma_dev, const float* act_low_dev, const float* act_high_dev, const uint8_t* restart_dev, int groups, int per_group,
                     int horizon, int act_dim, float smoothing, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev, float* cand_dev, void* stream);
int usim_plan_update(const float* cand_dev, const float* ret_dev, const float* act_low_dev, const float* act_high_dev, int groups, int per_group, int horizon, int act_dim,
                     float temperature, float* plan_dev, float* next_mean_dev, float* act_dev, int32_t* best_dev, float* weight_dev, void* stream);

/* ---- the guided planner: a critic's value behind the horizon, the actor's action as the tail of the nominal, cross-entropy refits inside a control step
 * (csrc/usim_score.hip, csrc/usim_plan.hip; planner.py MPPIPlanner(critic=, tail_action=, iterations=)).  The four calls keep the contract
 * of usim_plan_*: no handle; kernel launches on `stream` and nothing else -- no allocation, no synchronisation, capture-safe --; float32 in an order fixed by the code,
 * no floating-point atomics, nothing ordered by arrival, so the result is a function of the inputs alone and the result of a group (of an environment, for the score)
 * does not depend on the others.  USIM_ERR_INVALID before anything is enqueued: a NULL required pointer, a size <= 0 (or G K, G H beyond INT_MAX), act_dim outside
 * 1 .. 8, a scalar that is not finite or outside the range stated below.
 *
 * usim_score_block_tail: usim_score_block -- the same loop, the same bits for return_dev and length_dev -- and then, for an environment with NO done inside the block,
 *     return_dev[i] = fmaf(disc_T, s * tail_dev[i], return_dev[i])
 *   disc_T is the loop's own running discount after its nsteps steps (disc = 1; disc *= gamma per step, float32);  s = (float)sqrt(*ret_var_dev + epsilon), the sum
 *   and the root in float64 -- a critic trained under VecNormalize's norm_reward speaks in units of normalised return, s takes its value back to raw reward
 *   (usim_norm_stats.ret_var / .epsilon); ret_var_dev == NULL: s = 1 (epsilon is then unused).  tail_dev [n] of an environment that ended inside the block -- on its
 *   last step included -- is never read: a NaN there has no effect.  A non-finite tail of a survivor makes its return non-finite (usim_plan_update gives such a
 *   candidate weight 0).  tail_dev == NULL: usim_score_block.  gamma and epsilon must be finite, epsilon >= 0; length_dev may be NULL.
 *
 * usim_plan_sample_elem: usim_plan_sample with sigma_elem_dev [G][H][A] in place of sigma_dev [A]: the sample is fmaf(sigma_elem[g][t][a], e, m).  Noise keys, smoothing,
 *   restart handling (sigma_elem_dev is not touched by a restart) and clip are usim_plan_sample's; with sigma_elem[g][t][a] = sigma[a] so are the bits.
 *
 * usim_plan_refit: one cross-entropy refit of (mean_dev, sigma_elem_dev), both [G][H][A] and updated in place, per group g from cand_dev [H][n][A] and ret_dev [n]:
 *   the ELITE SET is the min(elites, number of finite returns) candidates with the largest finite returns under the total order "larger return, then lower index"
 *   (+0 and -0 are equal); a candidate with a non-finite return is never elite.  elite_dev [G][elites] int32 (may be NULL) receives the group's elite indices k in
 *   ASCENDING candidate index, padded with -1.  With E elites x_1 .. x_E = cand[t][g K + k][a] taken in that ascending order, per word (t, a), float32:
 *     s = s + x_i from 0;  m = s / E;   q = fmaf(d_i, d_i, q) from 0 with d_i = x_i - m;  sd = sqrtf(q / E)     (the population variance about m)
 *     mean[g][t][a]  = clip(fmaf(momentum, mean_old, c m), low[a], high[a])        c = (float)(1 - (double)momentum), rounded once on the host
 *     sigma[g][t][a] = fmaxf(fmaf(momentum, sigma_old, c sd), sigma_min)           a non-finite word of mean_old counts as 0, as in the sampler
 *   A group without a finite return keeps its mean and sigma bit for bit and gets all -1.  elites in 1 .. K, momentum in [0, 1), sigma_min > 0 and finite.
 *   K <= USIM_PLAN_REFIT_MAX_K = 4096, a larger per_group is refused: one workgroup per group ranks the group ONCE -- its K returns in LDS (9 K bytes with the list and
 *   the flags: 36 KB at the limit), every candidate's rank by counting, K^2 / 256 comparisons per thread (65536 at the limit, about 0.1 ms) -- and then reduces the
 *   H A words, one thread per word; twice the K would quadruple the ranking time of a launch that runs between 18 us simulator steps.
 *
 * usim_plan_tail: the actor's action at each candidate's final observation as that candidate's step H, into the LAST step of the shifted nominal:
 *     x_k = pol_act_dev[g K + k]   where length_dev[g K + k] == H and done_last_dev[g K + k] == 0  (the candidate played all H steps and did not end on the last one)
 *     x_k = cand[H - 1][g K + k]   otherwise (its own last action, what usim_plan_update keeps there)
 *   length_dev [n] int32 is usim_score_block's, which is H both for a survivor and for an episode that ended on step H; done_last_dev [n] uint8 is the slice
 *   done[H - 1] of the rollout block and tells them apart.  pol_act_dev [n][A] of a candidate that ended is never read.
 *   temperature > 0:  next_mean[g][H - 1][a] = clip(sum_k w_k x_k[a], low[a], high[a])  with w = weight_dev [n] as usim_plan_update wrote it, in that kernel's three
 *   stages (thread j of 256 takes k = j, j + 256, ... ascending, acc = fmaf(w_k, x_k, acc) from 0; the butterfly 32 .. 1 inside a wave; ((w0 + w1) + w2) + w3);
 *   a candidate with w_k == 0 is skipped -- the same bits for every finite x_k, and a non-finite action without weight does not reach the nominal.
 *   temperature == 0:  next_mean[g][H - 1] = x_best, best = best_dev[g], bit for bit (no clip); a best_dev[g] outside [0, K) writes nothing.
 *   No other word of next_mean_dev is written; call it after the usim_plan_update that wrote next_mean_dev, on the same stream.  All pointers are required. */
#define USIM_PLAN_REFIT_MAX_K 4096
int usim_score_block_tail(const float* rew_block_dev, const uint8_t* done_block_dev, int nsteps, int n, float gamma, const float* tail_dev, const double* ret_var_dev,
                          double epsilon, float* return_dev, int32_t* length_dev, void* stream);
int usim_plan_sample_elem(float* mean_dev, const float* sigma_elem_dev, const float* act_low_dev, const float* act_high_dev, const uint8_t* restart_dev, int groups,
                          int per_group, int horizon, int act_dim, float smoothing, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev, float* cand_dev,
                          void* stream);
int usim_plan_refit(const float* cand_dev, const float* ret_dev, const float* act_low_dev, const float* act_high_dev, int groups, int per_group, int horizon, int act_dim,
                    int elites, float momentum, float sigma_min, float* mean_dev, float* sigma_elem_dev, int32_t* elite_dev, void* stream);
int usim_plan_tail(const float* cand_dev, const float* weight_dev, const int32_t* best_dev, const int32_t* length_dev, const uint8_t* done_last_dev,
                   const float* pol_act_dev, const float* act_low_dev, const float* act_high_dev, int groups, int per_group, int horizon, int act_dim, float temperature,
                   float* next_mean_dev, void* stream);

/* ---- the caller's side of env.step() on the device: SB3 VecNormalize + MlpPolicy forward + sampling + rollout-buffer
 * writes + GAE, fused into a few kernels per rollout step (csrc/usim_policy.hip).  Everything is a device pointer into the CALLER's tensors
 * (torch parameters, policy.DeviceVecNormalize statistics, policy.DeviceRolloutBuffer slices); the library keeps no copy. ---- */
typedef struct usim_policy_net {               /* stable_baselines3 ActorCriticPolicy("MlpPolicy", net_arch pi=[256,128] vf=[256,128], tanh) of the shipped
                                                * checkpoints (src/rl.py:143; trained_rl_models/.zip policy.pth); torch.nn.Linear layout weight[out][in] */
    const float *pi_w1, *pi_b1, *pi_w2, *pi_b2;        /* mlp_extractor.policy_net: [256][19], [256], [128][256], [128] */
    const float *act_w, *act_b;                        /* action_net: [A][128], [A] */
    const float *vf_w1, *vf_b1, *vf_w2, *vf_b2;        /* mlp_extractor.value_net */
    const float *val_w, *val_b;                        /* value_net: [1][128], [1] */
    const float* log_std;                              /* [A] */
    const float* w2_packed;                            /* REQUIRED: USIM_POLICY_PACKED floats filled by usim_policy_pack from pi_w2 / vf_w2 as they are NOW -- the two layer-2
                                                        * matrices in the order the matrix-core operands are consumed, every word split into two float16 (hi + lo: layer 2 runs
                                                        * as three float16 products with float32 accumulation, 2^-22 relative).  Pack again after every change of the weights
                                                        * (policy.FusedRollout: before every eager launch, and as the first policy node of a recorded rollout) */
} usim_policy_net;
#define USIM_POLICY_PACKED (2 * 128 * 256)
int usim_policy_pack(const usim_policy_net* net, float* packed_dev, void* stream);

typedef struct usim_norm_stats {               /* stable_baselines3 VecNormalize (src/rl.py:140,177-184): RunningMeanStd of observations and of discounted returns */
    double *obs_mean, *obs_var, *obs_count;            /* [19], [19], scalar -- updated in place when training */
    double *ret_mean, *ret_var, *ret_count;            /* scalars */
    double* returns;                                   /* [n] discounted return accumulators */
    double* scratch;                                   /* USIM_POLICY_SCRATCH doubles of workspace, zero-initialised by the caller once (required when training) */
    double clip_obs, clip_reward, gamma, epsilon;      /* 10, 10, 0.99, 1e-8 in the shipped pickles */
} usim_norm_stats;

#define USIM_POLICY_SCRATCH 1280               /* 32 x 19 x 2 partial sums + an arrival counter */

typedef struct usim_policy_out {
    float* act_env_dev;        /* [n][A] REQUIRED: the sampled action clipped to the action box = the `action` argument of the following usim_step */
    float* nobs_dev;           /* [n][19] normalised observation            -> RolloutBuffer.observations[t]   (may be NULL, like the rest) */
    float* act_dev;            /* [n][A]  unclipped sample                  -> RolloutBuffer.actions[t] */
    float* value_dev;          /* [n]     value_net output                  -> RolloutBuffer.values[t] */
    float* logp_dev;           /* [n]     log-probability of the sample     -> RolloutBuffer.log_probs[t] */
    float* episode_start_dev;  /* [n]     1.0 where the previous step ended an episode -> RolloutBuffer.episode_starts[t] */
} usim_policy_out;

/* VecNormalize.normalize_obs (+ RunningMeanStd.update when training) -> ActorCriticPolicy.forward -> sample -> clip, for the n environments whose raw
 * observations are obs_dev [n][19].  prev_done_dev [n]: done flags of the previous step (NULL: every environment starts an episode).  The Gaussian
 * noise comes from a counter-based stream keyed (seed, env_offset + env, counter + *counter_base_dev): a new value per call -- counter from the host,
 * counter_base_dev (may be NULL) a device word that a recorded sequence of calls (HIP graph) advances between replays.  deterministic != 0: the
 * mean action.  training: 0 = statistics frozen, 1 = update them with obs_dev first, 2 = they already contain obs_dev (see usim_policy_reward). */
int usim_policy_step(const usim_policy_net* net, const usim_norm_stats* st, const float* obs_dev, const uint8_t* prev_done_dev, int n, int act_dim,
                     const float* act_low_dev, const float* act_high_dev, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev, int env_offset,
                     int training, int deterministic, const usim_policy_out* out, void* stream);
/* The same step with BOTH halves of VecNormalize.step_wait inside the policy launch (two launches per rollout step: this one and usim_step), statistics
 * updated in place.  update_obs: RunningMeanStd.update(obs_dev) before it is normalised (the observation an env step returned; 0 where the statistics have
 * already seen obs_dev).  have_prev: the reward side of the step BEFORE this observation -- rew_prev_dev / done_prev_dev [n] (the env's buffers, not yet
 * overwritten), nrew_prev_dev [n] receives the normalised reward; raw_sum_dev (may be NULL) += the sum of the raw rewards.  The workgroups exchange their
 * partial sums inside the launch and wait for one another (bounded), which needs all of them resident: n <= USIM_POLICY_FUSED_MAX_ENVS, else
 * USIM_ERR_UNSUPPORTED (use usim_policy_step + usim_policy_reward), and nothing else running on the device beside the launch.  work_dev: USIM_POLICY_FUSED_WORK(n)
 * doubles, zero-initialised once; counter + *counter_base_dev must not repeat for a workspace (it stamps the arrival flags).  After a synchronisation,
 * the 32-bit word behind the 2 x USIM_POLICY_FUSED_ROWS(n) flags that follow the rows is non-zero if a wait ever ran out. */
#define USIM_POLICY_FUSED_MAX_ENVS 8192
#define USIM_POLICY_FUSED_ROWS(n) (((n) + 31) / 32)
#define USIM_POLICY_FUSED_WORK(n) (USIM_POLICY_FUSED_ROWS(n) * 49 + 2)
typedef struct usim_policy_fused {
    double* work_dev;                /* USIM_POLICY_FUSED_WORK(n) doubles: one row of 48 per 32 environments (partial sums), then the arrival flags and a status word */
    const float* rew_prev_dev; const uint8_t* done_prev_dev; float* nrew_prev_dev; double* raw_sum_dev;
    int32_t update_obs, have_prev, norm_reward, reserved_;
} usim_policy_fused;
int usim_policy_step_fused(const usim_policy_net* net, const usim_norm_stats* st, const usim_policy_fused* f, const float* obs_dev, const uint8_t* prev_done_dev, int n,
                           int act_dim, const float* act_low_dev, const float* act_high_dev, uint64_t seed, uint32_t counter, const uint32_t* counter_base_dev,
                           int env_offset, int deterministic, const usim_policy_out* out, void* stream);
/* VecNormalize's reward side after the env step: returns = gamma returns + rew, RunningMeanStd.update(returns), nrew = clip(rew / sqrt(ret_var + eps)),
 * returns reset where done.  raw_sum_dev (may be NULL): += sum of the raw rewards.  next_obs_dev (may be NULL; used when training): the observation the step
 * returned -- its RunningMeanStd.update is made in the same launch (as VecNormalize.step_wait does, before the observation is normalised); the
 * usim_policy_step that consumes that observation is then called with training = 2 ("statistics already updated with this observation"). */
int usim_policy_reward(const usim_norm_stats* st, const float* rew_dev, const uint8_t* done_dev, int n, int training, int norm_reward, float* nrew_dev,
                       double* raw_sum_dev, const float* next_obs_dev, void* stream);
/* Time-limit bootstrap of OnPolicyAlgorithm.collect_rollouts (`rewards[idx] += gamma * V(terminal_observation)` where infos[idx]["TimeLimit.truncated"]),
 * for the step whose usim_step_io buffers are term_obs_dev [n][19], done_dev [n] and ep_length_dev [n].  Environment i is TRUNCATED iff done_dev[i] != 0 &&
 * ep_length_dev[i] >= horizon (ep_length_dev is stale where not done; an early termination that falls on the horizon step counts as truncated, as in the numpy
 * path's infos).  For those, rew_dev[i] = fmaf(gamma, V(nobs_i), rew_dev[i]) with
 *   nobs_i = clip((term_obs_i - obs_mean) * (1 / sqrt(obs_var + epsilon)), +-clip_obs)   in float64, rounded to float32 -- usim_policy_step's arithmetic with
 *                                                                                       training = 0: the statistics are read, never updated
 *   V      = value_net(tanh(vf_2(tanh(vf_1(nobs)))))                                     float32 fmaf in a fixed order per environment, tanh as in usim_policy_step
 * No other word of rew_dev is written, and no row of term_obs_dev of an environment that is not truncated is read (a NaN there has no effect).  An environment's
 * result depends on its own inputs only -- not on n, on which other environments are truncated or on the device -- and the same inputs give the same bits on every
 * call (no floating-point atomics).  count_dev (may be NULL): += the number of truncated environments.  Call it after rew_dev holds the (normalised) rewards of the
 * step and before the next usim_step rewrites the env's buffers; VecNormalize.step_wait normalises the terminal observation with statistics that already contain the
 * step's new observation, so it goes after the launch that updates them (usim_policy_reward with next_obs_dev, or the usim_policy_step_fused of the next step).
 * Reads vf_w1 vf_b1 vf_w2 vf_b2 val_w val_b of the net (plain float32, torch.nn.Linear layout) and obs_mean / obs_var / epsilon / clip_obs of the statistics; the
 * policy-side pointers, log_std and w2_packed are ignored and may be NULL (no usim_policy_pack needed).  One kernel launch on `stream` and nothing else: capture-safe.
 * A workgroup of 32 environments that has no truncated one -- the common case -- returns after reading its flags.
 * USIM_ERR_INVALID, before anything is enqueued and with nothing written: a NULL net, st, term_obs_dev, done_dev, ep_length_dev or rew_dev; a NULL vf_* / val_*
 * pointer, obs_mean or obs_var; n <= 0 or horizon <= 0; a gamma that is not finite or outside [0, 1]. */
int usim_policy_bootstrap(const usim_policy_net* net, const usim_norm_stats* st, const float* term_obs_dev, const uint8_t* done_dev, const int32_t* ep_length_dev,
                          int n, int horizon, float gamma, float* rew_dev, int32_t* count_dev, void* stream);
/* RolloutBuffer.compute_returns_and_advantage over [T][n] buffers (GAE(lambda), SB3's recursion) */
int usim_policy_gae(const float* rewards_dev, const float* values_dev, const float* episode_starts_dev, const float* last_values_dev, const uint8_t* last_done_dev,
                    int T, int n, float gamma, float gae_lambda, float* advantages_dev, float* returns_dev, void* stream);

/* ---- policy populations: K networks ("members") in one rollout (population.py).  n = K G environments, member k owning environments
 * [k G, (k + 1) G) of every [n]... buffer; K = members, G = envs_per_member, A = act_dim, P = usim_ppo_params(A).  The three calls take no handle, are kernel launches on
 * `stream` and nothing else (capture-safe: no allocation, no synchronisation, no host read of device memory) and use no floating-point atomics.  Shared layout:
 *   theta_dev   [K][stride] floats: row k is member k's flat parameter block in the field order of usim_ppo_params (pi_w1 pi_b1 pi_w2 pi_b2 act_w act_b vf_w1 vf_b1
 *               vf_w2 vf_b2 val_w val_b log_std); stride >= P and a multiple of 4 (words behind P in a row are never read)
 *   packed_dev  [K][USIM_POLICY_PACKED] floats on the 16-byte grid: row k is what usim_policy_pack writes for member k
 *   st          a usim_norm_stats whose pointers hold K consecutive copies of what they hold for one network: obs_mean / obs_var [K][19]; obs_count, ret_mean, ret_var,
 *               ret_count [K]; returns [n] (member k's accumulators are its environments'); scratch [K][USIM_POLICY_SCRATCH], zero-initialised once; clip_obs,
 *               clip_reward, gamma and epsilon are shared by all members
 * Each call computes, bit for bit -- every output word and every word of the statistics --, what K calls of its single-network counterpart compute, call k made with
 * member k's network and statistics, the slices [k G, (k + 1) G) of every per-environment buffer, n = G and (usim_policy_step) env_offset + k G.  A member reads and
 * writes its own rows only: a NaN in another member's observations, weights or statistics does not reach it.  Any G >= 1: a member's last workgroup handles its tail as
 * the single-network call handles n % 32.
 * USIM_ERR_INVALID before anything is enqueued: a NULL required pointer (named per call below), members or envs_per_member <= 0, K G beyond INT_MAX,
 * members > USIM_POLICY_MAX_MEMBERS (the member is a grid axis), act_dim outside 1 .. 8 (usim_policy_step itself accepts 1 .. 7: at 8 the equality above has no
 * single-network side), stride < P or not a multiple of 4, packed_dev off the 16-byte grid.
 *
 * usim_policy_pack_multi: one launch, grid (64, K).  Required: theta_dev, packed_dev.  Pack again after every change of any member's weights.
 * usim_policy_step_multi: usim_policy_step for every member -- grid (ceil(G / 32), 2, K), preceded when training == 1 by the statistics launch, grid (32, K).
 *   obs_dev [n][19], prev_done_dev [n] or NULL, act_low_dev / act_high_dev [A] (shared), out: [n]... buffers as for usim_policy_step.  Required: theta_dev, packed_dev,
 *   st with obs_mean and obs_var (training == 1: obs_count and scratch too), obs_dev, act_low_dev, act_high_dev, out, out->act_env_dev.  There is no multi form of
 *   usim_policy_step_fused (its cross-workgroup wait would have to become per member) nor of usim_policy_bootstrap; usim_policy_gae is per environment and serves as it is.
 * usim_policy_reward_multi: usim_policy_reward for every member in one launch -- grid (33, K) with next_obs_dev [n][19] while training, else (1, K).  raw_sum_dev: [K]
 *   doubles or NULL, member k's sum of raw rewards is added to word k.  Required: st with ret_var (training: ret_mean, ret_count, returns; with next_obs_dev also obs_mean,
 *   obs_var, obs_count, scratch), rew_dev, done_dev, nrew_dev. ---- */
#define USIM_POLICY_MAX_MEMBERS 65535
int usim_policy_pack_multi(const float* theta_dev, int stride, int members, int act_dim, float* packed_dev, void* stream);
int usim_policy_step_multi(const float* theta_dev, int stride, const float* packed_dev, const usim_norm_stats* st, const float* obs_dev, const uint8_t* prev_done_dev,
                           int members, int envs_per_member, int act_dim, const float* act_low_dev, const float* act_high_dev, uint64_t seed, uint32_t counter,
                           const uint32_t* counter_base_dev, int env_offset, int training, int deterministic, const usim_policy_out* out, void* stream);
int usim_policy_reward_multi(const usim_norm_stats* st, const float* rew_dev, const uint8_t* done_dev, int members, int envs_per_member, int training, int norm_reward,
                             float* nrew_dev, double* raw_sum_dev, const float* next_obs_dev, void* stream);

/* ---- the learner: one PPO minibatch step on the device (csrc/usim_ppo.hip; ppo.py NativePPO) -- the loss of stable-baselines3's
 * PPO.train on one minibatch of the rollout buffer with its gradient for every parameter of the usim_policy_net above (A <= 8), and clip_grad_norm_ +
 * torch.optim.Adam.step on one flat parameter block.  Both calls check their arguments before anything is enqueued (USIM_ERR_INVALID: a NULL required pointer, act_dim
 * outside 1 .. 8, batch < 1, rows < batch without an index list, a non-finite or negative clip_range / lr / eps, a non-finite coefficient, a beta outside [0, 1), a
 * work_dev off the 16-byte grid) and are kernel launches on `stream` and nothing else -- no allocation, no synchronisation, no host read of device memory: a grad + adam
 * pair can be captured into a graph as one chain.  Every sum over samples or workgroups has a fixed order (no floating-point atomics; USIM_PPO_WORKGROUPS partial
 * blocks, whatever the device), so the same inputs give the same bits on every call.
 *
 * usim_ppo_grad, per sample, with Ad the advantage after the optional per-minibatch normalisation (Ad - mean) / (std + 1e-8) (float64, unbiased std as torch.std;
 * skipped when batch == 1), log-prob the DiagGaussianDistribution.log_prob of act under (mean(obs), log_std), r = exp(log-prob - old_logp), c = clip_range:
 *   policy term  -min(Ad r, Ad clip(r, 1 - c, 1 + c))      (a gradient passes unless Ad > 0 and r > 1 + c, or Ad < 0 and r < 1 - c)
 *   value term   (ret - V(obs))^2                          entropy  sum log_std + A / 2 (1 + log 2 pi)
 *   loss = mean(policy) + vf_coef mean(value) - ent_coef entropy
 * grad_dev[usim_ppo_params(A)] receives d loss / d parameter in the flat order below; stats_dev[USIM_PPO_STATS]: policy_loss, value_loss, entropy_loss (= -entropy),
 * approx_kl (mean((r - 1) - log r)), clip_fraction (mean(|r - 1| > c)), loss, the gradient's 2-norm, 0.  w2_packed of the net is ignored.  An index outside
 * [0, rows) reads the nearest row of the buffer.  work_dev: usim_ppo_work_floats(A) floats on the 16-byte grid; the call rewrites every word it reads, so the
 * workspace needs no clearing between calls (zero it once for a defined first state).
 *
 * usim_ppo_adam: g' = g min(1, max_grad_norm / (|g| + 1e-6)) (max_grad_norm <= 0: no clipping); *step_dev += 1 on the device, t = *step_dev;
 *   m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;  theta -= lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * in float64 on the float32 words, each result rounded once.  The norm is formed here from grad_dev (the two calls are independent); stats_dev may be NULL, otherwise
 * slot 6 receives the norm used.
 *
 * clip_range_vf > 0 (SB3's clip_range_vf; 0 is its None), with old = old_value_dev[row] and c = clip_range_vf: the value term becomes (ret - Vp)^2 with
 * Vp = old + clamp(V - old, -c, c).  Where |V - old| <= c (the closed interval, as torch's clamp passes its gradient) Vp is V itself and the row and its gradient
 * 2 vf_coef (V - ret) / batch are the unclipped ones; elsewhere the row takes old +- c formed in float32 and its gradient is exactly 0.  With clip_range_vf == 0
 * old_value_dev is not read and the call computes the bits it computes without the field.
 *
 * The gate: target_kl's early stop of PPO.train as a decision taken on the device.  gate_dev points to USIM_PPO_GATE_WORDS int32 words that the caller clears at
 * the start of an update: [0] stop flag (0 or 1), [1] gradient calls evaluated since the words were cleared, [2] optimizer steps applied since then, [3] 0.
 * Every kernel of usim_ppo_grad reads [0] on entry.  Set: the call is a no-op -- grad_dev, stats_dev and the gate keep their contents (the workspace is
 * unspecified).  Clear: the call computes as without a gate, adds 1 to [1] and, last thing, sets [0] iff target_kl > 0 and the float32 approx_kl it has just
 * written satisfies stats[3] > 1.5f * target_kl (a float32 product and compare, SB3's condition), so [0] is a function of the written stats[3] exactly.
 * usim_ppo_adam_gated with [0] set writes nothing (theta, m, v, *step_dev and stats[6] keep their contents); otherwise it produces usim_ppo_adam's bits and adds 1
 * to [2].  That is SB3's order: the minibatch whose KL trips the threshold is evaluated but not stepped, and no later one is.  The caller reads the gate when it
 * reads the statistics -- once per update; a gated grad + adam pair is still launches on `stream` and nothing else, capturable as one chain.  The gate words are
 * written by single threads of single-workgroup kernels with plain stores.  Further refusals (USIM_ERR_INVALID): a negative or non-finite clip_range_vf or
 * target_kl, clip_range_vf > 0 with a NULL old_value_dev, target_kl > 0 with a NULL gate_dev. ---- */
#define USIM_PPO_STATS 8
#define USIM_PPO_GATE_WORDS 4
#define USIM_PPO_WORKGROUPS 128                /* gradient workgroups per network = partial blocks of the workspace: a constant, not the device's CU count */
/* floats in the flat parameter / gradient block, in the field order of usim_policy_net:
 * pi_w1 pi_b1 pi_w2 pi_b2 act_w act_b vf_w1 vf_b1 vf_w2 vf_b2 val_w val_b log_std
 * = 76032 + 130 A + 129;  < 0: error code */
int     usim_ppo_params(int act_dim);
int64_t usim_ppo_work_floats(int act_dim);     /* workspace of usim_ppo_grad, zero-initialised by the caller once */

typedef struct usim_ppo_batch {
    const float *obs_dev, *act_dev, *old_logp_dev, *adv_dev, *ret_dev;  /* RolloutBuffer slices flattened to [rows][19], [rows][A], [rows] x 3 */
    const int32_t* index_dev;                  /* [batch] rows of this minibatch (repeats allowed); NULL: rows 0 .. batch-1 */
    int32_t rows, batch, act_dim, normalize_advantage;
    float clip_range, ent_coef, vf_coef, reserved_;
    const float* old_value_dev;                /* [rows] RolloutBuffer.values, flattened like ret_dev; required iff clip_range_vf > 0 */
    int32_t*     gate_dev;                     /* USIM_PPO_GATE_WORDS int32 words, or NULL: no gate */
    float        clip_range_vf;                /* 0: off (SB3's None) */
    float        target_kl;                    /* 0: off (SB3's None) */
} usim_ppo_batch;

int usim_ppo_grad(const usim_policy_net* net, const usim_ppo_batch* b, float* work_dev, float* grad_dev, float* stats_dev, void* stream);
int usim_ppo_adam(float* theta_dev, const float* grad_dev, float* m_dev, float* v_dev, int32_t* step_dev, int params,
                  float lr, float beta1, float beta2, float eps, float max_grad_norm, float* stats_dev, void* stream);
/* usim_ppo_adam behind the gate (gate_dev NULL: usim_ppo_adam itself) */
int usim_ppo_adam_gated(float* theta_dev, const float* grad_dev, float* m_dev, float* v_dev, int32_t* step_dev, int params,
                        float lr, float beta1, float beta2, float eps, float max_grad_norm, float* stats_dev, int32_t* gate_dev, void* stream);

/* ---- population learners: K PPO minibatch steps in one gradient call and one Adam call (population.py PopulationPPO(concurrent=True)).
 * The member is one more grid axis of the learner's kernels, as in usim_policy_step_multi, in the same K-major layout: theta_dev, grad_dev, m_dev, v_dev
 * [K][stride] (stride >= P = usim_ppo_params(A) and a multiple of 4; the first P words of row k are member k's flat block, words behind P are never touched),
 * step_dev [K], stats_dev [K][USIM_PPO_STATS], gate_dev [K][USIM_PPO_GATE_WORDS] or NULL.  Both calls are launches on `stream` and nothing else (no allocation, no
 * synchronisation, no host read of device memory): a pair is capturable as one chain.
 *
 * THE CONTRACT: member k's words of grad_dev, stats_dev, theta_dev, m_dev, v_dev, step_dev and gate_dev after the calls are, bit for bit, what usim_ppo_grad /
 * usim_ppo_adam_gated write for that member alone -- its row of theta, its rows of the data, its index list, its hyper-parameters, its gate.  A member reads and
 * writes its own rows only: a NaN in one member's weights or data does not reach another's; a member whose stop flag is set is skipped (its workgroups return on
 * entry) while the others go on.
 *
 * usim_ppo_batch_multi: the data pointers of usim_ppo_batch over members x rows rows, member k owning rows [k rows, (k + 1) rows); index_dev [K][index_stride]
 * int32, each relative to the member's own rows and clamped to them as usim_ppo_grad clamps (NULL: rows 0 .. batch - 1 of every member); rows, batch, act_dim and
 * normalize_advantage are one value for all members.  hyper_dev [K][USIM_PPO_HYPER_WORDS] float32 -- lr, clip_range, ent_coef, vf_coef, max_grad_norm,
 * clip_range_vf, target_kl, 0 -- is written by the host once per update, not per minibatch: a sweep over any of them is one launch.  The table lives on the
 * device and is not checked: a non-finite or negative entry is the caller's error, and what it does stays inside its member.  Value clipping is an instance of
 * the gradient kernel, so it is on for all members or for none: value_clip != 0 reads clip_range_vf (> 0) per member from the table and needs old_value_dev;
 * value_clip == 0 ignores that column.  target_kl (<= 0: off) takes effect only with a gate_dev.
 *
 * usim_ppo_grad_multi: prep, grid (65, K); grad, grid (nb, 2, K) with nb = min(USIM_PPO_WORKGROUPS, ceil(batch / 32)) -- the lone decomposition without the
 * workgroups that have no tile, which a lone call has write zeros; reduce and finish add blocks / rows 0 .. nb - 1 in order (adding the lone call's further +0
 * blocks to a sum that started from +0 changes no bit).  usim_ppo_adam_multi: count (one thread per member), adam, grid (ceil(params / 1024), K); lr and
 * max_grad_norm (<= 0: no clipping) come from the table; stats_dev may be NULL, otherwise slot 6 of each row receives the norm used.
 * work_dev: usim_ppo_work_floats_multi(A, K, batch) floats on the 16-byte grid, K regions of equal size (a multiple of 4 floats, so every region starts on the
 * 16-byte grid), each: nb partial blocks | the four packed layer-2 matrices | nb rows of 8 float64 loss sums | the two advantage words.  The regions' size
 * follows the call's own nb and the call rewrites every word it reads: a workspace sized for the largest batch serves every smaller one (an epoch's trailing
 * partial minibatch), and no clearing between calls is needed.
 * USIM_ERR_INVALID before anything is enqueued: what usim_ppo_grad / usim_ppo_adam refuse (NULL required pointers, act_dim outside 1 .. 8, batch < 1, rows < 1,
 * rows < batch without an index list, eps negative or non-finite, a beta outside [0, 1), params < 1), members outside 1 .. USIM_POLICY_MAX_MEMBERS, stride < P
 * (usim_ppo_adam_multi: < params) or not a multiple of 4, members x rows beyond INT_MAX, index_stride < batch with an index list, a NULL hyper_dev, value_clip
 * with a NULL old_value_dev, work_dev off the 16-byte grid. ---- */
#define USIM_PPO_HYPER_WORDS 8
typedef struct usim_ppo_batch_multi {
    const float *obs_dev, *act_dev, *old_logp_dev, *adv_dev, *ret_dev;  /* [K rows][19], [K rows][A], [K rows] x 3 */
    const float*   old_value_dev;              /* [K rows]; required iff value_clip */
    const int32_t* index_dev;                  /* [K][index_stride], or NULL */
    const float*   hyper_dev;                  /* [K][USIM_PPO_HYPER_WORDS] */
    int32_t*       gate_dev;                   /* [K][USIM_PPO_GATE_WORDS], or NULL: no gate */
    int32_t index_stride, rows, batch, act_dim, normalize_advantage, value_clip;
} usim_ppo_batch_multi;
int64_t usim_ppo_work_floats_multi(int act_dim, int members, int batch);      /* < 0: error code */
int usim_ppo_grad_multi(const float* theta_dev, int stride, int members, const usim_ppo_batch_multi* b,
                        float* work_dev, float* grad_dev, float* stats_dev, void* stream);
int usim_ppo_adam_multi(float* theta_dev, const float* grad_dev, float* m_dev, float* v_dev, int32_t* step_dev,
                        int stride, int members, int params, const float* hyper_dev, float beta1, float beta2, float eps,
                        float* stats_dev, int32_t* gate_dev, void* stream);

/* ---- behaviour cloning (imitation.py NativeBC, DAggerTrainer): the supervised minibatch loss of the `imitation` package's BC on the same
 * networks, as further instances of usim_ppo_grad's gradient kernel -- the same parameter order, the same workspace (usim_ppo_work_floats; one buffer may serve both
 * calls in turn), the same four launches on `stream` and nothing else, the same fixed order of every sum, the same clamping of an index outside [0, rows).  The
 * optimiser step is usim_ppo_adam.  Per row, with mean the action head's output and log-prob the DiagGaussianDistribution.log_prob of usim_ppo_grad:
 *   policy term  USIM_BC_NLL: -log-prob(act | mean(obs), log_std)     (its gradient reaches mean and log_std)
 *                USIM_BC_MSE: sum_a (mean_a - act_a)^2                (its gradient reaches mean only)
 *   value term   (value - V(obs))^2, only with value_dev             entropy  sum log_std + A / 2 (1 + log 2 pi)
 *   loss = mean(policy) + vf_coef mean(value) - ent_coef entropy
 * Without a value term (value_dev NULL, or vf_coef == 0) the value network is not evaluated: every value-network word of grad_dev is +0.0f, value_loss is 0.
 * stats_dev[USIM_PPO_STATS]: policy_loss, value_loss, entropy_loss (= -entropy), action_mse (mean over rows of sum_a (mean_a - act_a)^2, in both forms), the mean
 * log-prob (in both forms), loss, the gradient's 2-norm, 0.
 * USIM_ERR_INVALID before anything is enqueued: a NULL net (or a NULL parameter of it other than w2_packed), b, obs_dev, act_dev, work_dev, grad_dev or stats_dev,
 * act_dim outside 1 .. 8, batch < 1, rows < 1, rows < batch without an index list, loss outside the two, a non-finite coefficient, work_dev off the 16-byte grid. ---- */
#define USIM_BC_NLL 0
#define USIM_BC_MSE 1
typedef struct usim_bc_batch {
    const float *obs_dev, *act_dev;            /* [rows][19] normalised observations, [rows][A] expert actions */
    const float *value_dev;                    /* [rows] value targets, or NULL: no value term */
    const int32_t* index_dev;                  /* as usim_ppo_batch */
    int32_t rows, batch, act_dim, loss;        /* loss: USIM_BC_NLL | USIM_BC_MSE */
    float ent_coef, vf_coef, reserved_[2];
} usim_bc_batch;
int usim_bc_grad(const usim_policy_net* net, const usim_bc_batch* b, float* work_dev, float* grad_dev, float* stats_dev, void* stream);

const char* usim_strerror(int status);
const char* usim_last_hip_error(const usim_handle* h);
const char* usim_version(void);

#ifdef __cplusplus
}
#endif
#endif /* USIM_H */
