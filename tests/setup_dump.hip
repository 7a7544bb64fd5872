// setup_dump -- prints what usim_create decides before it touches the device (csrc/usim_setup.h), for tests/test_host_setup.py.  A host program: no HIP call, no GPU.
//   setup_dump TORSO SHAPE ROBOT [field=value ...] [n_envs=N] [tables=PATH]
// TORSO, SHAPE, ROBOT and the field=value overrides (fields of usim_config, by name) go on top of usim_default_config's values.  Output, one "name value ..." line each:
// the configuration (cfg.*), check (check_config), build (build_model's status), DevCfg (C.*), DevModel (M.*), n_el, words, mapping (resolve_mapping for n_envs, default
// 4096; "refused").  tables=PATH: the table words as raw float32.  A refused configuration ends the output after its check line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/usim.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_device.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_robot.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_setup.h"

using namespace usim;

#define CFG_INT(X) X(struct_size) X(mode) X(torso) X(horizon) X(early_termination) X(deterministic_trajectory) X(torso_solref_randomization) X(initial_probe_pos_randomization) \
    X(friction_randomization) X(torso_drop) X(pgs_iters) X(ik_iters) X(env_offset) X(lanes_per_env) X(torso_shape) X(waves_per_simd) X(robot) X(substeps) X(probe_geoms) X(pair_model) X(warm_start)
#define CFG_DOUBLE(X) X(control_dt) X(kp_fixed) X(damping_ratio) X(kp_min) X(kp_max) X(out_max_pos) X(out_max_ori) X(stiffness) X(damping) X(elem_friction) X(probe_friction) \
    X(probe_radius) X(probe_halflen) X(probe_radius2) X(probe_height) X(probe_friction2) X(probe_halfwidth) X(probe_tip) X(armature_scale) X(joint_frictionloss)
#define C_INT(X) X(mode) X(horizon) X(early_term) X(det_traj) X(rand_solref) X(rand_pos) X(rand_fric) X(torso_drop) X(pgs_iters) X(ik_iters) X(env_offset) X(adim) X(probe_geoms) X(pair) X(substeps)
#define C_FLOAT(X) X(dt) X(kp_fixed) X(damping_ratio) X(kp_min) X(kp_max) X(out_pos) X(out_ori) X(stiffness) X(damping) X(elem_fric) X(probe_fric) X(probe_r) X(probe_hl) X(probe_hw) \
    X(probe_tip) X(probe_cull2) X(probe_deep0) X(probe_inv_band) X(probe_r2) X(probe_h) X(probe_ca) X(probe_cb) X(probe_cah) X(top_off) X(y_range) X(drop) X(probe_fric2) X(rn_scale) \
    X(dt_ctrl) X(frictionloss)

static bool set_field(usim_config& c, const std::string& name, const char* value) {
#define X(f) if (name == #f) { c.f = (int32_t)std::strtol(value, nullptr, 0); return true; }
    CFG_INT(X)
#undef X
#define X(f) if (name == #f) { c.f = std::strtod(value, nullptr); return true; }
    CFG_DOUBLE(X)
#undef X
    if (name == "seed") { c.seed = std::strtoull(value, nullptr, 0); return true; }
    return false;
}

template <size_t N> static void print_floats(const char* name, const float (&v)[N]) {
    std::printf("%s", name);
    for (size_t i = 0; i < N; ++i) std::printf(" %.9g", (double)v[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: setup_dump TORSO SHAPE ROBOT [field=value ...] [n_envs=N] [tables=PATH]\n"); return 2; }
    usim_config cfg;
    default_config(&cfg);
    cfg.torso = std::atoi(argv[1]); cfg.torso_shape = std::atoi(argv[2]); cfg.robot = std::atoi(argv[3]);
    int n_envs = 4096;
    std::string tables;
    for (int i = 4; i < argc; ++i) {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) { std::fprintf(stderr, "setup_dump: %s is not name=value\n", argv[i]); return 2; }
        const std::string name(argv[i], (size_t)(eq - argv[i]));
        if (name == "n_envs") n_envs = std::atoi(eq + 1);
        else if (name == "tables") tables = eq + 1;
        else if (!set_field(cfg, name, eq + 1)) { std::fprintf(stderr, "setup_dump: usim_config has no field %s\n", name.c_str()); return 2; }
    }
#define X(f) std::printf("cfg." #f " %d\n", (int)cfg.f);
    CFG_INT(X)
#undef X
#define X(f) std::printf("cfg." #f " %.17g\n", cfg.f);
    CFG_DOUBLE(X)
#undef X
    std::printf("cfg.seed %llu\n", (unsigned long long)cfg.seed);
    const bool ok = check_config(cfg);
    std::printf("check %d\n", ok ? 1 : 0);
    if (!ok) return 0;

    ModelTables model;
    const int rc = build_model(cfg, &model);
    std::printf("build %d\n", rc);
    if (rc != USIM_OK) return 0;
    const DevCfg C = translate_config(cfg);
#define X(f) std::printf("C." #f " %d\n", C.f);
    C_INT(X)
#undef X
    std::printf("C.key0 %u\nC.key1 %u\n", C.key0, C.key1);
#define X(f) std::printf("C." #f " %.9g\n", (double)C.f);
    C_FLOAT(X)
#undef X
    const DevModel& M = model.M;
    std::printf("M.m7 %.9g\nM.geps %.9g\nM.invw %.9g\nM.wfix %.9g\nM.wten %.9g\n", (double)M.m7, (double)M.geps, (double)M.invw, (double)M.wfix, (double)M.wten);
    print_floats("M.c7", M.c7); print_floats("M.I7", M.I7); print_floats("M.site7", M.site7); print_floats("M.hand7", M.hand7); print_floats("M.pcom7", M.pcom7);
    print_floats("M.pI7", M.pI7); print_floats("M.torso", M.torso); print_floats("M.grot", M.grot); print_floats("M.gquat", M.gquat); print_floats("M.ghat", M.ghat);
    print_floats("M.base", M.base); print_floats("M.ikb", M.ikb); print_floats("M.armature", M.armature);
    std::printf("n_el %d\nwords %zu\n", model.n_el, model.words.size());
    Mapping map;
    static const char* const kNames[] = {"FULL", "RIGID16", "SOFT16_W1", "SOFT16_W2", "SPLIT16", "SPLIT8"};
    std::printf("mapping %s\n", resolve_mapping(cfg.torso, cfg.lanes_per_env, cfg.waves_per_simd, n_envs, &map) ? kNames[(int)map] : "refused");
    if (!tables.empty()) {
        std::FILE* f = std::fopen(tables.c_str(), "wb");
        if (!f || std::fwrite(model.words.data(), sizeof(float), model.words.size(), f) != model.words.size() || std::fclose(f) != 0) { std::perror("setup_dump: tables"); return 1; }
    }
    return 0;
}
