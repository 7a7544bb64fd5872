// cull_dump -- prints the constant of the capsule-form broad phase (DevCfg::probe_cull2c, csrc/usim_setup.h translate_config) for tests/test_cull_bound.py; every other
// constant that test uses comes from tests/setup_dump.hip, which lists the DevCfg fields it prints by name.  A host program: no HIP call, no GPU.
//   cull_dump [probe_field=value ...]      (the double fields of usim_config whose name begins with probe_, on top of usim_default_config's values)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/usim.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_device.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_robot.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_setup.h"

using namespace usim;

#define PROBE_DOUBLE(X) X(probe_radius) X(probe_halflen) X(probe_radius2) X(probe_height) X(probe_halfwidth) X(probe_tip)

int main(int argc, char** argv) {
    usim_config cfg;
    default_config(&cfg);
    for (int i = 1; i < argc; ++i) {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) { std::fprintf(stderr, "cull_dump: %s is not name=value\n", argv[i]); return 2; }
        const std::string name(argv[i], (size_t)(eq - argv[i]));
        bool known = false;
#define X(f) if (name == #f) { cfg.f = std::strtod(eq + 1, nullptr); known = true; }
        PROBE_DOUBLE(X)
#undef X
        if (!known) { std::fprintf(stderr, "cull_dump: no probe field %s\n", name.c_str()); return 2; }
    }
    if (!check_config(cfg)) { std::printf("check 0\n"); return 0; }
    const DevCfg C = translate_config(cfg);
    std::printf("check 1\nC.probe_cull2c %.9g\n", (double)C.probe_cull2c);
    return 0;
}
