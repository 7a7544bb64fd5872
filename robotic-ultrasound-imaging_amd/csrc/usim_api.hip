// usim_api.hip -- host side of the C ABI declared in include/usim.h (libusim.so).
//
// Owns the SoA state block in HBM and enqueues the kernels of usim_kernels.hip (and of usim_full.h, usim_step16.h, which it includes) on the caller's HIP stream.
// What usim_create decides before it touches the device -- the model constants in double precision, the DevCfg translation, the mapping -- is usim_setup.h.
// The layout of the state block is stated once (StateLayout, usim_checkpoint.h); the checkpoint conversions over host copies of the block are that header's too.
// The entry points that take no handle are translation units of their own: usim_policy.hip (usim_policy_*), usim_pack.hip, usim_score.hip, usim_plan.hip (usim_plan_*).
// No torch types, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <new>

#include "../../include/usim.h"
#include "usim_device.h"
#include "usim_robot.h"
#include "usim_setup.h"          // what usim_create decides before it touches the device: Mapping, check_config, build_model, translate_config
#include "usim_checkpoint.h"     // the layout of the state block (StateLayout) and the checkpoint conversions over host copies of it
#include "usim_kernels.hip"      // the step, reset, bank and snapshot kernels share this translation unit with their host launcher (no relocatable device code)
#include "usim_snapshot.h"       // usim_save_envs / usim_load_envs (behind the step kernels)


using namespace usim;

// The launch table: which kernel a handle's mapping (usim_setup.h) runs for each kind of launch, cold and -- soft torso with usim_config.warm_start -- warm (W).
//   STEP   one physics step, one control step                        MULTI  several physics steps: io.nsub > 1 control steps or C.substeps > 1
//   ACTS   MULTI that plays a caller's action block (usim_rollout_actions): the kernel moves io.act on between the control steps
//   RESET  reset / refill launches (warm: they empty the warm rows of the environments they reset)
//   mapping     STEP                                MULTI                              ACTS                               RESET
//   FULL        usim_step_kernel<2, 64, 0>          = STEP (one step per launch, rollout_common)                          usim_step_kernel<2, 64, 1>
//   RIGID16     usim_step16_kernel<0, 2, 0, false>  usim_step16_kernel<0, 2, 0, true>  usim_step16_acts_kernel<0, 2>      usim_step16_kernel<0, 2, 1, false>       (W: no effect)
//   SOFT16_W1   ..16_kernel<1, 1, 0, false, W>      ..16_kernel<1, 1, 0, true, W>      ..16_acts_kernel<1, 1, W>          usim_step16_kernel<1, 2, 1, false, W>: SOFT16_W2's
//   SOFT16_W2   ..16_kernel<1, 2, 0, false, W>      ..16_kernel<1, 2, 0, true, W>      ..16_acts_kernel<1, 2, W>          for every soft mapping (not register-critical)
//   SPLIT16     usim_step32_kernel<false, 16, W>    usim_step32_kernel<true, 16, W>    usim_step32_acts_kernel<16, W>     same
//   SPLIT8      usim_step32_kernel<false, 8, W>     usim_step32_kernel<true, 8, W>     usim_step32_acts_kernel<8, W>      same
enum class Launch : int { STEP, MULTI, ACTS, RESET };
constexpr Launch launch_kind(bool reset, int nsub, int substeps, const float* act) {
    return reset ? Launch::RESET : nsub > 1 ? (act ? Launch::ACTS : Launch::MULTI) : substeps > 1 ? Launch::MULTI : Launch::STEP;
}

// one kernel with its launch geometry (environments and threads per workgroup, dynamic LDS words; the 16-lane kernels: + the arm table behind everything else);
// model and configuration by value, or through pointers for the split kernels
using StepKernel = void (*)(const DevModel, const DevCfg, float*, int, int, const DevIO, int, long long);
using SplitKernel = void (*)(const DevModel*, const DevCfg*, float*, int, int, const DevIO, int, long long);
struct Kernel { StepKernel step; SplitKernel split; int epb, nt, lds_words; };
struct Row { Mapping map; bool warm; Launch launch; Kernel k; };

// The rows of the three kernel families: key, kernel and geometry all follow from the template arguments.
template <Launch L> constexpr Row full_row() {
    static_assert(L == Launch::STEP || L == Launch::RESET, "the full torso runs one step per launch");
    StepKernel f = nullptr;
    if constexpr (L == Launch::STEP) f = usim_step_kernel<2, 64, 0>;
    else f = usim_step_kernel<2, 64, 1>;
    return {Mapping::FULL, false, L, {f, nullptr, FULL_EPB, FULL_NT, FULL_LDS_WORDS}};
}
template <int TORSO, int OCC, bool WARM, Launch L> constexpr Row wave_row() {                   // single-wave 16-lane kernels: 16 environments, four waves
    static_assert((TORSO == 1 || (TORSO == 0 && OCC == 2 && !WARM)) && (L != Launch::RESET || OCC == 2), "RIGID16, SOFT16_W1, SOFT16_W2; resets with the budget of two waves per SIMD");
    StepKernel f = nullptr;
    if constexpr (L == Launch::STEP) f = usim_step16_kernel<TORSO, OCC, 0, false, WARM>;
    else if constexpr (L == Launch::MULTI) f = usim_step16_kernel<TORSO, OCC, 0, true, WARM>;
    else if constexpr (L == Launch::ACTS) f = usim_step16_acts_kernel<TORSO, OCC, WARM>;
    else f = usim_step16_kernel<TORSO, OCC, 1, false, WARM>;
    return {TORSO == 0 ? Mapping::RIGID16 : OCC == 1 ? Mapping::SOFT16_W1 : Mapping::SOFT16_W2, WARM, L, {f, nullptr, 16, 256, arm_lds_base<TORSO, 0, 16>() + ARM_LDS_WORDS}};
}
template <int G, bool WARM, Launch L> constexpr Row split_row() {                               // split kernels: a wave pair per 64 / G environments, SPLIT_WPR pairs
    static_assert((G == 16 || G == 8) && L != Launch::RESET, "SPLIT16, SPLIT8; they reset with SOFT16_W2's kernel");
    SplitKernel f = nullptr;
    if constexpr (L == Launch::STEP) f = usim_step32_kernel<false, G, WARM>;
    else if constexpr (L == Launch::MULTI) f = usim_step32_kernel<true, G, WARM>;
    else f = usim_step32_acts_kernel<G, WARM>;
    return {G == 16 ? Mapping::SPLIT16 : Mapping::SPLIT8, WARM, L, {nullptr, f, (64 / G) * SPLIT_WPR, 128 * SPLIT_WPR, arm_lds_base<1, 1, G, L != Launch::STEP>() + ARM_LDS_WORDS}};
}

// Every step kernel of the library, once.  The compiler emits the kernels in the order in which they are named here: the order is the one the code object has always
// had (action blocks, warm, cold), so that a change to this file alone leaves the code object as it was.  New rows go behind their group.
constexpr Row kRows[] = {
    wave_row<0, 2, false, Launch::ACTS>(),
    wave_row<1, 1, true, Launch::ACTS>(), wave_row<1, 1, false, Launch::ACTS>(), wave_row<1, 2, true, Launch::ACTS>(), wave_row<1, 2, false, Launch::ACTS>(),
    split_row<16, true, Launch::ACTS>(), split_row<16, false, Launch::ACTS>(), split_row<8, true, Launch::ACTS>(), split_row<8, false, Launch::ACTS>(),

    wave_row<1, 2, true, Launch::RESET>(),
    wave_row<1, 1, true, Launch::MULTI>(), wave_row<1, 1, true, Launch::STEP>(), wave_row<1, 2, true, Launch::MULTI>(), wave_row<1, 2, true, Launch::STEP>(),
    split_row<16, true, Launch::MULTI>(), split_row<16, true, Launch::STEP>(), split_row<8, true, Launch::MULTI>(), split_row<8, true, Launch::STEP>(),

    full_row<Launch::RESET>(), full_row<Launch::STEP>(),
    wave_row<0, 2, false, Launch::MULTI>(), wave_row<0, 2, false, Launch::STEP>(), wave_row<0, 2, false, Launch::RESET>(),
    wave_row<1, 1, false, Launch::MULTI>(), wave_row<1, 1, false, Launch::STEP>(), wave_row<1, 2, false, Launch::MULTI>(), wave_row<1, 2, false, Launch::STEP>(),
    wave_row<1, 2, false, Launch::RESET>(),
    split_row<16, false, Launch::MULTI>(), split_row<16, false, Launch::STEP>(), split_row<8, false, Launch::MULTI>(), split_row<8, false, Launch::STEP>(),
};

// the row of (mapping, warm, launch): its index in kRows, -1 unless exactly one row answers
constexpr int find_row(Mapping m, bool warm, Launch l) {
    if (m == Mapping::FULL && l != Launch::RESET) l = Launch::STEP;        // one step per launch (rollout_common)
    if (soft_torso(m) && l == Launch::RESET) m = Mapping::SOFT16_W2;       // the soft mappings share its reset kernel
    warm = warm && soft_torso(m);                                         // rigid and full torso: no effect
    int at = -1, hits = 0;
    for (int i = 0; i < (int)(sizeof kRows / sizeof kRows[0]); ++i)
        if (kRows[i].map == m && kRows[i].warm == warm && kRows[i].launch == l) { at = i; ++hits; }
    return hits == 1 ? at : -1;
}
constexpr bool table_sound() {
    for (const Row& r : kRows) if (r.k.lds_words * (int)sizeof(float) > 160 * 1024 || r.k.nt > 1024 || r.k.epb < 1 || (r.k.step == nullptr) == (r.k.split == nullptr)) return false;
    for (int m = 0; m <= (int)Mapping::SPLIT8; ++m) for (int w = 0; w < 2; ++w) for (int l = 0; l <= (int)Launch::RESET; ++l) if (find_row((Mapping)m, w != 0, (Launch)l) < 0) return false;
    return true;
}
static_assert(table_sound(), "every row within 160 KB of LDS and 1024 threads; every (mapping, warm, launch) has exactly one row");
static const Kernel& kernel_of(Mapping m, bool warm, Launch l) { return kRows[find_row(m, warm, l)].k; }

struct usim_handle {
    usim_config cfg;
    Mapping map = Mapping::RIGID16;   // resolved by usim_create (resolve_mapping)
    StateLayout L{};                  // the state block: environments, regions, size (usim_checkpoint.h)
    int device = 0, adim = 6;
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

// per-handle copy of the table block (synchronous: complete before usim_create returns, so no stream of the caller can race with it)
static int upload_tables(usim_handle* h, const std::vector<float>& tb) {
    HIPCHK(h, hipMalloc(&h->d_tables, tb.size() * sizeof(float)));
    HIPCHK(h, hipMemcpy(h->d_tables, tb.data(), tb.size() * sizeof(float), hipMemcpyHostToDevice));
    h->M.tables = h->d_tables;
    return USIM_OK;
}

// dynamic LDS limit of every kernel the handle can launch: those of its mapping, for a soft-torso handle those of every soft-torso mapping (usim_set_mapping)
static int set_lds_limits(usim_handle* h) {
    for (int m = 0; m <= (int)Mapping::SPLIT8; ++m)
        if ((Mapping)m == h->map || (soft_torso((Mapping)m) && soft_torso(h->map)))
            for (const Launch l : {Launch::STEP, Launch::MULTI, Launch::ACTS, Launch::RESET}) {
                const Kernel& k = kernel_of((Mapping)m, h->warm, l);
                HIPCHK(h, hipFuncSetAttribute(k.step ? (const void*)k.step : (const void*)k.split, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_words * (int)sizeof(float)));
            }
    return USIM_OK;
}

// every environment's warm rows to "nothing kept" (synchronous)
static int warm_rows_reset(usim_handle* h) {
    std::vector<float> w((size_t)h->L.warm_words * h->L.npad);
    empty_warm(h->L.npad, w.data());
    HIPCHK(h, hipMemcpy(h->state + h->L.warm(0), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    return USIM_OK;
}

static int launch(usim_handle* h, DevIO io, Launch l, int flags, long long rstep, hipStream_t s) {
    io.bank_row0 = h->L.bank_row0;
    const Kernel& k = kernel_of(h->map, h->warm, l);
    const dim3 grid((h->L.n + k.epb - 1) / k.epb), block(k.nt);
    const size_t lds = (size_t)k.lds_words * sizeof(float);
    if (k.step) hipLaunchKernelGGL(k.step, grid, block, lds, s, h->M, h->C, h->state, h->L.n, h->L.npad, io, flags, rstep);
    else hipLaunchKernelGGL(k.split, grid, block, lds, s, h->d_M, h->d_C, h->state, h->L.n, h->L.npad, io, flags, rstep);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->hip_err = std::string("usim_step_kernel launch: ") + hipGetErrorString(e); return USIM_ERR_HIP; }
    return USIM_OK;
}
// the launch that a step's I/O block asks for
static Launch step_launch(const usim_handle* h, const DevIO& io) { return launch_kind(false, io.nsub, h->C.substeps, io.act); }

extern "C" {

int usim_default_config(usim_config* c) {
    if (!c || c->struct_size != (int32_t)sizeof(usim_config)) return USIM_ERR_INVALID;   // nothing is written to a struct of another layout
    default_config(c);
    return USIM_OK;
}

// check, build, translate (usim_setup.h); allocate and upload; resolve the mapping
int usim_create(const usim_config* cfg, int n_envs, int device, usim_handle** out) {
    if (!cfg || !out || n_envs <= 0 || !check_config(*cfg)) return USIM_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return USIM_ERR_NO_DEVICE;
    usim_handle* h = new (std::nothrow) usim_handle();
    if (!h) return USIM_ERR_ALLOC;
    *out = h;                       // returned even on failure so that usim_last_hip_error can be read; caller destroys
    h->cfg = *cfg; h->device = device;
    DeviceGuard guard(device);
    // warm start of the top-face contact solve (the rigid torso has no contact solve, the full torso is always warm: accepted, no effect).  USIM_WARM_START = 0 / 1
    // replaces the field, so that a fixed command line (bench.py) can time both; the handle's recorded configuration follows it
    if (const char* ws = std::getenv("USIM_WARM_START")) { if ((ws[0] == '0' || ws[0] == '1') && ws[1] == 0) h->cfg.warm_start = ws[0] - '0'; }
    h->warm = h->cfg.warm_start != 0 && cfg->torso == USIM_TORSO_TOP;
    ModelTables model;
    int rc = build_model(*cfg, &model);
    h->L = state_layout(cfg->torso, model.n_el, n_envs, h->warm);             // the one description of the state block: allocation, checkpoints, snapshots
    if (rc != USIM_OK) return rc;
    h->M = model.M;
    h->C = translate_config(*cfg);
    h->adim = h->C.adim;
    if (const char* spl = std::getenv("USIM_STEPS_PER_LAUNCH")) { const int v = std::atoi(spl); if (v >= 1 && v <= MAX_STEPS_PER_LAUNCH) h->steps_per_launch = v; }
    rc = upload_tables(h, model.words);
    if (rc != USIM_OK) return rc;
    {
        // device copy of the model and the configuration (both final here; upload_tables has set M.tables)
        const size_t offC = (sizeof(DevModel) + 255) / 256 * 256;
        HIPCHK(h, hipMalloc(&h->d_consts, offC + sizeof(DevCfg)));
        HIPCHK(h, hipMemcpy(h->d_consts, &h->M, sizeof(DevModel), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(static_cast<char*>(h->d_consts) + offC, &h->C, sizeof(DevCfg), hipMemcpyHostToDevice));
        h->d_M = static_cast<const DevModel*>(h->d_consts); h->d_C = reinterpret_cast<const DevCfg*>(static_cast<const char*>(h->d_consts) + offC);
    }
    HIPCHK(h, hipMalloc(&h->state, h->L.words * sizeof(float)));                // live rows, reset bank, warm rows (StateLayout)
    HIPCHK(h, hipMemset(h->state, 0, h->L.words * sizeof(float)));
    if (h->warm) { int rc2 = warm_rows_reset(h); if (rc2) return rc2; }
    HIPCHK(h, hipMalloc(&h->d_items, 2 * (size_t)h->L.n * BANK_DEPTH * sizeof(int2)));
    HIPCHK(h, hipMalloc(&h->d_count, 2 * sizeof(int)));
    HIPCHK(h, hipMemset(h->d_count, 0, 2 * sizeof(int)));
    HIPCHK(h, hipEventCreate(&h->ev0));
    HIPCHK(h, hipEventCreate(&h->ev1));
    for (int i = 0; i < usim_handle::RF_RING; ++i) { HIPCHK(h, hipEventCreate(&h->rf0[i])); HIPCHK(h, hipEventCreate(&h->rf1[i])); }
    if (!resolve_mapping(cfg->torso, cfg->lanes_per_env, cfg->waves_per_simd, n_envs, &h->map)) return USIM_ERR_INVALID;
    // the full torso runs one mapping: a wave per environment, the Panda's constants, one physics step per control step, one step per launch
    if (h->map == Mapping::FULL && (cfg->robot != USIM_ROBOT_PANDA || h->C.substeps > 1)) { h->hip_err = "torso = USIM_TORSO_FULL: Panda, substeps = 1"; return USIM_ERR_UNSUPPORTED; }
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
    return resolve_mapping(h->cfg.torso, lanes_per_env, waves_per_simd, h->L.n, &h->map) ? USIM_OK : USIM_ERR_INVALID;
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

int usim_num_envs(const usim_handle* h) { return h ? h->L.n : USIM_ERR_INVALID; }
int usim_action_dim(const usim_handle* h) { return h ? h->adim : USIM_ERR_INVALID; }
int usim_num_elements(const usim_handle* h) { return h ? h->L.n_el : USIM_ERR_INVALID; }
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
    if (s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return launch(h, b, Launch::RESET, 0, 0, s);
    const int slot = h->rf_next;
    h->rf_next = (slot + 1) % usim_handle::RF_RING;
    refill_collect(h, slot);                          // (a pair that is reused was recorded RF_RING refills = 512 steps ago: long finished)
    const bool timed = h->rf0[slot] && h->rf1[slot] && hipEventRecord(h->rf0[slot], s) == hipSuccess;
    const int rc = launch(h, b, Launch::RESET, 0, 0, s);
    if (timed && rc == USIM_OK && hipEventRecord(h->rf1[slot], s) == hipSuccess) h->rf_live[slot] = true;
    return rc;
}

// order episodes +1..+BANK_DEPTH for the selected environments and compute them
static int bank_fill(usim_handle* h, const uint8_t* mask_dev, hipStream_t s) {
    const int total = h->L.n * BANK_DEPTH;
    hipLaunchKernelGGL(usim_bank_items_kernel, dim3((total + 255) / 256), dim3(256), 0, s, h->state, h->L.n, mask_dev, h->d_items, h->d_count);
    HIPCHK(h, hipGetLastError());
    return bank_refill(h, s);
}

// direct reset of the selected environments followed by the fill of their bank rings, all on `stream`
static int reset_common(usim_handle* h, const uint8_t* mask_dev, const float* params_dev, float* obs_dev, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    DevIO io{}; io.mask = mask_dev; io.obs = obs_dev; io.reset_params = params_dev; io.refill = 0;
    int rc = launch(h, io, Launch::RESET, 0, 0, s);
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
    if (!(flags & LF_AUTO_RESET)) return launch(h, io, step_launch(h, io), flags, rstep, s);
    io.items = h->d_items; io.count = h->d_count;
    int rc = launch(h, io, step_launch(h, io), flags, rstep, s);
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
    hipLaunchKernelGGL(usim_random_actions_kernel, dim3((h->L.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->C, h->L.n, (long long)step, act_dev);
    HIPCHK(h, hipGetLastError());
    return USIM_OK;
}

// nsteps consecutive auto-reset steps in multi-step launches (usim_rollout_random, usim_rollout_actions; `flags` and io.act are all that differs between them).
// The 16-lane kernels run up to h->steps_per_launch consecutive steps per launch (usim_step16.h step16_body); a launch never crosses the refill period of the
// reset bank (an environment consumes at most one ring slot per step).  io.act, where there is one, is an action block [nsteps][n][A]: inside a launch the kernel
// moves it on from control step to control step (Launch::ACTS), between launches this loop does -- whether or not the outputs are blocks (block_advance).
static int rollout_common(usim_handle* h, DevIO io, int flags, long long first_step, int nsteps, int block_advance, void* stream) {
    const int kmax = multi_step(h->map) ? h->steps_per_launch : 1;
    for (int k = 0; k < nsteps;) {
        const int kk = launch_steps(nsteps - k, kmax, BANK_DEPTH - (int)h->steps_since_refill);
        io.nsub = kk; io.block = block_advance ? 1 : 0;
        h->steps_since_refill += kk - 1;                      // (step_common counts the launch as one step)
        const int rc = step_common(h, io, flags, first_step + k, stream);
        if (rc) return rc;
        k += kk;
        if (block_advance) advance_rollout_block(io, (size_t)h->L.n * kk, h->adim);
        if (io.act) io.act += (size_t)h->L.n * kk * h->adim;
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

// ---- checkpoints: synchronise, copy the block down, convert on the host (usim_checkpoint.h), copy it up.  The setters are read-modify-writes: words that a conversion
// does not own (the padding environments, lattice words between the regions) keep what they hold.
static int download(usim_handle* h, std::vector<float>& buf, size_t first, size_t words) {
    buf.resize(words);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(buf.data(), h->state + first, words * sizeof(float), hipMemcpyDeviceToHost));
    return USIM_OK;
}
static int upload(usim_handle* h, const std::vector<float>& buf, size_t first) {
    HIPCHK(h, hipMemcpy(h->state + first, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
    return USIM_OK;
}

int usim_get_body_state(usim_handle* h, double* body) {
    if (!h || !body || h->cfg.torso != USIM_TORSO_FULL) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    std::vector<float> lat;
    if (int rc = download(h, lat, h->L.lattice(0), (size_t)h->L.lat_words * h->L.npad)) return rc;
    body_words<TO_HOST>(h->L, h->M.base, lat.data(), body);
    return USIM_OK;
}
int usim_set_body_state(usim_handle* h, const double* body) {
    if (!h || !body || h->cfg.torso != USIM_TORSO_FULL) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    std::vector<float> lat;
    if (int rc = download(h, lat, h->L.lattice(0), (size_t)h->L.lat_words * h->L.npad)) return rc;
    body_words<TO_DEVICE>(h->L, h->M.base, lat.data(), body);
    return upload(h, lat, h->L.lattice(0));
}

int usim_get_warm_start(usim_handle* h, float* w) {
    if (!h || !w || !h->warm) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    std::vector<float> rows;
    if (int rc = download(h, rows, h->L.warm(0), (size_t)h->L.warm_words * h->L.n)) return rc;
    warm_words<TO_HOST>(h->L.n, rows.data(), w);
    return USIM_OK;
}
int usim_set_warm_start(usim_handle* h, const float* w) {
    if (!h || !w || !h->warm) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<float> rows((size_t)h->L.warm_words * h->L.n);
    warm_words<TO_DEVICE>(h->L.n, rows.data(), w);
    return upload(h, rows, h->L.warm(0));
}

int usim_get_state(usim_handle* h, float* scalars, float* lattice) {
    if (!h || !scalars) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    std::vector<float> buf;
    if (int rc = download(h, buf, 0, h->L.live_words())) return rc;
    state_words<TO_HOST>(h->L, buf.data(), scalars, lattice);
    return USIM_OK;
}

int usim_set_state(usim_handle* h, const float* scalars, const float* lattice) {
    if (!h || !scalars) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    std::vector<float> buf;
    if (int rc = download(h, buf, 0, h->L.live_words())) return rc;
    state_words<TO_DEVICE>(h->L, buf.data(), scalars, lattice);
    if (int rc = upload(h, buf, 0)) return rc;
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
static SnapLayout snap_layout(const usim_handle* h) { return {h->L.lat_words, h->L.warm_words, h->L.bank_row0}; }
static unsigned snap_grid(int rows, int lanes) { return (unsigned)(((size_t)rows * lanes + SNAP_WG - 1) / SNAP_WG); }

int usim_snapshot_words(const usim_handle* h) { return h ? h->L.snapshot_words() : USIM_ERR_INVALID; }      // (= snap_row_words(snap_layout(h)), what the kernels move)

int usim_save_envs(usim_handle* h, const int32_t* env_index_dev, int m, float* snap_dev, void* stream) {
    if (!h || !snap_dev || m <= 0 || (reinterpret_cast<uintptr_t>(snap_dev) & 15) || (!env_index_dev && m > h->L.n)) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    const SnapLayout L = snap_layout(h);
    hipStream_t s = (hipStream_t)stream;
    if (h->map == Mapping::FULL) hipLaunchKernelGGL(usim_save_envs_kernel<64>, dim3(snap_grid(m, 64)), dim3(SNAP_WG), 0, s, h->state, h->L.n, h->L.npad, L, env_index_dev, m, snap_dev);
    else hipLaunchKernelGGL(usim_save_envs_kernel<16>, dim3(snap_grid(m, 16)), dim3(SNAP_WG), 0, s, h->state, h->L.n, h->L.npad, L, env_index_dev, m, snap_dev);
    HIPCHK(h, hipGetLastError());
    return USIM_OK;
}

int usim_load_envs(usim_handle* h, const float* snap_dev, int m, const int32_t* row_of_env_dev, void* stream) {
    if (!h || !snap_dev || !row_of_env_dev || m <= 0 || (reinterpret_cast<uintptr_t>(snap_dev) & 15)) return USIM_ERR_INVALID;
    DeviceGuard guard(h->device);
    const SnapLayout L = snap_layout(h);
    hipStream_t s = (hipStream_t)stream;
    if (h->map == Mapping::FULL) hipLaunchKernelGGL(usim_load_envs_kernel<64>, dim3(snap_grid(h->L.n, 64)), dim3(SNAP_WG), 0, s, h->state, h->L.n, h->L.npad, L, snap_dev, m, row_of_env_dev);
    else hipLaunchKernelGGL(usim_load_envs_kernel<16>, dim3(snap_grid(h->L.n, 16)), dim3(SNAP_WG), 0, s, h->state, h->L.n, h->L.npad, L, snap_dev, m, row_of_env_dev);
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
    io.dbg = d;
    // USIM_PROFILE_NSUB = k: the stamps of the LAST of k consecutive steps of one launch (multi-step kernels; never across a refill period)
    if (const char* ns = std::getenv("USIM_PROFILE_NSUB")) { const int v = std::atoi(ns); if (v > 1 && launch_steps(v, MAX_STEPS_PER_LAUNCH, BANK_DEPTH - (int)h->steps_since_refill) == v) { io.nsub = v; h->steps_since_refill += v - 1; } }
    rc = step_common(h, io, LF_AUTO_RESET | LF_RANDOM_ACT, (long long)step, nullptr);
    HIPCHK(h, hipDeviceSynchronize());
    unsigned long long host[64];
    HIPCHK(h, hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost));
    HIPCHK(h, hipFree(d));
    for (int i = 0; i < (max_ticks < 64 ? max_ticks : 64); ++i) ticks[i] = host[i];      // 0-16: phases of the single-wave kernels; 20-29 / 30-39: arm / lattice side of the split kernel; 54-61: 1 + broad-phase queue length of the environments of its first lattice wave
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
