// capi.hip — the C ABI of include/rpt.h: contexts (one device, the devices of a node in one process, or one rank of a
// multi-process job), scene upload, launches, the RCCL gather.  Host code only; the kernels and their launch functions
// are in the k_*.hip translation units (launch.h); every environment variable the library reads is in knobs.h.
//
// There is NO CPU fallback: without a gfx950 device every entry point that computes returns
// RPT_ERR_NO_DEVICE / RPT_ERR_HIP.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>              // types and prototypes only: librccl.so.1 is loaded on demand (rccl_api)

#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_build.h"
#include "host_cut.h"
#include "host_emap.h"
#include "host_env.h"
#include "host_light.h"
#include "host_map.h"
#include "host_med.h"
#include "host_mmap.h"
#include "host_move.h"
#include "host_nrm.h"
#include "host_refit.h"
#include "host_smooth.h"
#include "host_tacc.h"
#include "host_tex.h"
#include "host_upload.h"
#include "knobs.h"
#include "launch.h"
#include "launch_build.h"
#include "launch_cut.h"
#include "launch_emap.h"
#include "launch_env.h"
#include "launch_gdn.h"
#include "launch_light.h"
#include "launch_med.h"
#include "launch_mmap.h"
#include "launch_move.h"
#include "launch_nrm.h"
#include "launch_query.h"
#include "launch_rad.h"
#include "launch_smooth.h"
#include "launch_tacc.h"
#include "launch_tex.h"
#include "mesh_args.h"
#include "mesh_args_mmap.h"
#include "mesh_args_emap.h"
#include "mesh_args_med.h"
#include "mesh_args_query.h"
#include "mesh_args_rad.h"
#ifdef RPT_TEST_HOOKS
#include "../../include/rpt_test.h"
#endif

using namespace rptdev;
using rpthost::SceneImage;
using rpthost::SceneKind;
using rpthost::make_camera;
using rpthost::knobs;

// What one device of a context owns.
struct DevState {
    int device = -1;
    int rank = 0;                     // this device's rank in the world (row blocks b with b % world == rank)
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_ready = nullptr;
    void* tables = nullptr;           // the scene's device tables (host_upload.h, SceneImage::bytes): a large or mesh scene's, a small one's class map
    SceneMesh scene;                  // a large or mesh scene's kernel argument: device pointers into `tables` (rpthost::bind_scene)
    void* refit = nullptr;            // a mesh scene's refit tables (host_refit.h, RefitLayout): from the first rpt_update_meshes to the next upload
    bool refit_full = false;          // ... allocated by rpt_rebuild_meshes: their level order has room for every hierarchy over the scene's triangles
    void* build = nullptr;            // rpt_rebuild_meshes' own tables (host_build.h, BuildLayout) and the node table it binds: from the
    void* build_nodes = nullptr;      // context's first rebuild to the next upload
    size_t build_temp_bytes = 0;
    void* move = nullptr;             // the device-source calls' check tables (host_move.h, MoveLayout): on the context's first device, from its
                                      // first rpt_update_meshes_device / rpt_rebuild_meshes_device to the next upload
    void* move_stage = nullptr;       // ... and copies of sources that lie on another device (12 B per vertex of the scene), made on demand
    void* smooth = nullptr;           // smooth shading's tables (host_smooth.h, SmoothLayout): while some mesh is SMOOTH (rpt_set_mesh_shading)
    void* light = nullptr;            // mesh lights' tables (host_light.h, LightLayout): while some mesh is ON (rpt_set_mesh_lights)
    void* tex = nullptr;              // mesh textures' tables (host_tex.h, TexLayout): while some mesh is textured (rpt_set_mesh_textures)
    void* env = nullptr;              // the environment's tables (host_env.h, EnvLayout): while one is set (rpt_set_environment)
    void* cut = nullptr;              // mesh cutouts' tables (host_cut.h, CutLayout): while some mesh's cutout is ON (rpt_set_mesh_cutouts)
    void* nrm = nullptr;              // mesh normal maps' tables (host_nrm.h, NrmLayout): while some mesh's map is ON (rpt_set_mesh_normal_maps)
    void* mmap = nullptr;             // mesh material maps' tables (host_mmap.h, MmapLayout): while some mesh's map is ON (rpt_set_mesh_material_maps)
    void* emap = nullptr;             // mesh emission maps' tables (host_emap.h, EmapLayout): while some mesh's map is ON (rpt_set_mesh_emission_maps)
    void* med = nullptr;              // mesh media's tables (host_med.h, MedLayout): while some mesh carries a medium (rpt_set_mesh_media)
    void* query = nullptr;            // ray queries' own tables (host_query.h, QueryLayout): from a mesh scene's first query to the next upload
    void* rad = nullptr;              // radiance queries' own tables (host_rad.h): from a mesh scene's first radiance query to the next upload
    float* fb = nullptr;              // staging for the host-pointer API (this device's rows, or a whole image)
    size_t fb_bytes = 0;
    float* tile = nullptr;            // resident ColorBuffer rows of this rank: rows_padded x width RGBA f32
    // The gather runs beside the next render (gather_to_root): it sends a SNAPSHOT of the tile on a stream of its own.
    float* snap = nullptr;            // the tile as it was when the gather was asked for
    hipStream_t comm_stream = nullptr;
    hipEvent_t snap_ready = nullptr;  // on `stream`: the snapshot is taken
    hipEvent_t snap_free = nullptr;   // on `comm_stream`: the snapshot has been sent (the next one may overwrite it)
    bool snap_used = false;
    float* dn = nullptr;              // the denoiser's intermediate buffer, grown on demand
    size_t dn_bytes = 0;
    // `dn` is scratch of the CONTEXT, while rpt_denoise_device runs on whatever stream the caller passes: a use on another stream
    // than the previous one waits for that one's event (same stream: ordered anyway)
    hipEvent_t dn_done = nullptr;
    hipStream_t dn_stream = nullptr;
    bool dn_used = false;
    // dispatch (kernel_common.h, "Dispatch: units, their order, their hand-off"), for launches of `sched_tiles` tiles: per tile 4 dwords of
    // cost, 1 of order, 1 of sorting scratch, 4 of start stamps (development), then the hand-off words (SchedLayout)
    uint32_t* sched = nullptr;        // the tables of the CURRENT launch shape (an entry of sched_cache)
    uint32_t last_choice = 0;         // the last launch's KernelChoice as bits (include/rpt_test.h, rpt_debug_kernel_choice)
    uint32_t last_form = 0xFFFFFFFFu; // the last launch's mesh form (mesh_args_mmap.h, mesh_form_ext_of; include/rpt_test.h, rpt_debug_mesh_form), 0xFFFFFFFF: none
    uint32_t sched_tiles = 0;
    uint64_t sched_launches = 0;      // launches since the order was last started from scratch (the costs are re-sorted after the 1st, 2nd, 4th, ...)
    // A context that alternates between launch shapes (a viewer's preview and full frames, bench.py's legs, one rank's tile and the
    // whole frame) keeps each shape's learned order: up to kSchedCache tables, keyed by what decides a tile's cost (sched_for).
    struct SchedEntry { uint64_t key[2]; uint32_t* buf; uint32_t tiles; uint64_t launches; uint64_t stamp; };
    std::vector<SchedEntry> sched_cache;
    uint64_t sched_key[2] = {0, 0};
    uint64_t sched_clock = 0;
    hipEvent_t sched_done = nullptr;
    hipStream_t sched_stream = nullptr;
    bool sched_used = false;
    bool sync_used = false;           // a chunked launch has run: the hand-off's timeout word is worth a look (check_handoffs)
    ncclComm_t comm = nullptr;
};

struct rpt_ctx {
    std::vector<DevState> devs;       // devs[0] is the context's "own" device (rank 0 in a multi context)
    int world = 1;
    bool use_comm = false;            // tiles are gathered through RCCL (false: world 1, or peer copies)
    bool peer_gather = false;         // single process, RPT_GATHER=p2p: hipMemcpyPeerAsync instead of RCCL
    uint32_t tile_rows = 2;
    uint32_t dispatch[4] = {0xFFFFFFFFu, 0, 0, 0};   // rpt_set_dispatch: cost_order (0xFFFFFFFF: the environment's defaults), unit_rounds, unit_min_spp, unit_slots
    rpthost::SceneState scene;        // its class, camera, small scenes' kernel argument (host_upload.h); every device's tables: DevState
    rpthost::RefitPlan refit;         // a mesh scene's plan for rpt_update_meshes (host_refit.h)
    rpthost::SmoothPlan smooth;       // its meshes' shading modes and the sizes of every device's smooth tables (host_smooth.h)
    rpthost::LightPlan light;         // which of its meshes are lights and the sizes of every device's light tables (host_light.h)
    rpthost::TexPlan tex;             // which of its meshes are textured, their UVs and the sizes of every device's texture tables (host_tex.h)
    rpthost::EnvPlan env;             // its environment's size, mode and scale, and Q as the devices computed it (host_env.h)
    rpthost::CutPlan cut;             // which of its meshes have a cutout and where each one's mask lies on every device (host_cut.h)
    rpthost::NrmPlan nrm;             // which of its meshes have a normal map and where each one's texels lie on every device (host_nrm.h)
    rpthost::MmapPlan mmap;           // which of its meshes have a material map and where each one's texels lie on every device (host_mmap.h)
    rpthost::EmapPlan emap;           // which of its meshes have an emission map and where each one's texels lie on every device (host_emap.h)
    rpthost::MedPlan med;             // which of its meshes carry a medium and the sizes of every device's media tables (host_med.h)
    rpthost::MedPlan rad;             // the plan of radiance queries' own tables: the scene's sizes, no medium (host_rad.h); made with the tables
    // resident ColorBuffer (buffer.rs:6-14): pixels as per-rank tiles + frames
    uint32_t res_w = 0, res_h = 0, res_tile_rows = 0, res_rows_padded = 0;
    uint64_t res_frames = 0;
    bool has_res = false;
    // on the root device: rank-major gathered tiles, the assembled image, the u8 frame
    float* gathered = nullptr;
    float* image = nullptr;
    uint8_t* frame_u8 = nullptr;
    void* stage = nullptr;            // page-locked host staging for downloads into pageable buffers (download_to_host)
    size_t stage_bytes = 0;
    hipEvent_t gather_done = nullptr;       // on the root's comm_stream: the assembled image of the last gather is complete
    bool gather_issued = false;
    bool timed = false;               // ev_begin / ev_end bracket a render
    std::string err;

    bool is_root() const { return devs[0].rank == 0; }
    bool plain() const { return world == 1 && !use_comm; }           // rpt_create: the tile IS the image
};

static thread_local std::string g_err;

static void set_err(rpt_ctx* ctx, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_err = buf;
}

#define RPT_HIP_CHECK(ctx, call)                                                                  \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            set_err(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return RPT_ERR_HIP;                                                                   \
        }                                                                                         \
    } while (0)

#define RPT_CHECK_RC(call) do { const int rc_ = (call); if (rc_ != RPT_OK) return rc_; } while (0)

// Every entry point runs on its context's device(s) and puts the caller's current device back afterwards
// (the caller may be a torch process with its own idea of the current device).
struct DeviceGuard {
    int prev = -1;
    hipError_t status;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        status = (prev == device) ? hipSuccess : hipSetDevice(device);
    }
    hipError_t to(int device) { return hipSetDevice(device); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define RPT_ON_DEVICE(ctx)                        \
    DeviceGuard guard_((ctx)->devs[0].device);    \
    RPT_HIP_CHECK(ctx, guard_.status)

// ---- RCCL, loaded on demand ------------------------------------------------------------------------------
// Only multi-GPU contexts need it, and a host process (torch) may already have its own copy of librccl.so.1 loaded:
// dlopen by soname then returns that one instead of bringing in a second runtime.
struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
};

// Loads librccl once per process (thread-safe: a function-local static's initialiser); false when it cannot be loaded.
static bool rccl_load(RcclApi& api)
{
    const char* forced = knobs().rccl_lib.empty() ? nullptr : knobs().rccl_lib.c_str();   // tests: a name that cannot be loaded exercises the error path
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    if (forced) api.handle = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
    else
        for (const char* n : names) {
            api.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
        }
    if (!api.handle) {
        const char* e = dlerror();                                   // (the call clears the pending error: read it once)
        api.error = e ? e : "dlopen(librccl.so.1) failed";
        return false;
    }
    bool ok = true;
    auto sym = [&](const char* name) { void* p = dlsym(api.handle, name); if (!p) { ok = false; api.error = std::string("librccl: missing symbol ") + name; } return p; };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.Send = (decltype(api.Send))sym("ncclSend");
    api.Recv = (decltype(api.Recv))sym("ncclRecv");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    if (!ok) { dlclose(api.handle); api.handle = nullptr; return false; }
    return true;
}

static RcclApi g_rccl;
static RcclApi* rccl_api()
{
    static const bool loaded = rccl_load(g_rccl);
    return loaded ? &g_rccl : nullptr;
}
static const char* rccl_why() { return g_rccl.error.empty() ? "unknown reason" : g_rccl.error.c_str(); }

#define RPT_RCCL_CHECK(ctx, api, call)                                                            \
    do {                                                                                          \
        ncclResult_t r_ = (call);                                                                 \
        if (r_ != ncclSuccess) {                                                                  \
            set_err(ctx, "%s failed: %s (%s:%d)", #call, (api)->GetErrorString(r_), __FILE__, __LINE__); \
            return RPT_ERR_RCCL;                                                                  \
        }                                                                                         \
    } while (0)

// Where things are in DevState::sched (dwords), for n tiles.
struct SchedLayout {
    size_t n;
    size_t cost() const { return 0; }
    size_t order() const { return 4 * n; }
    size_t sorted() const { return 5 * n; }
    size_t start() const { return 6 * n; }
    size_t sync() const { return 10 * n; }                          // kSyncTimeout (kept), then from kSyncTicket on: zeroed before a chunked launch
    size_t total() const { return 10 * n + 32 + n; }
};
constexpr size_t kSyncTimeoutWord = 0, kSyncZeroFrom = 16, kSyncDoneFrom = 32;     // = kernel_common.h's kSyncTimeout / kSyncTicket / kSyncDone

// Dispatch policy of a context (include/rpt.h, rpt_set_dispatch); the environment gives the defaults.
struct DispatchPolicy {
    uint32_t cost_order, unit_rounds, unit_min_spp, unit_slots;
};
static DispatchPolicy default_dispatch() { return DispatchPolicy{knobs().dispatch_order, knobs().unit_rounds, knobs().unit_min_spp, 0u}; }

static DispatchPolicy policy_of(const rpt_ctx* ctx)
{
    if (ctx->dispatch[0] == 0xFFFFFFFFu) return default_dispatch();
    return DispatchPolicy{ctx->dispatch[0], ctx->dispatch[1], ctx->dispatch[2], ctx->dispatch[3]};
}

// How many chunks of samples a launch of `nblocks` tiles x `spp` samples is cut into (kernel_common.h, units): enough for
// `unit_rounds` rounds of workgroups on the device, no chunk shorter than `unit_min_spp` samples; 1 when the tiles alone are
// that many rounds, or fit the device at once (then nothing waits for a slot and there is nothing to balance).  Measured
// (tools/tile_rows_time.py, tools/launch_size_time.py): one rank's share of configs[2] (3.2 rounds, 1 024 spp) 1 / 2 / 4 / 8
// chunks 11.05 / 10.92 / 11.22 / 11.24 Gsamples/s; 800x600 x 128 spp (1.5 rounds) 1 / 4 chunks 8.75 / 10.2; configs[1] (6.4
// rounds) 1 / 2 / 4 chunks 11.75 / 11.73 / 11.47; configs[3] (64 spp) 1 / 2 chunks 3.05 / 2.97: a chunk's end drains every wave.
static uint32_t unit_chunks(const DispatchPolicy& pol, uint64_t nblocks, uint32_t spp, uint32_t slots)
{
    if (pol.unit_rounds == 0u || pol.unit_min_spp == 0u || nblocks <= slots || spp < 2u * pol.unit_min_spp) return 1u;
    // From a third of the target on (configs[1]: 6.4 rounds) cutting buys nothing — 11.75 against 11.73 Gsamples/s — and every chunk
    // reads and writes the pixels once more (HBM traffic per launch 148 MB instead of 80): such launches stay whole.
    if (nblocks * 3u >= (uint64_t)pol.unit_rounds * slots) return 1u;
    const uint64_t want = ((uint64_t)pol.unit_rounds * slots + nblocks - 1u) / nblocks;
    const uint64_t most = spp / pol.unit_min_spp;
    const uint64_t n = want < most ? want : most;
    return n < 1u ? 1u : (uint32_t)n;
}

// Launches of at least this many samples per pixel re-sort the order from their own costs every time (one small kernel behind
// the launch); shorter ones only after the 1st, 2nd, 4th, 8th ... launch since the order was started.
constexpr uint32_t kOrderAlwaysFromSpp = 16;
// Small scenes: launches of at most knobs().compact_max_spp samples per pixel take the compacting kernel (k_compact.hip).
// (1 since round 3: 1080p, 1 spp 7.12 vs 6.83 Gsamples/s for the megakernel, 2 spp 7.01 vs 7.39: profiles/r3/spp_curve.txt)

// what rpt_update_meshes and rpt_rebuild_meshes allocated on a device (its current device; nothing of the scene may still run)
static void free_mesh_work(DevState& d)
{
    if (d.refit) { (void)hipFree(d.refit); d.refit = nullptr; }
    if (d.build) { (void)hipFree(d.build); d.build = nullptr; }
    if (d.build_nodes) { (void)hipFree(d.build_nodes); d.build_nodes = nullptr; }
    if (d.move) { (void)hipFree(d.move); d.move = nullptr; }
    if (d.move_stage) { (void)hipFree(d.move_stage); d.move_stage = nullptr; }
    if (d.smooth) { (void)hipFree(d.smooth); d.smooth = nullptr; }
    if (d.light) { (void)hipFree(d.light); d.light = nullptr; }
    if (d.tex) { (void)hipFree(d.tex); d.tex = nullptr; }
    if (d.env) { (void)hipFree(d.env); d.env = nullptr; }
    if (d.cut) { (void)hipFree(d.cut); d.cut = nullptr; }
    if (d.nrm) { (void)hipFree(d.nrm); d.nrm = nullptr; }
    if (d.mmap) { (void)hipFree(d.mmap); d.mmap = nullptr; }
    if (d.emap) { (void)hipFree(d.emap); d.emap = nullptr; }
    if (d.med) { (void)hipFree(d.med); d.med = nullptr; }
    if (d.query) { (void)hipFree(d.query); d.query = nullptr; }
    if (d.rad) { (void)hipFree(d.rad); d.rad = nullptr; }
    d.refit_full = false;
    d.build_temp_bytes = 0;
}

static void free_dev(DevState& d)
{
    DeviceGuard guard(d.device);
    if (d.fb) (void)hipFree(d.fb);
    if (d.tile) (void)hipFree(d.tile);
    if (d.tables) (void)hipFree(d.tables);
    free_mesh_work(d);
    if (d.dn) (void)hipFree(d.dn);
    for (DevState::SchedEntry& e : d.sched_cache) if (e.buf) (void)hipFree(e.buf);
    if (d.sched_done) (void)hipEventDestroy(d.sched_done);
    if (d.ev_begin) (void)hipEventDestroy(d.ev_begin);
    if (d.ev_end) (void)hipEventDestroy(d.ev_end);
    if (d.ev_ready) (void)hipEventDestroy(d.ev_ready);
    if (d.snap) (void)hipFree(d.snap);
    if (d.snap_ready) (void)hipEventDestroy(d.snap_ready);
    if (d.snap_free) (void)hipEventDestroy(d.snap_free);
    if (d.comm_stream) (void)hipStreamDestroy(d.comm_stream);
    if (d.dn_done) (void)hipEventDestroy(d.dn_done);
    if (d.stream) (void)hipStreamDestroy(d.stream);
    d = DevState();
}

// device checks + stream/events for one device of a context
static int open_dev(DevState& d, int device_id, int rank, const char* who)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_err(nullptr, "%s: no HIP device (%s); this library has no CPU fallback", who, e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return RPT_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= count) { set_err(nullptr, "%s: device %d out of range [0,%d)", who, device_id, count); return RPT_ERR_INVALID_ARG; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) { set_err(nullptr, "%s: hipGetDeviceProperties failed", who); return RPT_ERR_HIP; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(nullptr, "%s: device %d is %s; this library is built for gfx950 only", who, device_id, prop.gcnArchName);
        return RPT_ERR_NO_DEVICE;
    }
    d.device = device_id;
    d.rank = rank;
    DeviceGuard guard(device_id);
    if (guard.status != hipSuccess || hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&d.ev_begin) != hipSuccess || hipEventCreate(&d.ev_end) != hipSuccess ||
        hipEventCreateWithFlags(&d.ev_ready, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&d.comm_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&d.snap_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d.snap_free, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d.dn_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d.sched_done, hipEventDisableTiming) != hipSuccess) {
        set_err(nullptr, "%s: cannot create a stream on device %d", who, device_id);
        free_dev(d);
        return RPT_ERR_HIP;
    }
    return RPT_OK;
}

static void free_resident(rpt_ctx* ctx)
{
    for (DevState& d : ctx->devs) {
        DeviceGuard guard(d.device);
        if (d.tile) { (void)hipFree(d.tile); d.tile = nullptr; }
        if (d.snap) { (void)hipFree(d.snap); d.snap = nullptr; }
        d.snap_used = false;
    }
    DeviceGuard guard(ctx->devs[0].device);
    if (ctx->gathered) { (void)hipFree(ctx->gathered); ctx->gathered = nullptr; }
    if (ctx->image) { (void)hipFree(ctx->image); ctx->image = nullptr; }
    if (ctx->frame_u8) { (void)hipFree(ctx->frame_u8); ctx->frame_u8 = nullptr; }
    if (ctx->stage) { (void)hipHostFree(ctx->stage); ctx->stage = nullptr; ctx->stage_bytes = 0; }
    if (ctx->gather_done) { (void)hipEventDestroy(ctx->gather_done); ctx->gather_done = nullptr; }
    ctx->gather_issued = false;
    ctx->has_res = false;
    ctx->res_w = ctx->res_h = ctx->res_tile_rows = ctx->res_rows_padded = 0;
    ctx->res_frames = 0;
}

static uint32_t rows_padded_for(uint32_t height, uint32_t tile_rows, uint32_t world) { return tile_rows_padded(height, tile_rows, world); }

// Copy the rows rank `rank` owns between a host top-down image and its compact tile (either direction), following
// rpt_tile_copy_plan: one strided copy for the full blocks plus one plain copy when the rank owns the image's short last block.
static hipError_t copy_rank_rows(bool to_device, float* host_image, float* tile, uint32_t width, uint32_t height, uint32_t tile_rows,
                                 uint32_t rank, uint32_t world, hipStream_t st)
{
    const size_t row_bytes = (size_t)width * 16u;
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    rpt_tile_plan p;
    if (rpt_tile_copy_plan(height, tile_rows, rank, world, &p) != RPT_OK) return hipErrorInvalidValue;
    char* h0 = reinterpret_cast<char*>(host_image);
    char* t0 = reinterpret_cast<char*>(tile);
    if (p.full_blocks) {
        const size_t block_bytes = row_bytes * p.block_rows;
        char* h = h0 + row_bytes * p.host_row0;
        const size_t hpitch = row_bytes * p.host_row_stride;
        hipError_t e;
        if (p.full_blocks == 1) e = to_device ? hipMemcpyAsync(t0, h, block_bytes, kind, st) : hipMemcpyAsync(h, t0, block_bytes, kind, st);
        else e = to_device ? hipMemcpy2DAsync(t0, block_bytes, h, hpitch, block_bytes, p.full_blocks, kind, st)
                           : hipMemcpy2DAsync(h, hpitch, t0, block_bytes, block_bytes, p.full_blocks, kind, st);
        if (e != hipSuccess) return e;
    }
    if (p.ragged_rows) {
        char* h = h0 + row_bytes * p.ragged_host_row0;
        char* t = t0 + row_bytes * p.ragged_tile_row0;
        return to_device ? hipMemcpyAsync(t, h, row_bytes * p.ragged_rows, kind, st) : hipMemcpyAsync(h, t, row_bytes * p.ragged_rows, kind, st);
    }
    return hipSuccess;
}

// The dispatch tables for a launch of `nblocks` tiles of this shape: the context's current ones if the shape is the same, else the
// cached ones of that shape (their learned order intact), else new ones (bottom rows first, no costs).  Nothing is freed — and so
// nothing waits for the device — unless kSchedCache shapes are already held; then the least recently used goes.
constexpr size_t kSchedCache = 6;
static int sched_for(rpt_ctx* ctx, DevState& d, uint32_t nblocks, uint32_t width, uint32_t rows_local, uint32_t tile_rows, uint32_t rank, uint32_t world, hipStream_t stream)
{
    const uint64_t key[2] = {((uint64_t)width << 32) | rows_local, ((uint64_t)tile_rows << 40) ^ ((uint64_t)rank << 20) ^ (uint64_t)world};
    d.sched_clock += 1;
    if (d.sched && d.sched_key[0] == key[0] && d.sched_key[1] == key[1] && d.sched_tiles == nblocks) {
        for (DevState::SchedEntry& e : d.sched_cache) if (e.buf == d.sched) e.stamp = d.sched_clock;
        return RPT_OK;
    }
    for (DevState::SchedEntry& e : d.sched_cache) if (e.buf == d.sched) e.launches = d.sched_launches;     // park the current shape
    DevState::SchedEntry* hit = nullptr;
    for (DevState::SchedEntry& e : d.sched_cache) if (e.key[0] == key[0] && e.key[1] == key[1] && e.tiles == nblocks) hit = &e;
    if (!hit) {
        if (d.sched_cache.size() >= kSchedCache) {
            size_t lru = 0;
            for (size_t i = 1; i < d.sched_cache.size(); ++i) if (d.sched_cache[i].stamp < d.sched_cache[lru].stamp) lru = i;
            RPT_HIP_CHECK(ctx, hipFree(d.sched_cache[lru].buf));     // (hipFree waits for the device: rare by construction)
            d.sched_cache.erase(d.sched_cache.begin() + (long)lru);
        }
        const SchedLayout lay{(size_t)nblocks};
        uint32_t* buf = nullptr;
        RPT_HIP_CHECK(ctx, hipMalloc((void**)&buf, lay.total() * sizeof(uint32_t)));
        d.sched_cache.push_back(DevState::SchedEntry{{key[0], key[1]}, buf, nblocks, 0, d.sched_clock});
        hit = &d.sched_cache.back();
        RPT_HIP_CHECK(ctx, hipMemsetAsync(buf + lay.sync(), 0, (32 + lay.n) * sizeof(uint32_t), stream));
        RPT_HIP_CHECK(ctx, rptlaunch::sched_init(buf + lay.cost(), buf + lay.order(), nblocks, stream));
    }
    hit->stamp = d.sched_clock;
    d.sched = hit->buf;
    d.sched_tiles = hit->tiles;
    d.sched_launches = hit->launches;
    d.sched_key[0] = key[0]; d.sched_key[1] = key[1];
    return RPT_OK;
}

// Device d's mesh scene as mesh_args.h binds kernel arguments from it: mesh_scene_of<S>(mesh_view_of(ctx, d)), light_tables_of.
static rptargs::MeshView mesh_view_of(const rpt_ctx* ctx, const DevState& d)
{
    return rptargs::MeshView{d.scene, d.refit, d.smooth, d.light, d.tex, d.env, d.cut, d.nrm,
                             ctx->refit, ctx->smooth, ctx->light, ctx->tex, ctx->env, ctx->cut, ctx->nrm};
}

// One mesh render form: its argument (mesh_args.h) with the launch's camera and flags, through its launcher.
template <class S, class Launcher>
static hipError_t launch_mesh_form(const rptargs::MeshView& view, const SceneMesh& scm, Launcher launcher, const RenderParams& rp, uint32_t grid, hipStream_t stream)
{
    S s = rptargs::mesh_scene_of<S>(view);
    s.cam = scm.cam;
    s.flags = scm.flags;
    return launcher(s, rp, grid, stream);
}

// One material-mapped render form (mesh_args_mmap.h), likewise.
template <class S, class Launcher>
static hipError_t launch_mesh_map_form(const rptargs::MeshView& view, const rptargs::MmapView& maps, const SceneMesh& scm, Launcher launcher, const RenderParams& rp,
                                       uint32_t grid, hipStream_t stream)
{
    S s = rptargs::mesh_map_scene_of<S>(view, maps);
    s.cam = scm.cam;
    s.flags = scm.flags;
    return launcher(s, rp, grid, stream);
}

// One emission-mapped render form (mesh_args_emap.h), likewise.
template <class S, class Launcher>
static hipError_t launch_mesh_emit_form(const rptargs::MeshView& view, const rptargs::MmapView& maps, bool material_maps, const rptargs::EmapView& emits,
                                        const SceneMesh& scm, Launcher launcher, const RenderParams& rp, uint32_t grid, hipStream_t stream)
{
    S s = rptargs::mesh_emit_scene_of<S>(view, maps, material_maps, emits);
    s.cam = scm.cam;
    s.flags = scm.flags;
    return launcher(s, rp, grid, stream);
}

// One media render form (mesh_args_med.h), likewise.
template <class S, class Launcher>
static hipError_t launch_mesh_med_form(const rptargs::MeshView& view, const rptargs::MmapView& maps, bool material_maps, const rptargs::EmapView& emits,
                                       bool emission_maps, const rptargs::MedView& meds, const SceneMesh& scm, Launcher launcher, const RenderParams& rp,
                                       uint32_t grid, hipStream_t stream)
{
    S s = rptargs::mesh_med_scene_of<S>(view, maps, material_maps, emits, emission_maps, meds);
    s.cam = scm.cam;
    s.flags = scm.flags;
    return launcher(s, rp, grid, stream);
}

// One render launch sequence on one device.
static int launch_render(rpt_ctx* ctx, DevState& d, float* pixels_dev, uint32_t width, uint32_t height, uint64_t frames_done, uint32_t spp,
                         uint64_t seed, uint32_t flags, uint32_t tile_rows, uint32_t rank, uint32_t world, hipStream_t stream)
{
    if (world == 1) tile_rows = height;                              // one block: local row == global row
    if (flags & ~(uint32_t)RPT_RENDER_ALL_FLAGS) {
        set_err(ctx, "render: unknown flag bits 0x%x (bits 2-4, 6-7, 9-10 named A/B kernel forms until ABI 3; they are gone, include/rpt.h)", flags & ~(uint32_t)RPT_RENDER_ALL_FLAGS);
        return RPT_ERR_INVALID_ARG;
    }
    const SceneKind kind = ctx->scene.kind;
    const bool media = ctx->scene.media;
    SceneSmallSdf scs = ctx->scene.small;
    SceneLarge scl = d.scene;
    SceneMesh scm = d.scene;
    const bool smooth = kind == SceneKind::mesh && d.smooth && d.refit && ctx->smooth.any();      // some mesh is SMOOTH: k_smooth.hip's form
    const bool lights = kind == SceneKind::mesh && d.light && d.refit && ctx->light.any();        // some mesh is ON: k_light.hip's form, for flat and smooth meshes alike
    const bool textured = kind == SceneKind::mesh && d.tex && d.refit && ctx->tex.any();          // some mesh is textured: k_tex.hip's forms, over either of the two above
    const bool environment = kind == SceneKind::mesh && d.env && d.refit && ctx->env.any();       // an environment is set: k_env.hip's one form, over all of the above
    const bool cutouts = kind == SceneKind::mesh && d.cut && d.tex && d.refit && ctx->cut.any();  // some mesh's cutout is ON: k_cut.hip's forms, over the textured mesh-light form or the environment's
    const bool normal_maps = kind == SceneKind::mesh && d.nrm && d.tex && d.refit && ctx->nrm.any();   // some mesh's normal map is ON: k_nrm.hip's forms, over the four above that hold every table
    const bool material_maps = kind == SceneKind::mesh && d.mmap && d.tex && d.refit && ctx->mmap.any();   // some mesh's material map is ON: k_mmap.hip's forms, over the eight textured forms that hold every table
    const bool emission_maps = kind == SceneKind::mesh && d.emap && d.tex && d.refit && ctx->emap.any();   // some mesh's emission map is ON: k_emap.hip's forms, over the eight material-mapped forms
    const bool mesh_media = kind == SceneKind::mesh && d.med && d.refit && ctx->med.any();   // some mesh carries a medium: k_med.hip's forms, over the eight emission-mapped forms
    scs.cam = scl.cam = scm.cam = make_camera(ctx->scene.camera, (float)width, (float)height);
    const bool in_hbm = kind == SceneKind::large || kind == SceneKind::mesh;     // the scene's tables are in device memory
    const bool has_sdf = !in_hbm && scs.sdf.n_prims > 0;
    const bool nested = (flags & RPT_RENDER_NESTED_LOOPS) != 0;
    const bool fast = (flags & RPT_RENDER_FAST_MATH) != 0;

    RenderParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.pixels = pixels_dev;
    rp.width = width; rp.height = height;
    rp.rows_local = tile_row_count(height, tile_rows, rank, world);
    rp.tile_rows = tile_rows; rp.rank = rank; rp.world = world;
    rp.seed = seed;
    rp.tiles_x = (width + 15u) / 16u;
    rp.shade_threshold = has_sdf ? knobs().sdf_shade_room : knobs().shade_threshold;      // (k_sdf.hip: the second room's threshold; knobs.h keeps both in 1..64)
    // (small scenes' megakernel only; 8 ... 48 are within 2 % of each other, +5.9 % over finishing un-voted)
    rp.finish_threshold = knobs().finish_threshold;
    rp.march_min_lanes = knobs().sdf_march_min_lanes;
    rp.compact = (!in_hbm && !has_sdf && ((flags & RPT_RENDER_SMALL_COMPACT) || spp <= knobs().compact_max_spp)) ? 1u : 0u;
    if (flags & RPT_RENDER_RUSSIAN_ROULETTE) { scs.flags |= kSceneFlagRussianRoulette; scl.flags |= kSceneFlagRussianRoulette; scm.flags |= kSceneFlagRussianRoulette; }
    if (rp.rows_local == 0) return RPT_OK;
    const uint32_t tiles_y = (rp.rows_local + 15u) / 16u;
    const uint64_t nblocks = (uint64_t)rp.tiles_x * tiles_y;
    if (nblocks > 0x7FFFFFFFull) { set_err(ctx, "render: grid too large"); return RPT_ERR_INVALID_ARG; }
    // The nested-loop kernel is the differential baseline of the reference's own scene class; the other classes have one form.
    if (nested && (kind == SceneKind::large || has_sdf || media)) {
        set_err(ctx, "render: RPT_RENDER_NESTED_LOOPS exists for small scenes without an SDF object or media only");
        return RPT_ERR_UNSUPPORTED;
    }
    if (kind == SceneKind::mesh && (flags & (RPT_RENDER_FAST_MATH | RPT_RENDER_NESTED_LOOPS | RPT_RENDER_SMALL_COMPACT))) {
        set_err(ctx, "render: scenes with meshes have one kernel form (strict, path-regenerating): no RPT_RENDER_FAST_MATH, NESTED_LOOPS or SMALL_COMPACT");
        return RPT_ERR_UNSUPPORTED;
    }
    if (media && fast) {
        set_err(ctx, "render: scenes with participating media (RPT_SCENE_MEDIA) have no relaxed-arithmetic kernel form");
        return RPT_ERR_UNSUPPORTED;
    }

    // Which instantiation (launch.h, KernelChoice): the kernels that know the reference scene's table sizes, and those that read a
    // hit's material from a table (at most three primitives, at most one of them with a procedural material).
    KernelChoice kc;
    {
        const SceneSmall& sc = scs;
        const bool can_size = !knobs().no_sized_kernels && !media && !in_hbm && !nested;
        kc.sized = can_size && !has_sdf && sc.n_spheres == 2u && sc.n_planes == 1u && sc.n_lights == 1u;      // (kernel_common.h, RPT_REFERENCE_SIZES)
        kc.sized_sdf = (can_size && has_sdf && sc.n_planes == 1u && sc.n_lights == 1u && scs.sdf.n_prims <= 4u) ? scs.sdf.n_prims : 0u;
        kc.material_table = !knobs().no_material_table && !media && !in_hbm && !nested && rptlaunch::material_table_fits_small(scs, has_sdf);      // (with or without the sizes)
        kc.material_table_wide = !knobs().no_material_table && !media && !in_hbm && !nested && !has_sdf && !rp.compact && rptlaunch::material_table_fits_small(scs, false, 4u);
        // five to twelve primitives: the table by class of accepted set (launch.h, MatClassMap), in the megakernel of small scenes
        if (!kc.material_table && !kc.material_table_wide && !knobs().no_material_table && !media && !in_hbm && !nested && !has_sdf && !rp.compact &&
            ctx->scene.class_map_ok && d.tables) {
            kc.material_table_mapped = true;
            kc.class_map = ctx->scene.class_map;
            kc.class_map.cls = reinterpret_cast<const uint8_t*>(d.tables);
        }
        kc.extra_lds = knobs().debug_extra_lds;
        d.last_choice = (kc.sized ? 1u : 0u) | (kc.material_table ? 2u : 0u) | (kc.material_table_wide ? 4u : 0u) | (kc.material_table_mapped ? 8u : 0u) |
                        ((kc.material_table_mapped ? kc.class_map.n_classes : 0u) << 8) | (kc.sized_sdf << 16) |
                        (fast ? 1u << 20 : 0u) | (rp.compact && !nested ? 1u << 21 : 0u) |
                        (rp.compact && !nested && nblocks <= kCompactDenseMaxBlocks ? 1u << 22 : 0u) | (nested ? 1u << 23 : 0u) |
                        (media || mesh_media ? 1u << 24 : 0u) | (kind == SceneKind::mesh ? 1u << 25 : 0u) |
                        (smooth ? 1u << 26 : 0u) | (lights ? 1u << 27 : 0u) | (textured ? 1u << 28 : 0u) |
                        (environment ? 1u << 29 : 0u) | (cutouts ? 1u << 30 : 0u) | (normal_maps ? 1u << 31 : 0u);
        // (material and emission maps have no bit: the mesh form says it — 12 .. 19 and 20 .. 27, include/rpt_test.h, rpt_debug_mesh_form)
        d.last_form = kind == SceneKind::mesh ? rptargs::mesh_form_med_of(smooth, lights, textured, environment, cutouts, normal_maps, material_maps, emission_maps, mesh_media)
                                              : 0xFFFFFFFFu;
    }
    const auto launch = [&](uint32_t grid) -> hipError_t {
        if (kind == SceneKind::mesh) {
            using rptargs::MeshForm;
            const rptargs::MeshView view = mesh_view_of(ctx, d);
            if (d.last_form >= rptargs::kMeshFormMedFirst) {
                using rptargs::MeshMedForm;
                const rptargs::MmapView maps{d.mmap, ctx->mmap};
                const rptargs::EmapView emits{d.emap, ctx->emap};
                const rptargs::MedView meds{d.med, ctx->med};
                switch ((MeshMedForm)d.last_form) {
                case MeshMedForm::light_tex: return launch_mesh_med_form<SceneMeshMed>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med, rp, grid, stream);
                case MeshMedForm::env: return launch_mesh_med_form<SceneMeshMedEnv>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med_env, rp, grid, stream);
                case MeshMedForm::cut: return launch_mesh_med_form<SceneMeshMedCut>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med_cut, rp, grid, stream);
                case MeshMedForm::cut_env: return launch_mesh_med_form<SceneMeshMedCutEnv>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med_cut_env, rp, grid, stream);
                case MeshMedForm::nrm: return launch_mesh_med_form<SceneMeshMedNrm>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med_nrm, rp, grid, stream);
                case MeshMedForm::nrm_env: return launch_mesh_med_form<SceneMeshMedNrmEnv>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med_nrm_env, rp, grid, stream);
                case MeshMedForm::nrm_cut: return launch_mesh_med_form<SceneMeshMedNrmCut>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med_nrm_cut, rp, grid, stream);
                case MeshMedForm::nrm_cut_env: return launch_mesh_med_form<SceneMeshMedNrmCutEnv>(view, maps, material_maps, emits, emission_maps, meds, scm, rptlaunch::render_mesh_med_nrm_cut_env, rp, grid, stream);
                }
            }
            if (d.last_form >= rptargs::kMeshFormEmitFirst) {
                using rptargs::MeshEmitForm;
                const rptargs::MmapView maps{d.mmap, ctx->mmap};
                const rptargs::EmapView emits{d.emap, ctx->emap};
                switch ((MeshEmitForm)d.last_form) {
                case MeshEmitForm::light_tex: return launch_mesh_emit_form<SceneMeshEmit>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit, rp, grid, stream);
                case MeshEmitForm::env: return launch_mesh_emit_form<SceneMeshEmitEnv>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit_env, rp, grid, stream);
                case MeshEmitForm::cut: return launch_mesh_emit_form<SceneMeshEmitCut>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit_cut, rp, grid, stream);
                case MeshEmitForm::cut_env: return launch_mesh_emit_form<SceneMeshEmitCutEnv>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit_cut_env, rp, grid, stream);
                case MeshEmitForm::nrm: return launch_mesh_emit_form<SceneMeshEmitNrm>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit_nrm, rp, grid, stream);
                case MeshEmitForm::nrm_env: return launch_mesh_emit_form<SceneMeshEmitNrmEnv>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit_nrm_env, rp, grid, stream);
                case MeshEmitForm::nrm_cut: return launch_mesh_emit_form<SceneMeshEmitNrmCut>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit_nrm_cut, rp, grid, stream);
                case MeshEmitForm::nrm_cut_env: return launch_mesh_emit_form<SceneMeshEmitNrmCutEnv>(view, maps, material_maps, emits, scm, rptlaunch::render_mesh_emit_nrm_cut_env, rp, grid, stream);
                }
            }
            if (d.last_form >= rptargs::kMeshFormMapFirst) {
                using rptargs::MeshMapForm;
                const rptargs::MmapView maps{d.mmap, ctx->mmap};
                switch ((MeshMapForm)d.last_form) {
                case MeshMapForm::light_tex: return launch_mesh_map_form<SceneMeshMap>(view, maps, scm, rptlaunch::render_mesh_map, rp, grid, stream);
                case MeshMapForm::env: return launch_mesh_map_form<SceneMeshMapEnv>(view, maps, scm, rptlaunch::render_mesh_map_env, rp, grid, stream);
                case MeshMapForm::cut: return launch_mesh_map_form<SceneMeshMapCut>(view, maps, scm, rptlaunch::render_mesh_map_cut, rp, grid, stream);
                case MeshMapForm::cut_env: return launch_mesh_map_form<SceneMeshMapCutEnv>(view, maps, scm, rptlaunch::render_mesh_map_cut_env, rp, grid, stream);
                case MeshMapForm::nrm: return launch_mesh_map_form<SceneMeshMapNrm>(view, maps, scm, rptlaunch::render_mesh_map_nrm, rp, grid, stream);
                case MeshMapForm::nrm_env: return launch_mesh_map_form<SceneMeshMapNrmEnv>(view, maps, scm, rptlaunch::render_mesh_map_nrm_env, rp, grid, stream);
                case MeshMapForm::nrm_cut: return launch_mesh_map_form<SceneMeshMapNrmCut>(view, maps, scm, rptlaunch::render_mesh_map_nrm_cut, rp, grid, stream);
                case MeshMapForm::nrm_cut_env: return launch_mesh_map_form<SceneMeshMapNrmCutEnv>(view, maps, scm, rptlaunch::render_mesh_map_nrm_cut_env, rp, grid, stream);
                }
            }
            switch (rptargs::mesh_form_of(smooth, lights, textured, environment, cutouts, normal_maps)) {
            case MeshForm::nrm_cut_env: return launch_mesh_form<SceneMeshNrmCutEnv>(view, scm, rptlaunch::render_mesh_nrm_cut_env, rp, grid, stream);
            case MeshForm::nrm_cut: return launch_mesh_form<SceneMeshNrmCut>(view, scm, rptlaunch::render_mesh_nrm_cut, rp, grid, stream);
            case MeshForm::nrm_env: return launch_mesh_form<SceneMeshNrmEnv>(view, scm, rptlaunch::render_mesh_nrm_env, rp, grid, stream);
            case MeshForm::nrm: return launch_mesh_form<SceneMeshNrm>(view, scm, rptlaunch::render_mesh_nrm, rp, grid, stream);
            case MeshForm::cut_env: return launch_mesh_form<SceneMeshCutEnv>(view, scm, rptlaunch::render_mesh_cut_env, rp, grid, stream);
            case MeshForm::cut: return launch_mesh_form<SceneMeshCut>(view, scm, rptlaunch::render_mesh_cut, rp, grid, stream);
            case MeshForm::env: return launch_mesh_form<SceneMeshEnv>(view, scm, rptlaunch::render_mesh_env, rp, grid, stream);
            case MeshForm::light_tex: return launch_mesh_form<SceneMeshLightTex>(view, scm, rptlaunch::render_mesh_light_tex, rp, grid, stream);
            case MeshForm::tex: return launch_mesh_form<SceneMeshTex>(view, scm, rptlaunch::render_mesh_tex, rp, grid, stream);
            case MeshForm::light: return launch_mesh_form<SceneMeshLight>(view, scm, rptlaunch::render_mesh_light, rp, grid, stream);
            case MeshForm::smooth: return launch_mesh_form<SceneMeshSmooth>(view, scm, rptlaunch::render_mesh_smooth, rp, grid, stream);
            case MeshForm::flat: return launch_mesh_form<SceneMesh>(view, scm, rptlaunch::render_mesh, rp, grid, stream);
            }
        }
        if (kind == SceneKind::large) return fast ? rptlaunch_fast::render_large(scl, false, rp, grid, stream) : rptlaunch::render_large(scl, media, rp, grid, stream);
        if (has_sdf) return fast ? rptlaunch_fast::render_sdf(scs, false, rp, grid, stream, kc) : rptlaunch::render_sdf(scs, media, rp, grid, stream, kc);
        if (rp.compact && !nested) return fast ? rptlaunch_fast::render_compact(scs, false, rp, grid, stream, kc) : rptlaunch::render_compact(scs, media, rp, grid, stream, kc);
        return fast ? rptlaunch_fast::render_small(scs, false, nested, rp, grid, stream, kc) : rptlaunch::render_small(scs, media, nested, rp, grid, stream, kc);
    };

    // Dispatch (kernel_common.h): this device's launches of `nblocks` tiles run most expensive tile first, as measured by the previous
    // one, and in units of one tile x one chunk of the samples.
    // Kernels without units: nested loops, the compacting kernel of small scenes.
    const bool unit_kernel = !nested && !rp.compact;
    const SchedLayout lay{(size_t)nblocks};
    bool reorder = false;
    DispatchPolicy pol = policy_of(ctx);
    // workgroup slots of the device: 5 workgroups per CU (__launch_bounds__(256, 5))
    static const int n_cu = []() { int dev = 0, n = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
    const uint32_t slots = pol.unit_slots ? pol.unit_slots : (uint32_t)n_cu * 5u;
    // The compacting kernel of one-sample launches below three rounds of workgroups stays bottom rows first: most expensive first
    // costs 8 % at the reference's 800x600 window (1.5 rounds; 0.081 -> 0.088 ms) and gains 2 % at 1920x1080 (6.4 rounds).
    if (!unit_kernel && nblocks < 3ull * slots) pol.cost_order = 0u;
    if (!nested && (pol.cost_order != 0u || unit_kernel)) {
        RPT_CHECK_RC(sched_for(ctx, d, (uint32_t)nblocks, width, rp.rows_local, tile_rows, rank, world, stream));
        if (d.sched_used && d.sched_stream != stream) RPT_HIP_CHECK(ctx, hipStreamWaitEvent(stream, d.sched_done, 0));
        if (pol.cost_order != 0u) {
            d.sched_launches += 1;
            reorder = spp >= kOrderAlwaysFromSpp || (d.sched_launches & (d.sched_launches - 1u)) == 0u;
            rp.tile_order = d.sched + lay.order();
            rp.tile_cost = reorder ? d.sched + lay.cost() : nullptr;
            rp.tile_start = (reorder && knobs().dispatch_timeline) ? d.sched + lay.start() : nullptr;
        }
        rp.sched_sync = d.sched + lay.sync();
    }

    const uint32_t max_chunk = rptlaunch::max_spp_per_launch(has_sdf);
    if (unit_kernel) {
        // ONE launch whatever spp is: the LDS tables of the state-machine kernels hold a chunk's samples, and a launch is as many
        // chunks as it takes.
        uint32_t n_chunks = unit_chunks(pol, nblocks, spp, slots);
        uint32_t chunk_spp = (spp + n_chunks - 1u) / n_chunks;
        if (chunk_spp > max_chunk) chunk_spp = max_chunk;
        n_chunks = (spp + chunk_spp - 1u) / chunk_spp;
        if (nblocks * n_chunks > 0x7FFFFFFFull) { set_err(ctx, "render: grid too large (%llu tiles x %u chunks of samples)", (unsigned long long)nblocks, n_chunks); return RPT_ERR_INVALID_ARG; }
        rp.n_chunks = n_chunks;
        rp.chunk_spp = chunk_spp;
        rp.spp = spp;
        rp.frames_done = frames_done;
        if (n_chunks > 1u) RPT_HIP_CHECK(ctx, hipMemsetAsync(d.sched + lay.sync() + kSyncZeroFrom, 0, (32 - kSyncZeroFrom + lay.n) * sizeof(uint32_t), stream));
        RPT_HIP_CHECK(ctx, launch((uint32_t)(nblocks * n_chunks)));
        d.sync_used = d.sync_used || n_chunks > 1u;
    } else
    // Kernels without units: batches beyond what one launch holds are split into consecutive launches (the running mean carries
    // over in the framebuffer).
    for (uint32_t done = 0; done < spp;) {
        const uint32_t chunk = (spp - done > max_chunk) ? max_chunk : (spp - done);
        rp.spp = chunk;
        rp.frames_done = frames_done + done;
        rp.n_chunks = 0u;
        RPT_HIP_CHECK(ctx, launch((uint32_t)nblocks));
        done += chunk;
    }
    if (rp.tile_order || rp.sched_sync) {
        if (reorder && pol.cost_order != 2u)
            RPT_HIP_CHECK(ctx, rptlaunch::sched_order(d.sched + lay.cost(), d.sched + lay.order(), d.sched_tiles, stream));
        RPT_HIP_CHECK(ctx, hipEventRecord(d.sched_done, stream));
        d.sched_stream = stream;
        d.sched_used = true;
    }
    return RPT_OK;
}

// Behind a wait for the device: did a unit of a chunked launch give up waiting for its tile's previous chunk (kernel_common.h,
// unit_begin)?  It cannot happen by construction (the predecessor holds an earlier ticket); if it ever does the image is wrong —
// the unit has poisoned its pixels with NaN — and the caller must know.  The word is cleared once it has been reported.
static int check_handoffs(rpt_ctx* ctx, DevState& d)
{
    if (!d.sync_used) return RPT_OK;
    d.sync_used = false;
    bool any = false;
    for (DevState::SchedEntry& e : d.sched_cache) {
        uint32_t* word = e.buf + SchedLayout{(size_t)e.tiles}.sync() + kSyncTimeoutWord;
        uint32_t timed_out = 0;
        RPT_HIP_CHECK(ctx, hipMemcpy(&timed_out, word, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (timed_out) { any = true; RPT_HIP_CHECK(ctx, hipMemset(word, 0, sizeof(uint32_t))); }
    }
    if (any) {
        set_err(ctx, "render: a workgroup timed out waiting for its tile's previous chunk of samples on device %d; the tile's pixels are NaN", d.device);
        return RPT_ERR_HIP;
    }
    return RPT_OK;
}
static int check_handoffs_all(rpt_ctx* ctx)
{
    DeviceGuard guard(ctx->devs[0].device);
    for (DevState& d : ctx->devs) {
        if (!d.sync_used) continue;
        RPT_HIP_CHECK(ctx, guard.to(d.device));
        RPT_CHECK_RC(check_handoffs(ctx, d));
    }
    return RPT_OK;
}

static int ensure_fb(rpt_ctx* ctx, DevState& d, size_t bytes)
{
    if (bytes > d.fb_bytes) {
        if (d.fb) { RPT_HIP_CHECK(ctx, hipFree(d.fb)); d.fb = nullptr; d.fb_bytes = 0; }
        RPT_HIP_CHECK(ctx, hipMalloc((void**)&d.fb, bytes));
        d.fb_bytes = bytes;
    }
    return RPT_OK;
}

// Page-locks a caller's host buffer for the duration of one call (rpt_render on several devices).  A buffer the caller
// has registered itself stays as it is; any other failure leaves the buffer pageable (the copies then take HIP's
// staging path: correct, less overlap).
struct HostPin {
    void* p = nullptr;
    void lock(void* ptr, size_t bytes)
    {
        const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
        if (e == hipSuccess) p = ptr;
        else (void)hipGetLastError();
    }
    ~HostPin() { if (p) (void)hipHostUnregister(p); }
};

// The library is built with -fvisibility=hidden: what include/rpt.h (and, in the test build, include/rpt_test.h) declares is ALL it exports.
#pragma GCC visibility push(default)
extern "C" {

uint32_t rpt_abi_version(void) { return RPT_ABI_VERSION; }
uint32_t rpt_sizeof_scene_desc(void) { return (uint32_t)sizeof(rpt_scene_desc); }
uint32_t rpt_build_has_test_hooks(void)
{
#ifdef RPT_TEST_HOOKS
    return 1u;
#else
    return 0u;
#endif
}

const char* rpt_last_error(const rpt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

// renderer/src/analytical.rs as data (see include/rpt.h)
int rpt_scene_analytical(rpt_scene_desc* out)
{
    if (!out) return RPT_ERR_INVALID_ARG;
    static rpt_sphere spheres[2];
    static rpt_plane planes[1];
    static rpt_light lights[1];
    static rpt_material mats[3];
    memset(spheres, 0, sizeof(spheres));
    memset(planes, 0, sizeof(planes));
    memset(lights, 0, sizeof(lights));
    memset(mats, 0, sizeof(mats));
    memset(out, 0, sizeof(*out));

    spheres[0] = rpt_sphere{{-1.1f, 0.0f, 0.0f}, 1.0f, 0};           // analytical.rs:41
    spheres[1] = rpt_sphere{{1.1f, 0.0f, 0.0f}, 1.0f, 1};            // analytical.rs:70
    planes[0] = rpt_plane{{0.0f, 1.0f, 0.0f}, {0.0f, -1.0f, 0.0f}, 0.0001f, 2, 0.0f};   // analytical.rs:194-198

    mats[0].mask = RPT_MAT_RGB | RPT_MAT_ROUGHNESS | RPT_MAT_METALLIC;              // analytical.rs:56-58
    mats[0].rgb[0] = mats[0].rgb[1] = mats[0].rgb[2] = 1.0f;
    mats[0].roughness = 0.05f;
    mats[0].metallic = 1.0f;
    mats[1].mask = RPT_MAT_RGB | RPT_MAT_CLEARCOAT | RPT_MAT_CLEARCOAT_GLOSS | RPT_MAT_ROUGHNESS;   // analytical.rs:82-85
    mats[1].rgb[0] = 1.0f; mats[1].rgb[1] = 0.186f; mats[1].rgb[2] = 0.0f;
    mats[1].clearcoat = 1.0f;
    mats[1].clearcoat_gloss = 1.0f;
    mats[1].roughness = 0.1f;
    mats[2].mask = RPT_MAT_ROUGHNESS;                                               // analytical.rs:107-116
    mats[2].roughness = 1.0f;
    mats[2].proc_kind = RPT_PROC_CHECKER_DIR;
    mats[2].proc_params[0] = 0.5f; mats[2].proc_params[1] = 100.0f;
    mats[2].proc_params[2] = 0.25f; mats[2].proc_params[3] = 0.1f;

    lights[0].type = RPT_LIGHT_SPHERICAL;                                           // analytical.rs:15-16
    lights[0].position[0] = 3.0f; lights[0].position[1] = 2.0f; lights[0].position[2] = 2.0f;
    lights[0].emission[0] = lights[0].emission[1] = lights[0].emission[2] = 3.0f;
    lights[0].radius = 1.0f;
    lights[0].area = 4.0f * 3.14159265358979323846f * lights[0].radius * lights[0].radius;   // light.rs:22

    out->abi_version = RPT_ABI_VERSION;
    out->flags = 0;
    out->camera.origin[2] = 3.0f;                                                   // pinhole.rs:16
    out->camera.fov_deg = 80.0f;                                                    // pinhole.rs:23
    out->background.kind = RPT_BG_GRADIENT_Y;                                       // analytical.rs:28-32
    out->background.colour_a[0] = out->background.colour_a[1] = out->background.colour_a[2] = 1.0f;
    out->background.colour_b[0] = 0.5f; out->background.colour_b[1] = 0.7f; out->background.colour_b[2] = 1.0f;
    out->background.gamma = 2.2f;
    out->background.scale = 0.5f;
    out->eps = 0.005f;                                                              // tracer.rs:16
    out->max_depth = 4;                                                             // scene.rs:29
    out->n_spheres = 2; out->spheres = spheres;
    out->n_planes = 1; out->planes = planes;
    out->n_lights = 1; out->lights = lights;
    out->n_materials = 3; out->materials = mats;
    out->n_meshes = 0; out->meshes = nullptr;                         // (the reference's scene has no triangles)
    return RPT_OK;
}

int rpt_create(rpt_ctx** out, int device_id)
{
    if (!out) { set_err(nullptr, "rpt_create: out is NULL"); return RPT_ERR_INVALID_ARG; }
    *out = nullptr;
    rpt_ctx* ctx = new (std::nothrow) rpt_ctx();
    if (!ctx) return RPT_ERR_HIP;
    ctx->devs.resize(1);
    int rc = open_dev(ctx->devs[0], device_id, 0, "rpt_create");
    if (rc != RPT_OK) { delete ctx; return rc; }
    *out = ctx;
    return RPT_OK;
}

int rpt_create_multi(rpt_ctx** out, const int* device_ids, int n_devices)
{
    if (!out) { set_err(nullptr, "rpt_create_multi: out is NULL"); return RPT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) { set_err(nullptr, "rpt_create_multi: need 1..64 device ids"); return RPT_ERR_INVALID_ARG; }
    // A device may be listed more than once: every entry is a rank with its own stream and its share of the rows, and the
    // kernels of one GPU's ranks run side by side — a progressive render's launches then fill each other's tails (one MI355X, the
    // resident 1920x1080 frame: 11.4 -> 12.0 Gsamples/s with the device listed twice; 3840x270: 7.6 -> 9.3).  RCCL needs one device
    // per rank, so such contexts gather with peer copies (on one device: device-to-device copies); RPT_GATHER=p2p asks for that
    // with distinct devices too.
    bool distinct = true;
    for (int i = 0; i < n_devices; ++i)
        for (int j = 0; j < i; ++j) distinct = distinct && device_ids[i] != device_ids[j];
    const bool peer = !distinct || knobs().gather == "p2p";
    rpt_ctx* ctx = new (std::nothrow) rpt_ctx();
    if (!ctx) return RPT_ERR_HIP;
    ctx->devs.resize((size_t)n_devices);
    ctx->world = n_devices;
    ctx->peer_gather = peer;
    ctx->use_comm = !peer;
    for (int i = 0; i < n_devices; ++i) {
        int rc = open_dev(ctx->devs[(size_t)i], device_ids[i], i, "rpt_create_multi");
        if (rc != RPT_OK) { for (DevState& d : ctx->devs) if (d.device >= 0) free_dev(d); delete ctx; return rc; }
    }
    if (ctx->use_comm) {
        RcclApi* api = rccl_api();
        int rc = RPT_OK;
        if (!api) { set_err(nullptr, "rpt_create_multi: cannot load RCCL: %s", rccl_why()); rc = RPT_ERR_RCCL; }
        else {
            std::vector<ncclComm_t> comms((size_t)n_devices, nullptr);
            DeviceGuard guard(device_ids[0]);
            ncclResult_t r = api->CommInitAll(comms.data(), n_devices, device_ids);
            if (r != ncclSuccess) { set_err(nullptr, "rpt_create_multi: ncclCommInitAll failed: %s", api->GetErrorString(r)); rc = RPT_ERR_RCCL; }
            else for (int i = 0; i < n_devices; ++i) ctx->devs[(size_t)i].comm = comms[(size_t)i];
        }
        if (rc != RPT_OK) { for (DevState& d : ctx->devs) free_dev(d); delete ctx; return rc; }
    }
    *out = ctx;
    return RPT_OK;
}

int rpt_comm_unique_id(rpt_unique_id* out)
{
    static_assert(sizeof(rpt_unique_id) == sizeof(ncclUniqueId), "rpt_unique_id carries an ncclUniqueId");
    if (!out) { set_err(nullptr, "rpt_comm_unique_id: out is NULL"); return RPT_ERR_INVALID_ARG; }
    RcclApi* api = rccl_api();
    if (!api) { set_err(nullptr, "rpt_comm_unique_id: cannot load RCCL: %s", rccl_why()); return RPT_ERR_RCCL; }
    ncclUniqueId id;
    ncclResult_t r = api->GetUniqueId(&id);
    if (r != ncclSuccess) { set_err(nullptr, "rpt_comm_unique_id: ncclGetUniqueId failed: %s", api->GetErrorString(r)); return RPT_ERR_RCCL; }
    memcpy(out->bytes, &id, sizeof(id));
    return RPT_OK;
}

int rpt_create_rank(rpt_ctx** out, int device_id, int rank, int world, const rpt_unique_id* id)
{
    if (!out) { set_err(nullptr, "rpt_create_rank: out is NULL"); return RPT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!id || world < 1 || rank < 0 || rank >= world) { set_err(nullptr, "rpt_create_rank: invalid argument (rank %d of %d)", rank, world); return RPT_ERR_INVALID_ARG; }
    RcclApi* api = rccl_api();
    if (!api) { set_err(nullptr, "rpt_create_rank: cannot load RCCL: %s", rccl_why()); return RPT_ERR_RCCL; }
    rpt_ctx* ctx = new (std::nothrow) rpt_ctx();
    if (!ctx) return RPT_ERR_HIP;
    ctx->devs.resize(1);
    ctx->world = world;
    ctx->use_comm = true;
    int rc = open_dev(ctx->devs[0], device_id, rank, "rpt_create_rank");
    if (rc != RPT_OK) { delete ctx; return rc; }
    {
        DeviceGuard guard(device_id);
        ncclUniqueId nid;
        memcpy(&nid, id->bytes, sizeof(nid));
        ncclResult_t r = api->CommInitRank(&ctx->devs[0].comm, world, nid, rank);
        if (r != ncclSuccess) {
            set_err(nullptr, "rpt_create_rank: ncclCommInitRank failed: %s", api->GetErrorString(r));
            free_dev(ctx->devs[0]);
            delete ctx;
            return RPT_ERR_RCCL;
        }
    }
    *out = ctx;
    return RPT_OK;
}

int rpt_world(const rpt_ctx* ctx, int* rank, int* world, int* n_local)
{
    if (!ctx) return RPT_ERR_INVALID_ARG;
    if (rank) *rank = ctx->devs[0].rank;
    if (world) *world = ctx->world;
    if (n_local) *n_local = (int)ctx->devs.size();
    return RPT_OK;
}

int rpt_set_tile_rows(rpt_ctx* ctx, uint32_t tile_rows)
{
    if (!ctx || tile_rows == 0) { set_err(ctx, "rpt_set_tile_rows: invalid argument"); return RPT_ERR_INVALID_ARG; }
    ctx->tile_rows = tile_rows;
    return RPT_OK;
}

int rpt_set_dispatch(rpt_ctx* ctx, uint32_t cost_order, uint32_t unit_rounds, uint32_t unit_min_spp, uint32_t unit_slots)
{
    if (!ctx || cost_order > 2u) { set_err(ctx, "rpt_set_dispatch: invalid argument"); return RPT_ERR_INVALID_ARG; }
    ctx->dispatch[0] = cost_order; ctx->dispatch[1] = unit_rounds; ctx->dispatch[2] = unit_min_spp; ctx->dispatch[3] = unit_slots;
    return RPT_OK;
}

void rpt_destroy(rpt_ctx* ctx)
{
    if (!ctx) return;
    for (DevState& d : ctx->devs) { DeviceGuard guard(d.device); (void)hipStreamSynchronize(d.stream); (void)hipStreamSynchronize(d.comm_stream); }
    free_resident(ctx);
    RcclApi* api = ctx->use_comm ? rccl_api() : nullptr;
    for (DevState& d : ctx->devs) {
        if (d.comm && api) { DeviceGuard guard(d.device); (void)api->CommDestroy(d.comm); d.comm = nullptr; }
        free_dev(d);
    }
    delete ctx;
}

// rpt_upload_scene stages the new scene's tables on every device first (stage_scene: the context is untouched until every device
// has them), then commits (commit_scene).  Staging holds the old and the new tables together for a moment.
static int stage_scene(rpt_ctx* ctx, const SceneImage& img, std::vector<void*>& fresh)
{
    static const char* const kind_name[] = {"", "class map", "large scene", "mesh"};
    fresh.assign(ctx->devs.size(), nullptr);
    if (img.bytes.empty()) return RPT_OK;
    for (size_t i = 0; i < ctx->devs.size(); ++i) {
        DeviceGuard guard(ctx->devs[i].device);
        hipError_t e = guard.status;
        if (e == hipSuccess) e = hipMalloc(&fresh[i], img.bytes.size());
        if (e == hipSuccess) e = hipMemcpy(fresh[i], img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_err(ctx, "rpt_upload_scene: uploading the %s tables to device %d failed: %s", kind_name[(int)img.state.kind], ctx->devs[i].device,
                    hipGetErrorString(e));
            for (size_t k = 0; k <= i; ++k)
                if (fresh[k]) { DeviceGuard g(ctx->devs[k].device); (void)hipFree(fresh[k]); }
            return RPT_ERR_HIP;
        }
    }
    return RPT_OK;
}

// Every device drops its old tables and takes its staged ones; then the context's scene is replaced, and the dispatch order of every
// launch shape is learned again.
static void commit_scene(rpt_ctx* ctx, SceneImage& img, const std::vector<void*>& fresh)
{
    for (size_t i = 0; i < ctx->devs.size(); ++i) {
        DevState& d = ctx->devs[i];
        DeviceGuard guard(d.device);
        if (d.tables) {
            (void)hipStreamSynchronize(d.stream);                   // a running launch may still read the old tables
            (void)hipFree(d.tables);                                // (and hipFree waits for the device: launches on other streams)
        }
        free_mesh_work(d);                                          // (written by rpt_update_meshes / rpt_rebuild_meshes only, which wait for their own work;
                                                                    //  a rebuilt node table is read by launches: the wait above covers it)
        d.tables = fresh[i];
        rpthost::bind_scene(img, static_cast<unsigned char*>(d.tables), d.scene);
        d.sched_launches = 0;
        for (DevState::SchedEntry& e : d.sched_cache) e.launches = 0;
    }
    ctx->scene = img.state;
    ctx->refit = std::move(img.refit);
    ctx->smooth = rpthost::SmoothPlan();                            // every mesh FLAT
    ctx->light = rpthost::LightPlan();                              // every mesh OFF
    ctx->tex = rpthost::TexPlan();                                  // every mesh untextured
    ctx->env = rpthost::EnvPlan();                                  // no environment
    ctx->cut = rpthost::CutPlan();                                  // every cutout OFF
    ctx->nrm = rpthost::NrmPlan();                                  // every normal map OFF
    ctx->mmap = rpthost::MmapPlan();                                // every material map OFF
    ctx->emap = rpthost::EmapPlan();                                // every emission map OFF
    ctx->med = rpthost::MedPlan();                                  // no mesh carries a medium
}

int rpt_upload_scene(rpt_ctx* ctx, const rpt_scene_desc* s)
{
    if (!ctx || !s) { set_err(ctx, "rpt_upload_scene: NULL argument"); return RPT_ERR_INVALID_ARG; }
    SceneImage img;
    std::string why;
    const int rc = rpthost::prepare_scene(s, img, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    std::vector<void*> fresh;
    RPT_CHECK_RC(stage_scene(ctx, img, fresh));
    commit_scene(ctx, img, fresh);
    return RPT_OK;
}

// ---- rpt_update_meshes (include/rpt.h, "moving meshes") --------------------------------------------------------------------------
// A runtime failure part-way through an update may leave tables half written: the context drops its scene, on every device.
static void drop_scene(rpt_ctx* ctx)
{
    for (DevState& d : ctx->devs) {
        DeviceGuard guard(d.device);
        (void)hipDeviceSynchronize();
        if (d.tables) { (void)hipFree(d.tables); d.tables = nullptr; }
        free_mesh_work(d);
        d.scene = SceneMesh();
    }
    ctx->scene = rpthost::SceneState();
    ctx->refit = rpthost::RefitPlan();
    ctx->smooth = rpthost::SmoothPlan();
    ctx->light = rpthost::LightPlan();
    ctx->tex = rpthost::TexPlan();
    ctx->env = rpthost::EnvPlan();
    ctx->cut = rpthost::CutPlan();
    ctx->nrm = rpthost::NrmPlan();
    ctx->mmap = rpthost::MmapPlan();
    ctx->emap = rpthost::EmapPlan();
    ctx->med = rpthost::MedPlan();
}

// Where the named meshes' new positions come from: host arrays (rpt_update_meshes, rpt_rebuild_meshes) or device arrays through a
// transform (their _device forms, checked before: check_positions_device).  The only thing in which the two forms' device work differs.
struct MeshPositions {
    const rpt_mesh_vertices* host = nullptr;
    uint32_t n_host = 0;
    const rpt_mesh_source* dev = nullptr;
    uint32_t n_dev = 0;
    const int* dev_device = nullptr;  // per source: the device that holds it (host_move.h, check_mesh_sources)
};

// `*src`: source `so` where device `d` (the current one) can read it — in place when it lies there, else copied into d's own memory,
// on d's stream.
static int source_on_device(rpt_ctx* ctx, DevState& d, const rpt_mesh_source& so, int so_device, const float** src)
{
    if (so_device == d.device) { *src = so.vertices_dev; return RPT_OK; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (!d.move_stage) RPT_HIP_CHECK(ctx, hipMalloc(&d.move_stage, 12 * (size_t)plan.n_vertices()));
    float* at = static_cast<float*>(d.move_stage) + 3 * (size_t)plan.mesh_first[so.mesh];
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(at, so.vertices_dev, 12 * (size_t)so.n_vertices, hipMemcpyDefault, d.stream));
    *src = at;
    return RPT_OK;
}

// The named meshes' positions into `vertices`, device d's concatenated vertex table, on d's stream.
static int put_positions(rpt_ctx* ctx, DevState& d, const MeshPositions& pos, unsigned char* vertices)
{
    const rpthost::RefitPlan& plan = ctx->refit;
    for (uint32_t u = 0; u < pos.n_host; ++u) {
        if (pos.host[u].n_vertices == 0) continue;
        RPT_HIP_CHECK(ctx, hipMemcpyAsync(vertices + 12 * (size_t)plan.mesh_first[pos.host[u].mesh], pos.host[u].vertices,
                                          12 * (size_t)pos.host[u].n_vertices, hipMemcpyHostToDevice, d.stream));
    }
    for (uint32_t u = 0; u < pos.n_dev; ++u) {
        const rpt_mesh_source& so = pos.dev[u];
        if (so.n_vertices == 0) continue;
        const float* src = nullptr;
        RPT_CHECK_RC(source_on_device(ctx, d, so, pos.dev_device[u], &src));
        RPT_HIP_CHECK(ctx, rptlaunch::move_apply(src, rpthost::move_transform_of(so.transform),
                                                 reinterpret_cast<float*>(vertices) + 3 * (size_t)plan.mesh_first[so.mesh], so.n_vertices, d.stream));
    }
    return RPT_OK;
}

// One device's part of an update: wait for its earlier work, make its refit tables if this is the context's first update, copy the
// named meshes' vertices in, refit every triangle row and slot box, then the nodes level by level, deepest first (kernel boundaries
// on one stream order the levels), and wait.
// Device d's refit tables, if it has none yet (no update, rebuild or rpt_set_mesh_shading since the upload): the plan's staging, on
// d's stream.  What the context's first update does, and rpt_set_mesh_shading before it: shading reads the positions and slot_vertex.
static int ensure_refit(rpt_ctx* ctx, DevState& d)
{
    if (d.refit) return RPT_OK;
    const rpthost::RefitPlan& plan = ctx->refit;
    const rpthost::RefitLayout lay(plan.n_vertices(), plan.n_slots, plan.n_nodes);
    RPT_HIP_CHECK(ctx, hipMalloc(&d.refit, lay.total));
    unsigned char* base = static_cast<unsigned char*>(d.refit);
    if (!plan.vertices.empty()) RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + lay.off_vertices, plan.vertices.data(), sizeof(float) * plan.vertices.size(), hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + lay.off_slot_vertex, plan.slot_vertex.data(), sizeof(uint32_t) * plan.slot_vertex.size(), hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + lay.off_level_nodes, plan.level_nodes.data(), sizeof(uint32_t) * plan.level_nodes.size(), hipMemcpyHostToDevice, d.stream));
    return RPT_OK;
}

// The normals of every SMOOTH mesh from the positions device d holds, on d's stream (k_smooth.hip: one launch pair); nothing while
// every mesh is FLAT.  The last device work of every call that moves a mesh, and of rpt_set_mesh_shading.
static int smooth_normals_device(rpt_ctx* ctx, DevState& d)
{
    if (!d.smooth) return RPT_OK;
    const rpthost::SmoothPlan& sp = ctx->smooth;
    const rpthost::SmoothLayout sl = sp.layout();
    unsigned char* base = static_cast<unsigned char*>(d.smooth);
    RPT_HIP_CHECK(ctx, rptlaunch::smooth_normals(static_cast<const float*>(d.refit), reinterpret_cast<const uint32_t*>(base + sl.off_face_vertex),
                                                 reinterpret_cast<float4*>(base + sl.off_face), sp.n_faces, reinterpret_cast<const uint32_t*>(base + sl.off_adj_first),
                                                 reinterpret_cast<const uint32_t*>(base + sl.off_adj), reinterpret_cast<float4*>(base + sl.off_normals), sp.n_vertices,
                                                 d.stream));
    return RPT_OK;
}

// The tables of every ON mesh from the positions device d holds, on d's stream (k_light.hip: five launches); nothing while every
// mesh is OFF.  Beside smooth_normals_device in every call that moves a mesh, and the last device work of rpt_set_mesh_lights.
static int light_tables_device(rpt_ctx* ctx, DevState& d)
{
    if (!d.light) return RPT_OK;
    RPT_HIP_CHECK(ctx, rptlaunch::light_tables(static_cast<const float*>(d.refit), rptargs::light_tables_of(mesh_view_of(ctx, d)), d.stream));
    return RPT_OK;
}

static int update_device(rpt_ctx* ctx, DevState& d, const MeshPositions& pos)
{
    const rpthost::RefitPlan& plan = ctx->refit;
    const rpthost::RefitLayout lay(plan.n_vertices(), plan.n_slots, plan.n_nodes);
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    unsigned char* base = static_cast<unsigned char*>(d.refit);
    RPT_CHECK_RC(put_positions(ctx, d, pos, base + lay.off_vertices));
    float4* tris = const_cast<float4*>(d.scene.tris);
    float4* nodes = const_cast<float4*>(d.scene.nodes);
    const float* slot_box = reinterpret_cast<const float*>(base + lay.off_slot_box);
    const uint32_t* level_nodes = reinterpret_cast<const uint32_t*>(base + lay.off_level_nodes);
    RPT_HIP_CHECK(ctx, rptlaunch::refit_triangles(reinterpret_cast<const float*>(base + lay.off_vertices), reinterpret_cast<const uint32_t*>(base + lay.off_slot_vertex),
                                                  tris, reinterpret_cast<float*>(base + lay.off_slot_box), plan.n_slots, d.stream));
    for (uint32_t level = plan.n_levels(); level-- > 0;)
        RPT_HIP_CHECK(ctx, rptlaunch::refit_nodes(nodes, slot_box, level_nodes + plan.level_first[level], plan.level_first[level + 1u] - plan.level_first[level], d.stream));
    RPT_CHECK_RC(smooth_normals_device(ctx, d));
    RPT_CHECK_RC(light_tables_device(ctx, d));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

// Every device's update_device with checked positions, then the host's record: what rpt_update_meshes and rpt_update_meshes_device share.
static int run_update(rpt_ctx* ctx, const MeshPositions& pos, const std::vector<float>& max_abs, const char* call)
{
    {
        DeviceGuard guard(ctx->devs[0].device);
        int rc_dev = RPT_OK;
        for (DevState& d : ctx->devs) {
            if (guard.to(d.device) != hipSuccess) { set_err(ctx, "%s: cannot select device %d", call, d.device); rc_dev = RPT_ERR_HIP; }
            else rc_dev = update_device(ctx, d, pos);
            if (rc_dev != RPT_OK) break;
        }
        if (rc_dev != RPT_OK) {
            const std::string first = ctx->err;
            drop_scene(ctx);
            set_err(ctx, "%s; the context now holds no scene", first.c_str());
            return rc_dev;
        }
    }
    // every device holds the moved scene: the host's record follows
    ctx->refit.release_staging();
    ctx->refit.mesh_max_abs = max_abs;
    const uint32_t use_bvh = rpthost::refit_use_bvh(max_abs) ? 1u : 0u;
    for (DevState& d : ctx->devs) d.scene.use_bvh = use_bvh;
    return RPT_OK;
}

int rpt_update_meshes(rpt_ctx* ctx, const rpt_mesh_vertices* updates, uint32_t n_updates)
{
    if (!ctx) { set_err(nullptr, "rpt_update_meshes: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (n_updates == 0) return RPT_OK;
    std::vector<float> max_abs;
    std::string why;
    const int rc = rpthost::check_mesh_update(ctx->refit, ctx->scene.kind == SceneKind::mesh, updates, n_updates, max_abs, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    bool any = false;                                               // (meshes without vertices only: nothing moves)
    for (uint32_t u = 0; u < n_updates; ++u) any = any || updates[u].n_vertices != 0;
    if (!any) return RPT_OK;
    MeshPositions pos;
    pos.host = updates; pos.n_host = n_updates;
    return run_update(ctx, pos, max_abs, "rpt_update_meshes");
}

// ---- rpt_rebuild_meshes (include/rpt.h, "rebuilding a moved mesh's hierarchy") -----------------------------------------------------
// One device's part of a rebuild: wait for its earlier work; make the refit tables as a first update does, but with a level order
// that has room for any hierarchy over the scene's triangles (tables an update made are copied into larger ones); make the build's
// tables and the new node table if this is the context's first rebuild; copy the named meshes' vertices in; then, on the device's
// stream, the slots' boxes in the present order, the new order (k_build.hip, build_order), the rows and boxes in the new order, the
// new shape (build_shape).  The host reads the levels' counts back once, launches the refit of the nodes level by level, deepest
// first, and waits.  `levels`: host_build.h's kBuildLevelWords words, as the device left them.
static int rebuild_device(rpt_ctx* ctx, DevState& d, const MeshPositions& pos, uint32_t* levels)
{
    using namespace rpthost;
    const RefitPlan& plan = ctx->refit;
    const uint32_t n = plan.n_slots, max_nodes = build_max_nodes(n);
    const RefitLayout lay(plan.n_vertices(), n, max_nodes);
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    if (!d.refit) {
        RPT_HIP_CHECK(ctx, hipMalloc(&d.refit, lay.total));
        d.refit_full = true;
        unsigned char* base = static_cast<unsigned char*>(d.refit);
        if (!plan.vertices.empty()) RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + lay.off_vertices, plan.vertices.data(), sizeof(float) * plan.vertices.size(), hipMemcpyHostToDevice, d.stream));
        RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + lay.off_slot_vertex, plan.slot_vertex.data(), sizeof(uint32_t) * plan.slot_vertex.size(), hipMemcpyHostToDevice, d.stream));
    } else if (!d.refit_full) {
        void* larger = nullptr;
        RPT_HIP_CHECK(ctx, hipMalloc(&larger, lay.total));
        hipError_t e = hipMemcpyAsync(larger, d.refit, lay.off_slot_box, hipMemcpyDeviceToDevice, d.stream);      // the vertices and the slots' vertex indices
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) (void)hipFree(larger);
        RPT_HIP_CHECK(ctx, e);
        (void)hipFree(d.refit);
        d.refit = larger;
        d.refit_full = true;
    }
    if (!d.build) {
        RPT_HIP_CHECK(ctx, rptlaunch::build_temp_bytes(n, &d.build_temp_bytes));
        const BuildLayout bl(n, max_nodes, build_level_bound(n, kBvhMaxDepth - 1u), d.build_temp_bytes);
        RPT_HIP_CHECK(ctx, hipMalloc(&d.build, bl.total));
    }
    if (!d.build_nodes) RPT_HIP_CHECK(ctx, hipMalloc(&d.build_nodes, sizeof(BvhNode) * (size_t)max_nodes));
    unsigned char* base = static_cast<unsigned char*>(d.refit);
    unsigned char* work = static_cast<unsigned char*>(d.build);
    RPT_CHECK_RC(put_positions(ctx, d, pos, base + lay.off_vertices));
    const BuildLayout bl(n, max_nodes, build_level_bound(n, kBvhMaxDepth - 1u), d.build_temp_bytes);
    rptlaunch::BuildTables t;
    t.n_slots = n; t.max_nodes = max_nodes;
    t.tris = const_cast<float4*>(d.scene.tris);
    t.nodes = static_cast<float4*>(d.build_nodes);
    t.slot_box = reinterpret_cast<const float*>(base + lay.off_slot_box);
    t.slot_vertex = reinterpret_cast<uint32_t*>(base + lay.off_slot_vertex);
    t.level_nodes = reinterpret_cast<uint32_t*>(base + lay.off_level_nodes);
    t.keys_in = reinterpret_cast<uint64_t*>(work + bl.off_keys_in); t.keys_out = reinterpret_cast<uint64_t*>(work + bl.off_keys_out);
    t.vals_in = reinterpret_cast<uint32_t*>(work + bl.off_vals_in); t.vals_out = reinterpret_cast<uint32_t*>(work + bl.off_vals_out);
    t.gather = reinterpret_cast<uint32_t*>(work + bl.off_gather);
    t.range = reinterpret_cast<uint2*>(work + bl.off_range);
    t.mid = reinterpret_cast<uint32_t*>(work + bl.off_mid);
    t.flags = reinterpret_cast<uint32_t*>(work + bl.off_flags); t.offsets = reinterpret_cast<uint32_t*>(work + bl.off_offsets);
    t.levels = reinterpret_cast<uint32_t*>(work + bl.off_levels);
    t.bounds = reinterpret_cast<uint32_t*>(work + bl.off_bounds);
    t.temp = work + bl.off_temp; t.temp_bytes = d.build_temp_bytes;
    const float* vertices = reinterpret_cast<const float*>(base + lay.off_vertices);
    float* slot_box = reinterpret_cast<float*>(base + lay.off_slot_box);
    RPT_HIP_CHECK(ctx, rptlaunch::refit_triangles(vertices, t.slot_vertex, t.tris, slot_box, n, d.stream));
    RPT_HIP_CHECK(ctx, rptlaunch::build_order(t, d.stream));
    RPT_HIP_CHECK(ctx, rptlaunch::refit_triangles(vertices, t.slot_vertex, t.tris, slot_box, n, d.stream));
    const uint32_t leaf = knobs().build_leaf < 1u ? 1u : (knobs().build_leaf > kBvhLeafMax ? kBvhLeafMax : knobs().build_leaf);
    RPT_HIP_CHECK(ctx, rptlaunch::build_shape(t, leaf, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(levels, t.levels, sizeof(uint32_t) * kBuildLevelWords, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    // the table is bound only if it is one the walk can use: at most kBvhMaxDepth levels, each where the last one ended
    uint32_t n_levels = 0, n_nodes = 0;
    bool sound = levels[kBuildStatus] == 0u && levels[kBuildLevelCount] == 1u && levels[kBuildLevelCount + kBvhMaxDepth] == 0u;
    for (uint32_t k = 0; sound && k < kBvhMaxDepth && levels[kBuildLevelCount + k]; ++k) {
        sound = levels[k] == n_nodes && levels[kBuildLevelCount + k] <= max_nodes - n_nodes;
        n_nodes += levels[kBuildLevelCount + k];
        n_levels = k + 1u;
    }
    if (!sound) {
        set_err(ctx, "rpt_rebuild_meshes: the build on device %d did not finish within %u levels (status %u)", d.device, kBvhMaxDepth, levels[kBuildStatus]);
        return RPT_ERR_HIP;
    }
    for (uint32_t level = n_levels; level-- > 0;)
        RPT_HIP_CHECK(ctx, rptlaunch::refit_nodes(t.nodes, t.slot_box, t.level_nodes + levels[level], levels[kBuildLevelCount + level], d.stream));
    RPT_CHECK_RC(smooth_normals_device(ctx, d));
    RPT_CHECK_RC(light_tables_device(ctx, d));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    d.scene.nodes = t.nodes;
    return RPT_OK;
}

// Every device's rebuild_device with checked positions, then the host's record: what rpt_rebuild_meshes and rpt_rebuild_meshes_device share.
static int run_rebuild(rpt_ctx* ctx, const MeshPositions& pos, const std::vector<float>& max_abs, const char* call)
{
    using namespace rpthost;
    uint32_t levels[kBuildLevelWords] = {}, first_levels[kBuildLevelWords] = {};
    const auto t_build = std::chrono::steady_clock::now();
    {
        DeviceGuard guard(ctx->devs[0].device);
        int rc_dev = RPT_OK;
        for (size_t i = 0; i < ctx->devs.size(); ++i) {
            DevState& d = ctx->devs[i];
            if (guard.to(d.device) != hipSuccess) { set_err(ctx, "%s: cannot select device %d", call, d.device); rc_dev = RPT_ERR_HIP; }
            else rc_dev = rebuild_device(ctx, d, pos, levels);
            if (rc_dev == RPT_OK && i == 0) memcpy(first_levels, levels, sizeof(levels));
            if (rc_dev == RPT_OK && memcmp(first_levels, levels, sizeof(levels)) != 0) {
                set_err(ctx, "%s: device %d built another hierarchy than device %d", call, d.device, ctx->devs[0].device);
                rc_dev = RPT_ERR_HIP;
            }
            if (rc_dev != RPT_OK) break;
        }
        if (rc_dev != RPT_OK) {
            const std::string first = ctx->err;
            drop_scene(ctx);
            set_err(ctx, "%s; the context now holds no scene", first.c_str());
            return rc_dev;
        }
    }
    // every device holds the rebuilt scene: the host's record follows
    RefitPlan& plan = ctx->refit;
    plan.release_staging();
    plan.mesh_max_abs = max_abs;
    plan.level_first.clear();
    plan.n_nodes = 0;
    for (uint32_t k = 0; k < kBvhMaxDepth && levels[kBuildLevelCount + k]; ++k) {
        plan.level_first.push_back(levels[k]);
        plan.n_nodes += levels[kBuildLevelCount + k];
    }
    plan.level_first.push_back(plan.n_nodes);
    ctx->scene.mesh_nodes = plan.n_nodes;
    ctx->scene.mesh_depth = plan.n_levels();                        // (breadth-first: the deepest level's children are leaves)
    ctx->scene.mesh_build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_build).count();
    const uint32_t use_bvh = refit_use_bvh(max_abs) ? 1u : 0u;
    for (DevState& d : ctx->devs) d.scene.use_bvh = use_bvh;
    return RPT_OK;
}

int rpt_rebuild_meshes(rpt_ctx* ctx, const rpt_mesh_vertices* updates, uint32_t n_updates)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_rebuild_meshes: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<float> max_abs;
    if (n_updates == 0) {                                           // a rebuild over the positions the context holds
        if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_rebuild_meshes: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
        if (!ctx->refit.ok) { set_err(ctx, "rpt_rebuild_meshes: the scene's meshes hold 2^32 vertices or more"); return RPT_ERR_UNSUPPORTED; }
        max_abs = ctx->refit.mesh_max_abs;
    } else {
        std::string why;
        const int rc = check_mesh_update(ctx->refit, ctx->scene.kind == SceneKind::mesh, updates, n_updates, max_abs, why);
        if (rc != RPT_OK) {
            const std::string theirs = "rpt_update_meshes: ";       // (host_refit.h, update_error: the checks are an update's, the call is this one)
            if (why.compare(0, theirs.size(), theirs) == 0) why = "rpt_rebuild_meshes: " + why.substr(theirs.size());
            set_err(ctx, "%s", why.c_str());
            return rc;
        }
    }
    MeshPositions pos;
    pos.host = updates; pos.n_host = n_updates;
    return run_rebuild(ctx, pos, max_abs, "rpt_rebuild_meshes");
}

// ---- rpt_update_meshes_device / rpt_rebuild_meshes_device (include/rpt.h, "moving meshes from device memory") ----------------------
// host_move.h's MoveSourceQuery: device memory is what hipPointerGetAttributes reports as hipMemoryTypeDevice, and nothing else; and
// `bytes` from `p` on must lie inside the allocation `p` points into (hipMemGetAddressRange), so that no kernel reads beyond it
static int query_source(const void* p, size_t bytes, int* device)
{
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return rpthost::kMoveSourceNotDevice; }
    if (attr.type != hipMemoryTypeDevice || attr.isManaged) return rpthost::kMoveSourceNotDevice;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) == hipSuccess) {
        const uintptr_t at = reinterpret_cast<uintptr_t>(p), lo = reinterpret_cast<uintptr_t>(base);
        if (at < lo || at - lo > size || size - (at - lo) < bytes) return rpthost::kMoveSourceShort;
    } else (void)hipGetLastError();                                 // (memory whose range the runtime does not report: the extent is the caller's word)
    *device = attr.device;
    return rpthost::kMoveSourceOk;
}

// The device check of a call whose host checks have passed, on the context's first device (the current one): its check tables if this
// is the context's first device-source call, the words zeroed, one check launch per source, the words read back.  Nothing the
// context's scene consists of is written.  RPT_OK: `max_abs` has the named meshes' new values.
static int check_positions_device(rpt_ctx* ctx, const rpt_mesh_source* sources, uint32_t n_sources, const int* devices, const char* call,
                                  std::vector<float>& max_abs)
{
    using namespace rpthost;
    DevState& d = ctx->devs[0];
    const RefitPlan& plan = ctx->refit;
    const MoveLayout ml(plan.n_meshes(), plan.n_vertices());
    if (!d.move) {
        void* fresh = nullptr;
        RPT_HIP_CHECK(ctx, hipMalloc(&fresh, ml.total));
        hipError_t e = plan.referenced.empty() ? hipSuccess
                                               : hipMemcpy(static_cast<unsigned char*>(fresh) + ml.off_referenced, plan.referenced.data(), plan.referenced.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(fresh);
        RPT_HIP_CHECK(ctx, e);
        d.move = fresh;
    }
    unsigned char* base = static_cast<unsigned char*>(d.move);
    uint32_t* words = reinterpret_cast<uint32_t*>(base + ml.off_words);
    const size_t word_bytes = sizeof(uint32_t) * kMoveWords * plan.n_meshes();
    RPT_HIP_CHECK(ctx, hipMemsetAsync(words, 0, word_bytes, d.stream));
    for (uint32_t u = 0; u < n_sources; ++u) {
        const rpt_mesh_source& so = sources[u];
        if (so.n_vertices == 0) continue;
        const float* src = nullptr;
        RPT_CHECK_RC(source_on_device(ctx, d, so, devices[u], &src));
        RPT_HIP_CHECK(ctx, rptlaunch::move_check(src, move_transform_of(so.transform), base + ml.off_referenced + plan.mesh_first[so.mesh],
                                                 words + kMoveWords * (size_t)so.mesh, so.n_vertices, d.stream));
    }
    std::vector<uint32_t> got(kMoveWords * (size_t)plan.n_meshes(), 0u);
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(got.data(), words, word_bytes, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    for (uint32_t u = 0; u < n_sources; ++u) {
        const rpt_mesh_source& so = sources[u];
        float big = 0.0f;
        std::string why;
        if (so.n_vertices != 0 && move_check_result(so, &got[kMoveWords * (size_t)so.mesh], call, big, why) != RPT_OK) {
            set_err(ctx, "%s", why.c_str());
            return RPT_ERR_INVALID_ARG;
        }
        max_abs[so.mesh] = big;
    }
    return RPT_OK;
}

static int move_meshes_device(rpt_ctx* ctx, const rpt_mesh_source* sources, uint32_t n_sources, bool rebuild)
{
    const char* call = rebuild ? "rpt_rebuild_meshes_device" : "rpt_update_meshes_device";
    if (!ctx) { set_err(nullptr, "%s: ctx is NULL", call); return RPT_ERR_INVALID_ARG; }
    if (n_sources == 0) {                                           // nothing to do, or a rebuild over the positions the context holds
        if (!rebuild) return RPT_OK;
        if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "%s: needs an uploaded scene with meshes", call); return RPT_ERR_NO_SCENE; }
        if (!ctx->refit.ok) { set_err(ctx, "%s: the scene's meshes hold 2^32 vertices or more", call); return RPT_ERR_UNSUPPORTED; }
        return run_rebuild(ctx, MeshPositions(), ctx->refit.mesh_max_abs, call);
    }
    std::vector<int> devices;
    std::string why;
    const int rc = rpthost::check_mesh_sources(ctx->refit, ctx->scene.kind == SceneKind::mesh, sources, n_sources, query_source, call, devices, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    bool any = false;                                               // (meshes without vertices only: nothing moves)
    for (uint32_t u = 0; u < n_sources; ++u) any = any || sources[u].n_vertices != 0;
    if (!any && !rebuild) return RPT_OK;
    std::vector<float> max_abs = ctx->refit.mesh_max_abs;
    {
        // everything enqueued on a device that holds a source has finished before the source is read; then the check
        DeviceGuard guard(ctx->devs[0].device);
        int rc_dev = RPT_OK;
        for (uint32_t u = 0; u < n_sources && rc_dev == RPT_OK; ++u) {
            bool seen = devices[u] < 0;
            for (uint32_t k = 0; k < u; ++k) seen = seen || devices[k] == devices[u];
            if (seen) continue;
            if (guard.to(devices[u]) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
                (void)hipGetLastError();
                set_err(ctx, "%s: cannot wait for device %d, which holds mesh %u's source", call, devices[u], sources[u].mesh);
                rc_dev = RPT_ERR_HIP;
            }
        }
        if (rc_dev == RPT_OK && guard.to(ctx->devs[0].device) != hipSuccess) { set_err(ctx, "%s: cannot select device %d", call, ctx->devs[0].device); rc_dev = RPT_ERR_HIP; }
        if (rc_dev == RPT_OK) rc_dev = check_positions_device(ctx, sources, n_sources, devices.data(), call, max_abs);
        if (rc_dev == RPT_ERR_HIP) {
            const std::string first = ctx->err;
            drop_scene(ctx);
            set_err(ctx, "%s; the context now holds no scene", first.c_str());
        }
        if (rc_dev != RPT_OK) return rc_dev;
    }
    MeshPositions pos;
    pos.dev = sources; pos.n_dev = n_sources; pos.dev_device = devices.data();
    return rebuild ? run_rebuild(ctx, pos, max_abs, call) : run_update(ctx, pos, max_abs, call);
}

int rpt_update_meshes_device(rpt_ctx* ctx, const rpt_mesh_source* sources, uint32_t n_sources) { return move_meshes_device(ctx, sources, n_sources, false); }
int rpt_rebuild_meshes_device(rpt_ctx* ctx, const rpt_mesh_source* sources, uint32_t n_sources) { return move_meshes_device(ctx, sources, n_sources, true); }

int rpt_download_mesh_vertices(rpt_ctx* ctx, uint32_t mesh, float* vertices, uint32_t n_vertices)
{
    if (!ctx) { set_err(nullptr, "rpt_download_mesh_vertices: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_download_mesh_vertices: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (!plan.ok) { set_err(ctx, "rpt_download_mesh_vertices: the scene's meshes hold 2^32 vertices or more"); return RPT_ERR_UNSUPPORTED; }
    if (mesh >= plan.n_meshes()) { set_err(ctx, "rpt_download_mesh_vertices: mesh %u out of range (the scene has %u)", mesh, plan.n_meshes()); return RPT_ERR_INVALID_ARG; }
    const uint32_t first = plan.mesh_first[mesh], count = plan.mesh_first[mesh + 1u] - first;
    if (n_vertices != count) { set_err(ctx, "rpt_download_mesh_vertices: mesh %u: n_vertices %u != the uploaded mesh's %u", mesh, n_vertices, count); return RPT_ERR_INVALID_ARG; }
    if (count == 0) return RPT_OK;
    if (!vertices) { set_err(ctx, "rpt_download_mesh_vertices: vertices is NULL"); return RPT_ERR_INVALID_ARG; }
    const DevState& d = ctx->devs[0];
    if (!d.refit) {                                                 // no update yet: the upload's positions, still on the host
        memcpy(vertices, &plan.vertices[3 * (size_t)first], 12 * (size_t)count);
        return RPT_OK;
    }
    RPT_ON_DEVICE(ctx);
    const rpthost::RefitLayout lay(plan.n_vertices(), 0, 0);        // (the vertices come first whatever follows them)
    RPT_HIP_CHECK(ctx, hipMemcpy(vertices, static_cast<const unsigned char*>(d.refit) + lay.off_vertices + 12 * (size_t)first, 12 * (size_t)count, hipMemcpyDeviceToHost));
    return RPT_OK;
}

// ---- rpt_set_mesh_shading / rpt_download_mesh_normals (include/rpt.h, "smooth mesh shading") ---------------------------------------
// One device's part: wait for its earlier work (a launch may still read the old tables), make its refit tables if it has none, drop
// the old smooth tables, copy the new ones in, compute the normals, and wait.  ctx->smooth is already the new plan.
static int shade_device(rpt_ctx* ctx, DevState& d)
{
    const rpthost::SmoothPlan& sp = ctx->smooth;
    const rpthost::SmoothLayout sl = sp.layout();
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    if (d.smooth) { (void)hipFree(d.smooth); d.smooth = nullptr; }
    RPT_HIP_CHECK(ctx, hipMalloc(&d.smooth, sl.total));
    unsigned char* base = static_cast<unsigned char*>(d.smooth);
    const auto put = [&](size_t off, const std::vector<uint32_t>& v) {
        return v.empty() ? hipSuccess : hipMemcpyAsync(base + off, v.data(), sizeof(uint32_t) * v.size(), hipMemcpyHostToDevice, d.stream);
    };
    RPT_HIP_CHECK(ctx, put(sl.off_face_vertex, sp.face_vertex));
    RPT_HIP_CHECK(ctx, put(sl.off_adj_first, sp.adj_first));
    RPT_HIP_CHECK(ctx, put(sl.off_adj, sp.adj));
    RPT_HIP_CHECK(ctx, put(sl.off_bits, sp.bits));
    RPT_CHECK_RC(smooth_normals_device(ctx, d));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

// The flattened triangles' corners, read back from the context's first device (the current one): its refit tables' slot_vertex and
// the rows' index words say which slot holds which triangle, whatever updates and rebuilds have done since the upload.
static int read_flat_indices(rpt_ctx* ctx, std::vector<uint32_t>& flat, const char* who = "rpt_set_mesh_shading")
{
    DevState& d = ctx->devs[0];
    const rpthost::RefitPlan& plan = ctx->refit;
    const size_t n = plan.n_slots;
    const rpthost::RefitLayout rl(plan.n_vertices(), 0, 0);
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    std::vector<unsigned char> rows(48 * n);
    std::vector<uint32_t> slot_vertex(3 * n);
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(rows.data(), d.scene.tris, rows.size(), hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(slot_vertex.data(), static_cast<const unsigned char*>(d.refit) + rl.off_slot_vertex, 12 * n, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    if (!rpthost::smooth_flat_indices(rows.data(), slot_vertex.data(), n, flat)) {
        set_err(ctx, "%s: the triangle table of device %d does not name every triangle once", who, d.device);
        return RPT_ERR_HIP;
    }
    for (uint32_t x : flat)
        if (x >= plan.n_vertices()) { set_err(ctx, "%s: device %d's slot_vertex table names a vertex out of range", who, d.device); return RPT_ERR_HIP; }
    return RPT_OK;
}

int rpt_set_mesh_shading(rpt_ctx* ctx, const rpt_mesh_shading* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_shading: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<uint8_t> mode;
    std::string why;
    const int rc = check_mesh_shading(ctx->refit, ctx->scene.kind == SceneKind::mesh, items, n_items, ctx->smooth.mode, mode, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    if (n_items == 0) return RPT_OK;
    SmoothPlan fresh;
    fresh.mode = mode;
    DeviceGuard guard(ctx->devs[0].device);
    int rc_dev = guard.status == hipSuccess ? RPT_OK : RPT_ERR_HIP;
    if (rc_dev != RPT_OK) set_err(ctx, "rpt_set_mesh_shading: cannot select device %d", ctx->devs[0].device);
    if (rc_dev == RPT_OK && !fresh.any()) {                         // every mesh FLAT (again): the context is what it was before the first call
        for (DevState& d : ctx->devs) {
            if (!d.smooth) continue;
            if (guard.to(d.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {      // a launch may still read the tables
                set_err(ctx, "rpt_set_mesh_shading: cannot wait for device %d", d.device);
                rc_dev = RPT_ERR_HIP;
                break;
            }
            (void)hipFree(d.smooth);
            d.smooth = nullptr;
        }
        if (rc_dev == RPT_OK) { ctx->smooth = SmoothPlan(); return RPT_OK; }
    }
    if (rc_dev == RPT_OK) {
        std::vector<uint32_t> flat;
        rc_dev = read_flat_indices(ctx, flat);
        if (rc_dev == RPT_OK) {
            build_smooth_plan(ctx->refit, flat.data(), mode, fresh);
            ctx->smooth = std::move(fresh);
        }
    }
    for (size_t i = 0; rc_dev == RPT_OK && i < ctx->devs.size(); ++i) {
        DevState& d = ctx->devs[i];
        if (guard.to(d.device) != hipSuccess) { set_err(ctx, "rpt_set_mesh_shading: cannot select device %d", d.device); rc_dev = RPT_ERR_HIP; }
        else rc_dev = shade_device(ctx, d);
    }
    if (rc_dev != RPT_OK) {
        const std::string first = ctx->err;
        drop_scene(ctx);
        set_err(ctx, "%s; the context now holds no scene", first.c_str());
        return rc_dev;
    }
    ctx->refit.release_staging();                                   // every device holds the refit tables
    ctx->smooth.release_staging();
    return RPT_OK;
}

int rpt_download_mesh_normals(rpt_ctx* ctx, uint32_t mesh, float* normals, uint32_t n_vertices)
{
    if (!ctx) { set_err(nullptr, "rpt_download_mesh_normals: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_download_mesh_normals: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (!plan.ok) { set_err(ctx, "rpt_download_mesh_normals: the scene's meshes hold 2^32 vertices or more"); return RPT_ERR_UNSUPPORTED; }
    if (mesh >= plan.n_meshes()) { set_err(ctx, "rpt_download_mesh_normals: mesh %u out of range (the scene has %u)", mesh, plan.n_meshes()); return RPT_ERR_INVALID_ARG; }
    const uint32_t first = plan.mesh_first[mesh], count = plan.mesh_first[mesh + 1u] - first;
    if (n_vertices != count) { set_err(ctx, "rpt_download_mesh_normals: mesh %u: n_vertices %u != the uploaded mesh's %u", mesh, n_vertices, count); return RPT_ERR_INVALID_ARG; }
    const DevState& d = ctx->devs[0];
    if (!ctx->smooth.smooth(mesh) || !d.smooth) { set_err(ctx, "rpt_download_mesh_normals: mesh %u is FLAT: the context holds no normals for it (rpt_set_mesh_shading)", mesh); return RPT_ERR_INVALID_ARG; }
    if (count == 0) return RPT_OK;
    if (!normals) { set_err(ctx, "rpt_download_mesh_normals: normals is NULL"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    const rpthost::SmoothPlan& sp = ctx->smooth;
    const rpthost::SmoothLayout sl = sp.layout();
    std::vector<float> rows(4 * (size_t)count);
    RPT_HIP_CHECK(ctx, hipMemcpy(rows.data(), static_cast<const unsigned char*>(d.smooth) + sl.off_normals + 16 * (size_t)first, 16 * (size_t)count, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < count; ++v) memcpy(normals + 3 * v, &rows[4 * v], 12);
    return RPT_OK;
}

// A descriptor table written at `off` of a device's map tables.  The device is idle (the caller waited).
static int put_desc(rpt_ctx* ctx, void* tables, size_t off, const std::vector<uint32_t>& desc)
{
    if (!desc.empty()) RPT_HIP_CHECK(ctx, hipMemcpy(static_cast<unsigned char*>(tables) + off, desc.data(), 4 * desc.size(), hipMemcpyHostToDevice));
    return RPT_OK;
}

// The descriptors of device d's cutouts, normal maps, material maps and emission maps again, by the texture ordinals and wraps of
// ctx->tex (host_cut.h, cut_desc_table; host_map.h, map_desc_table): after a texture call, and inside the feature's own setter.  The
// masks and the texels stay where they are.  The emission maps have a second table by light ordinal (host_emap.h,
// emap_light_desc_table), so theirs are written after a light call too.
static int cut_desc_device(rpt_ctx* ctx, DevState& d) { return put_desc(ctx, d.cut, ctx->cut.layout().off_desc, rpthost::cut_desc_table(ctx->cut, ctx->tex)); }
static int nrm_desc_device(rpt_ctx* ctx, DevState& d) { return put_desc(ctx, d.nrm, ctx->nrm.layout().off_desc, rpthost::nrm_desc_table(ctx->nrm, ctx->tex)); }
static int mmap_desc_device(rpt_ctx* ctx, DevState& d) { return put_desc(ctx, d.mmap, ctx->mmap.layout().off_desc, rpthost::mmap_desc_table(ctx->mmap, ctx->tex)); }
static int emap_desc_device(rpt_ctx* ctx, DevState& d)
{
    const rpthost::EmapLayout el = ctx->emap.layout();
    RPT_CHECK_RC(put_desc(ctx, d.emap, el.off_desc, rpthost::emap_desc_table(ctx->emap, ctx->tex)));
    return put_desc(ctx, d.emap, el.off_light_desc, rpthost::emap_light_desc_table(ctx->emap, ctx->tex, ctx->light));
}

// ---- rpt_set_mesh_lights / rpt_download_mesh_light_table (include/rpt.h, "mesh lights") --------------------------------------------
// One device's part: wait for its earlier work (a launch may still read the old tables), make its refit tables if it has none, drop
// the old light tables, copy the new ones in, compute the ON meshes' tables, and wait.  ctx->light is already the new plan.
static int light_device(rpt_ctx* ctx, DevState& d)
{
    const rpthost::LightPlan& lp = ctx->light;
    const rpthost::LightLayout ll = lp.layout();
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    if (d.light) { (void)hipFree(d.light); d.light = nullptr; }
    RPT_HIP_CHECK(ctx, hipMalloc(&d.light, ll.total));
    unsigned char* base = static_cast<unsigned char*>(d.light);
    const auto put = [&](size_t off, const std::vector<uint32_t>& v) {
        return v.empty() ? hipSuccess : hipMemcpyAsync(base + off, v.data(), sizeof(uint32_t) * v.size(), hipMemcpyHostToDevice, d.stream);
    };
    RPT_HIP_CHECK(ctx, put(ll.off_desc, lp.desc));
    RPT_HIP_CHECK(ctx, put(ll.off_face_vertex, lp.face_vertex));
    RPT_HIP_CHECK(ctx, put(ll.off_face_mesh, lp.face_mesh));
    RPT_HIP_CHECK(ctx, put(ll.off_tri_light, lp.tri_light));
    if (ll.total > ll.off_flat_bits) RPT_HIP_CHECK(ctx, hipMemsetAsync(base + ll.off_flat_bits, 0, ll.total - ll.off_flat_bits, d.stream));
    RPT_CHECK_RC(light_tables_device(ctx, d));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

int rpt_set_mesh_lights(rpt_ctx* ctx, const rpt_mesh_light* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_lights: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<uint8_t> mode;
    std::string why;
    const bool mesh_scene = ctx->scene.kind == SceneKind::mesh;
    const SceneMesh& sc0 = ctx->devs[0].scene;
    const int rc = check_mesh_lights(ctx->refit, mesh_scene, mesh_scene ? sc0.flags : 0u, (mesh_scene ? sc0.n_lights : 0u) + (ctx->env.sampled() ? 1u : 0u), items, n_items, ctx->light.mode, mode, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    for (uint32_t m = 0; m < mode.size(); ++m)                      // include/rpt.h, "mesh cutouts": a cutout mesh cannot be a mesh light
        if (mode[m] == RPT_MESH_LIGHT_ON && ctx->cut.on(m)) {
            set_err(ctx, "rpt_set_mesh_lights: mesh %u has a cutout: next-event estimation would sample points inside holes (rpt_set_mesh_cutouts)", m);
            return RPT_ERR_UNSUPPORTED;
        }
    if (n_items == 0) return RPT_OK;
    LightPlan fresh;
    fresh.mode = mode;
    DeviceGuard guard(ctx->devs[0].device);
    int rc_dev = guard.status == hipSuccess ? RPT_OK : RPT_ERR_HIP;
    if (rc_dev != RPT_OK) set_err(ctx, "rpt_set_mesh_lights: cannot select device %d", ctx->devs[0].device);
    if (rc_dev == RPT_OK && !fresh.any()) {                         // every mesh OFF (again): the context is what it was before the first call
        for (DevState& d : ctx->devs) {
            if (!d.light) continue;
            if (guard.to(d.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {      // a launch may still read the tables
                set_err(ctx, "rpt_set_mesh_lights: cannot wait for device %d", d.device);
                rc_dev = RPT_ERR_HIP;
                break;
            }
            (void)hipFree(d.light);
            d.light = nullptr;
        }
        if (rc_dev == RPT_OK) { ctx->light = LightPlan(); return RPT_OK; }
    }
    if (rc_dev == RPT_OK) {
        std::vector<uint32_t> flat;
        rc_dev = read_flat_indices(ctx, flat, "rpt_set_mesh_lights");
        if (rc_dev == RPT_OK) {
            build_light_plan(ctx->refit, flat.data(), mode, fresh);
            ctx->light = std::move(fresh);
        }
    }
    for (size_t i = 0; rc_dev == RPT_OK && i < ctx->devs.size(); ++i) {
        DevState& d = ctx->devs[i];
        if (guard.to(d.device) != hipSuccess) { set_err(ctx, "rpt_set_mesh_lights: cannot select device %d", d.device); rc_dev = RPT_ERR_HIP; }
        else rc_dev = light_device(ctx, d);
        if (rc_dev == RPT_OK && d.emap && ctx->emap.any()) rc_dev = emap_desc_device(ctx, d);    // the sampler's table goes by light ordinal
    }
    if (rc_dev != RPT_OK) {
        const std::string first = ctx->err;
        drop_scene(ctx);
        set_err(ctx, "%s; the context now holds no scene", first.c_str());
        return rc_dev;
    }
    ctx->refit.release_staging();                                   // every device holds the refit tables
    ctx->light.release_staging();
    return RPT_OK;
}

int rpt_download_mesh_light_table(rpt_ctx* ctx, uint32_t mesh, uint64_t* cdf, uint32_t n_triangles, int32_t* exponent, float* area)
{
    if (!ctx) { set_err(nullptr, "rpt_download_mesh_light_table: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_download_mesh_light_table: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (!plan.ok) { set_err(ctx, "rpt_download_mesh_light_table: the scene's meshes hold 2^32 vertices or more"); return RPT_ERR_UNSUPPORTED; }
    if (mesh >= plan.n_meshes()) { set_err(ctx, "rpt_download_mesh_light_table: mesh %u out of range (the scene has %u)", mesh, plan.n_meshes()); return RPT_ERR_INVALID_ARG; }
    const uint32_t count = plan.tri_first[mesh + 1u] - plan.tri_first[mesh];
    if (n_triangles != count) { set_err(ctx, "rpt_download_mesh_light_table: mesh %u: n_triangles %u != the uploaded mesh's %u", mesh, n_triangles, count); return RPT_ERR_INVALID_ARG; }
    const DevState& d = ctx->devs[0];
    const rpthost::LightPlan& lp = ctx->light;
    const uint32_t ord = lp.ordinal(mesh);
    if (ord == rpthost::kLightNone || !d.light) { set_err(ctx, "rpt_download_mesh_light_table: mesh %u is OFF: the context holds no table for it (rpt_set_mesh_lights)", mesh); return RPT_ERR_INVALID_ARG; }
    if (!exponent || !area || (count && !cdf)) { set_err(ctx, "rpt_download_mesh_light_table: cdf, exponent or area is NULL"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    const rpthost::LightLayout ll = lp.layout();
    const unsigned char* base = static_cast<const unsigned char*>(d.light);
    LightMeshDesc desc;
    RPT_HIP_CHECK(ctx, hipMemcpy(&desc, base + ll.off_desc + sizeof(LightMeshDesc) * (size_t)ord, sizeof(desc), hipMemcpyDeviceToHost));
    if (count) RPT_HIP_CHECK(ctx, hipMemcpy(cdf, base + ll.off_cdf + 8 * (size_t)lp.on_first[ord], 8 * (size_t)count, hipMemcpyDeviceToHost));
    *exponent = desc.exponent;
    *area = desc.area;
    return RPT_OK;
}

// ---- rpt_set_mesh_media / rpt_download_mesh_medium (include/rpt.h, "mesh media") ---------------------------------------------------
static int free_tables(rpt_ctx* ctx, DeviceGuard& guard, void* DevState::*slot, const char* call);      // (below)
// One device's part: wait for its earlier work (a launch may still read the old tables), make its refit tables if it has none (the
// media forms read slot_vertex and the vertices), drop the old media tables, fill and copy the new ones in, and wait.  ctx->med is
// already the new plan.
static int med_device(rpt_ctx* ctx, DevState& d)
{
    const rpthost::MedPlan& mp = ctx->med;
    const rpthost::MedLayout ml = mp.layout();
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    if (d.med) { (void)hipFree(d.med); d.med = nullptr; }
    RPT_HIP_CHECK(ctx, hipMalloc(&d.med, ml.total));
    unsigned char* base = static_cast<unsigned char*>(d.med);
    RPT_HIP_CHECK(ctx, hipMemsetAsync(base, 0, ml.total, d.stream));
    for (const rpthost::MapFill& f : ml.emap.fills())
        if (f.bytes && f.value) RPT_HIP_CHECK(ctx, hipMemsetAsync(base + ml.off_emap + f.off, f.value, f.bytes, d.stream));
    const auto put = [&](size_t off, const std::vector<uint32_t>& v) {
        return v.empty() ? hipSuccess : hipMemcpyAsync(base + off, v.data(), sizeof(uint32_t) * v.size(), hipMemcpyHostToDevice, d.stream);
    };
    RPT_HIP_CHECK(ctx, put(ml.off_rows, mp.rows));
    RPT_HIP_CHECK(ctx, put(ml.off_tri_medium, mp.tri_medium));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

int rpt_set_mesh_media(rpt_ctx* ctx, const rpt_mesh_medium* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_media: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<MedEntry> medium;
    std::string why;
    const int rc = check_mesh_media(ctx->refit, ctx->scene.kind == SceneKind::mesh, items, n_items, ctx->med.medium, medium, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    if (n_items == 0) return RPT_OK;
    MedPlan fresh;
    build_med_plan(ctx->refit, std::move(medium), fresh);
    DeviceGuard guard(ctx->devs[0].device);
    int rc_dev = guard.status == hipSuccess ? RPT_OK : RPT_ERR_HIP;
    if (rc_dev != RPT_OK) set_err(ctx, "rpt_set_mesh_media: cannot select device %d", ctx->devs[0].device);
    if (rc_dev == RPT_OK && !fresh.any()) {                         // no mesh carries a medium (again): the context is what it was before the first call
        rc_dev = free_tables(ctx, guard, &DevState::med, "rpt_set_mesh_media");
        if (rc_dev == RPT_OK) { ctx->med = MedPlan(); return RPT_OK; }
    }
    if (rc_dev == RPT_OK) ctx->med = std::move(fresh);
    for (size_t i = 0; rc_dev == RPT_OK && i < ctx->devs.size(); ++i) {
        DevState& d = ctx->devs[i];
        if (guard.to(d.device) != hipSuccess) { set_err(ctx, "rpt_set_mesh_media: cannot select device %d", d.device); rc_dev = RPT_ERR_HIP; }
        else rc_dev = med_device(ctx, d);
    }
    if (rc_dev != RPT_OK) {
        const std::string first = ctx->err;
        drop_scene(ctx);
        set_err(ctx, "%s; the context now holds no scene", first.c_str());
        return rc_dev;
    }
    ctx->refit.release_staging();                                   // every device holds the refit tables
    ctx->med.release_staging();
    return RPT_OK;
}

int rpt_download_mesh_medium(rpt_ctx* ctx, uint32_t mesh, rpt_mesh_medium* out)
{
    if (!ctx) { set_err(nullptr, "rpt_download_mesh_medium: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_download_mesh_medium: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (mesh >= plan.n_meshes()) { set_err(ctx, "rpt_download_mesh_medium: mesh %u out of range (the scene has %u)", mesh, plan.n_meshes()); return RPT_ERR_INVALID_ARG; }
    if (!out) { set_err(ctx, "rpt_download_mesh_medium: out is NULL"); return RPT_ERR_INVALID_ARG; }
    rpthost::med_item_of(ctx->med, mesh, *out);
    if (ctx->med.on(mesh) && ctx->devs[0].med) {                    // the row as the first device holds it
        uint32_t ord = 0;
        for (uint32_t j = 0; j < ctx->med.n_media(); ++j) if (ctx->med.on_mesh[j] == mesh) ord = j;
        rpthost::MedRow row;
        RPT_ON_DEVICE(ctx);
        RPT_HIP_CHECK(ctx, hipMemcpy(&row, static_cast<const unsigned char*>(ctx->devs[0].med) + ctx->med.layout().off_rows + sizeof(row) * (size_t)ord, sizeof(row), hipMemcpyDeviceToHost));
        out->medium_type = row.type;
        out->density = row.density;
        out->color[0] = row.color[0]; out->color[1] = row.color[1]; out->color[2] = row.color[2];
        out->anisotropy = row.anisotropy;
    }
    return RPT_OK;
}

// ---- what rpt_set_mesh_textures and the four image-map setters share ----------------------------------------------------------------
// "Every mesh OFF (again)": wait on every device that holds `slot` tables (a launch may still read them) and free them.
static int free_tables(rpt_ctx* ctx, DeviceGuard& guard, void* DevState::*slot, const char* call)
{
    for (DevState& d : ctx->devs) {
        if (!(d.*slot)) continue;
        if (guard.to(d.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            set_err(ctx, "%s: cannot wait for device %d", call, d.device);
            return RPT_ERR_HIP;
        }
        (void)hipFree(d.*slot);
        d.*slot = nullptr;
    }
    return RPT_OK;
}

// A setter failed on some device after it began to change the context: the scene goes, the first message stays.
static int fail_without_scene(rpt_ctx* ctx, int rc)
{
    const std::string first = ctx->err;
    drop_scene(ctx);
    set_err(ctx, "%s; the context now holds no scene", first.c_str());
    return rc;
}

// The four features that read a mesh's texture (its UVs and wrap), in the order rpt_set_mesh_textures visits them.
struct TexReader {
    const char *a_thing, *thing, *call;
    void* DevState::*slot;
    bool (*on)(const rpt_ctx&, uint32_t mesh);
    bool (*any)(const rpt_ctx&);
    int (*desc_device)(rpt_ctx*, DevState&);
};
static const TexReader kTexReaders[4] = {
    {"a cutout", "cutout", "rpt_set_mesh_cutouts", &DevState::cut,
     [](const rpt_ctx& c, uint32_t m) { return c.cut.on(m); }, [](const rpt_ctx& c) { return c.cut.any(); }, cut_desc_device},
    {"a normal map", "normal map", "rpt_set_mesh_normal_maps", &DevState::nrm,
     [](const rpt_ctx& c, uint32_t m) { return c.nrm.on(m); }, [](const rpt_ctx& c) { return c.nrm.any(); }, nrm_desc_device},
    {"a material map", "material map", "rpt_set_mesh_material_maps", &DevState::mmap,
     [](const rpt_ctx& c, uint32_t m) { return c.mmap.on(m); }, [](const rpt_ctx& c) { return c.mmap.any(); }, mmap_desc_device},
    {"an emission map", "emission map", "rpt_set_mesh_emission_maps", &DevState::emap,
     [](const rpt_ctx& c, uint32_t m) { return c.emap.on(m); }, [](const rpt_ctx& c) { return c.emap.any(); }, emap_desc_device},
};

// ---- rpt_set_mesh_textures / rpt_download_mesh_texture (include/rpt.h, "mesh textures") -------------------------------------------
// One device's part: wait for its earlier work (a launch may still read the old tables), make its refit tables if it has none, make
// the new tables, copy the kept meshes' texels over from the old ones on the device, decode the named meshes' images, drop the old
// tables, and wait.  ctx->tex is already the new plan; `old` is the plan the old tables were made by.
static int tex_device(rpt_ctx* ctx, DevState& d, const rpthost::TexPlan& old, const rpt_mesh_texture* items, uint32_t n_items)
{
    const rpthost::TexPlan& tp = ctx->tex;
    const rpthost::TexLayout tl = tp.layout();
    const rpthost::TexLayout ol = old.layout();
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    void* fresh = nullptr;
    void* stage = nullptr;
    RPT_HIP_CHECK(ctx, hipMalloc(&fresh, tl.total));
    // the named images' bytes and one L table each, in one allocation that lives until the decodes have run
    size_t stage_bytes = 0;
    for (uint32_t i = 0; i < n_items; ++i)
        if (items[i].width) stage_bytes += 1024 + (((size_t)items[i].width * items[i].height * 4 + 15) & ~(size_t)15);
    const auto fail = [&](int rc) { (void)hipFree(fresh); if (stage) (void)hipFree(stage); return rc; };
    const auto work = [&]() -> int {
        if (stage_bytes) RPT_HIP_CHECK(ctx, hipMalloc(&stage, stage_bytes));
        unsigned char* base = static_cast<unsigned char*>(fresh);
        const auto put = [&](size_t off, const void* p, size_t bytes) {
            return bytes == 0 ? hipSuccess : hipMemcpyAsync(base + off, p, bytes, hipMemcpyHostToDevice, d.stream);
        };
        RPT_HIP_CHECK(ctx, put(tl.off_desc, tp.desc.data(), 4 * tp.desc.size()));
        RPT_HIP_CHECK(ctx, put(tl.off_tri_tex, tp.tri_tex.data(), 4 * tp.tri_tex.size()));
        RPT_HIP_CHECK(ctx, put(tl.off_uvs, tp.uvs.data(), 4 * tp.uvs.size()));
        if (tl.off_texels > tl.off_flat_bits) RPT_HIP_CHECK(ctx, hipMemsetAsync(base + tl.off_flat_bits, 0, tl.off_texels - tl.off_flat_bits, d.stream));
        std::vector<uint8_t> named(tp.image.size(), 0);
        size_t at = 0;
        for (uint32_t i = 0; i < n_items; ++i) {
            const rpt_mesh_texture& it = items[i];
            named[it.mesh] = 1;
            if (!it.width) continue;
            const rpthost::TexImage& im = tp.image[it.mesh];
            const size_t n = (size_t)im.width * im.height;
            unsigned char* at_dev = static_cast<unsigned char*>(stage) + at;
            RPT_HIP_CHECK(ctx, hipMemcpyAsync(at_dev + 1024, it.texels, 4 * n, hipMemcpyHostToDevice, d.stream));
            RPT_HIP_CHECK(ctx, rptlaunch::tex_decode(at_dev + 1024, reinterpret_cast<float*>(at_dev),
                                                     reinterpret_cast<rpthost::TexTexel*>(base + tl.off_texels) + im.first, (uint32_t)n, im.gamma, d.stream));
            at += 1024 + ((4 * n + 15) & ~(size_t)15);
        }
        for (uint32_t m = 0; m < tp.image.size(); ++m) {
            if (named[m] || !tp.image[m].width) continue;           // a mesh not named keeps its texture: the decoded texels move on the device
            if (!d.tex || !old.textured(m)) { set_err(ctx, "rpt_set_mesh_textures: device %d holds no texels for mesh %u", d.device, m); return RPT_ERR_HIP; }
            const size_t n = (size_t)tp.image[m].width * tp.image[m].height;
            RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + tl.off_texels + 16 * (size_t)tp.image[m].first,
                                              static_cast<const unsigned char*>(d.tex) + ol.off_texels + 16 * (size_t)old.image[m].first, 16 * n,
                                              hipMemcpyDeviceToDevice, d.stream));
        }
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
        return RPT_OK;
    };
    const int rc = work();
    if (rc != RPT_OK) return fail(rc);
    if (stage) (void)hipFree(stage);
    if (d.tex) (void)hipFree(d.tex);
    d.tex = fresh;
    return RPT_OK;
}

int rpt_set_mesh_textures(rpt_ctx* ctx, const rpt_mesh_texture* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_textures: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<TexImage> image;
    std::string why;
    const int rc = check_mesh_textures(ctx->refit, ctx->scene.kind == SceneKind::mesh, items, n_items, ctx->tex.image, image, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    for (const TexReader& r : kTexReaders)                          // include/rpt.h, "mesh cutouts" and the maps: each reads the texture's UVs and wrap
        for (uint32_t m = 0; m < image.size(); ++m)
            if (image[m].width == 0u && r.on(*ctx, m)) {
                set_err(ctx, "rpt_set_mesh_textures: mesh %u has %s, which reads its texture's UVs and wrap: remove the %s first (%s)", m, r.a_thing, r.thing, r.call);
                return RPT_ERR_INVALID_ARG;
            }
    if (n_items == 0) return RPT_OK;
    bool any = false;
    for (const TexImage& im : image) any = any || im.width != 0u;
    DeviceGuard guard(ctx->devs[0].device);
    int rc_dev = guard.status == hipSuccess ? RPT_OK : RPT_ERR_HIP;
    if (rc_dev != RPT_OK) set_err(ctx, "rpt_set_mesh_textures: cannot select device %d", ctx->devs[0].device);
    if (rc_dev == RPT_OK && !any) {                                 // no mesh textured (again): the context is what it was before the first call
        rc_dev = free_tables(ctx, guard, &DevState::tex, "rpt_set_mesh_textures");
        if (rc_dev == RPT_OK) { ctx->tex = TexPlan(); return RPT_OK; }
    }
    TexPlan old;
    if (rc_dev == RPT_OK) {
        std::vector<float> uvs = ctx->tex.uvs;
        tex_merge_uvs(ctx->refit, items, n_items, uvs);
        old = std::move(ctx->tex);
        build_tex_plan(ctx->refit, std::move(image), std::move(uvs), ctx->tex);
    }
    for (size_t i = 0; rc_dev == RPT_OK && i < ctx->devs.size(); ++i) {
        DevState& d = ctx->devs[i];
        if (guard.to(d.device) != hipSuccess) { set_err(ctx, "rpt_set_mesh_textures: cannot select device %d", d.device); rc_dev = RPT_ERR_HIP; }
        else rc_dev = tex_device(ctx, d, old, items, n_items);
        for (const TexReader& r : kTexReaders)                      // the ordinals or a wrap may have changed
            if (rc_dev == RPT_OK && d.*r.slot && r.any(*ctx)) rc_dev = r.desc_device(ctx, d);
    }
    if (rc_dev != RPT_OK) return fail_without_scene(ctx, rc_dev);
    ctx->refit.release_staging();                                   // every device holds the refit tables
    ctx->tex.release_staging();
    return RPT_OK;
}

int rpt_download_mesh_texture(rpt_ctx* ctx, uint32_t mesh, float* texels, uint32_t width, uint32_t height)
{
    if (!ctx) { set_err(nullptr, "rpt_download_mesh_texture: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_download_mesh_texture: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (!plan.ok) { set_err(ctx, "rpt_download_mesh_texture: the scene's meshes hold 2^32 vertices or more"); return RPT_ERR_UNSUPPORTED; }
    if (mesh >= plan.n_meshes()) { set_err(ctx, "rpt_download_mesh_texture: mesh %u out of range (the scene has %u)", mesh, plan.n_meshes()); return RPT_ERR_INVALID_ARG; }
    const DevState& d = ctx->devs[0];
    const rpthost::TexPlan& tp = ctx->tex;
    if (!tp.textured(mesh) || !d.tex) { set_err(ctx, "rpt_download_mesh_texture: mesh %u is untextured: the context holds no texels for it (rpt_set_mesh_textures)", mesh); return RPT_ERR_INVALID_ARG; }
    const rpthost::TexImage& im = tp.image[mesh];
    if (width != im.width || height != im.height) { set_err(ctx, "rpt_download_mesh_texture: mesh %u: %u x %u is not its texture's %u x %u", mesh, width, height, im.width, im.height); return RPT_ERR_INVALID_ARG; }
    if (!texels) { set_err(ctx, "rpt_download_mesh_texture: texels is NULL"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    const rpthost::TexLayout tl = tp.layout();
    RPT_HIP_CHECK(ctx, hipMemcpy(texels, static_cast<const unsigned char*>(d.tex) + tl.off_texels + 16 * (size_t)im.first, 16 * (size_t)im.width * im.height, hipMemcpyDeviceToHost));
    return RPT_OK;
}

// ---- rpt_set_environment / rpt_download_environment_table (include/rpt.h, "environment lighting") ---------------------------------
// One device's part: wait for its earlier work (a launch may still read the old tables), make its refit tables if it has none, make
// the new tables and the empty ones, copy the image in, run the table kernels, read Q and W_max back, drop the old tables.  `ep` is
// the new plan (ctx->env still the old one); *q and *w_max: what this device computed.
static int env_device(rpt_ctx* ctx, DevState& d, const rpthost::EnvPlan& ep, const float* texels, uint64_t* q, uint32_t* w_max)
{
    const rpthost::EnvLayout el = ep.layout();
    const size_t n = ep.n_texels();
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    void* fresh = nullptr;
    void* stage = nullptr;
    const auto fail = [&](int rc) { if (fresh) (void)hipFree(fresh); if (stage) (void)hipFree(stage); return rc; };
    const auto work = [&]() -> int {
        RPT_HIP_CHECK(ctx, hipMalloc(&fresh, el.total));
        RPT_HIP_CHECK(ctx, hipMalloc(&stage, 12 * n));
        unsigned char* base = static_cast<unsigned char*>(fresh);
        RPT_HIP_CHECK(ctx, hipMemcpyAsync(stage, texels, 12 * n, hipMemcpyHostToDevice, d.stream));
        RPT_HIP_CHECK(ctx, hipMemsetAsync(base + el.off_head, 0, 16, d.stream));
        if (el.off_flat_bits > el.off_none) RPT_HIP_CHECK(ctx, hipMemsetAsync(base + el.off_none, 0xFF, el.off_flat_bits - el.off_none, d.stream));
        if (el.total > el.off_flat_bits) RPT_HIP_CHECK(ctx, hipMemsetAsync(base + el.off_flat_bits, 0, el.total - el.off_flat_bits, d.stream));
        EnvTables t{};
        t.raw = static_cast<const float*>(stage);
        t.texels = reinterpret_cast<rpthost::EnvTexel*>(base + el.off_texels);
        t.cdf = reinterpret_cast<uint64_t*>(base + el.off_cdf);
        t.block = reinterpret_cast<uint64_t*>(base + el.off_block);
        t.w_max = reinterpret_cast<uint32_t*>(base + el.off_head);
        t.n_texels = (uint32_t)n;
        t.sampled = ep.sampled() ? 1u : 0u;
        RPT_HIP_CHECK(ctx, rptlaunch::env_tables(t, d.stream));
        *q = 0;
        *w_max = 0u;
        if (ep.sampled()) {
            RPT_HIP_CHECK(ctx, hipMemcpyAsync(q, base + el.off_cdf + 8 * (n - 1), 8, hipMemcpyDeviceToHost, d.stream));
            RPT_HIP_CHECK(ctx, hipMemcpyAsync(w_max, base + el.off_head, 4, hipMemcpyDeviceToHost, d.stream));
        }
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
        return RPT_OK;
    };
    const int rc = work();
    if (rc != RPT_OK) return fail(rc);
    (void)hipFree(stage);
    if (d.env) (void)hipFree(d.env);
    d.env = fresh;
    return RPT_OK;
}

int rpt_set_environment(rpt_ctx* ctx, const rpt_environment* env)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_environment: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::string why;
    const bool mesh_scene = ctx->scene.kind == SceneKind::mesh;
    const uint64_t n_other = mesh_scene ? (uint64_t)ctx->devs[0].scene.n_lights + ctx->light.n_on() : 0u;
    const int rc = check_environment(mesh_scene, n_other, env, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    if (!ctx->refit.ok) { set_err(ctx, "rpt_set_environment: the scene's meshes hold 2^32 vertices or more"); return RPT_ERR_UNSUPPORTED; }
    if (!env && !ctx->env.any()) return RPT_OK;
    DeviceGuard guard(ctx->devs[0].device);
    int rc_dev = guard.status == hipSuccess ? RPT_OK : RPT_ERR_HIP;
    if (rc_dev != RPT_OK) set_err(ctx, "rpt_set_environment: cannot select device %d", ctx->devs[0].device);
    if (rc_dev == RPT_OK && !env) {                                 // removed: the context is what it was before the first call
        for (DevState& d : ctx->devs) {
            if (!d.env) continue;
            if (guard.to(d.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {      // a launch may still read the tables
                set_err(ctx, "rpt_set_environment: cannot wait for device %d", d.device);
                rc_dev = RPT_ERR_HIP;
                break;
            }
            (void)hipFree(d.env);
            d.env = nullptr;
        }
        if (rc_dev == RPT_OK) { ctx->env = EnvPlan(); return RPT_OK; }
    }
    EnvPlan fresh;
    if (rc_dev == RPT_OK) {
        fresh.size = env->size;
        fresh.mode = env->mode;
        fresh.scale = env->scale;
        fresh.n_tris = ctx->refit.n_slots;
    }
    for (size_t i = 0; rc_dev == RPT_OK && i < ctx->devs.size(); ++i) {
        DevState& d = ctx->devs[i];
        uint64_t q = 0;
        uint32_t w_max = 0;
        if (guard.to(d.device) != hipSuccess) { set_err(ctx, "rpt_set_environment: cannot select device %d", d.device); rc_dev = RPT_ERR_HIP; }
        else rc_dev = env_device(ctx, d, fresh, env->texels, &q, &w_max);
        if (rc_dev != RPT_OK) break;
        float wm;
        memcpy(&wm, &w_max, 4);
        if (i == 0) {
            fresh.q_total = q;
            fresh.exponent = q ? env_exponent(wm) : 0;
        } else if (q != fresh.q_total) {                            // integer sums: every device has the same bits
            set_err(ctx, "rpt_set_environment: device %d computed another table than device %d", d.device, ctx->devs[0].device);
            rc_dev = RPT_ERR_HIP;
        }
    }
    if (rc_dev != RPT_OK) {
        const std::string first = ctx->err;
        drop_scene(ctx);
        set_err(ctx, "%s; the context now holds no scene", first.c_str());
        return rc_dev;
    }
    ctx->env = fresh;
    ctx->refit.release_staging();                                   // every device holds the refit tables
    return RPT_OK;
}

int rpt_download_environment_table(rpt_ctx* ctx, uint64_t* cdf, uint32_t n_texels, int32_t* exponent)
{
    if (!ctx) { set_err(nullptr, "rpt_download_environment_table: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_download_environment_table: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const rpthost::EnvPlan& ep = ctx->env;
    const DevState& d = ctx->devs[0];
    if (!ep.sampled() || !d.env) { set_err(ctx, "rpt_download_environment_table: no RPT_ENV_SAMPLED environment is set: the context holds no table (rpt_set_environment)"); return RPT_ERR_INVALID_ARG; }
    if (n_texels != ep.n_texels()) { set_err(ctx, "rpt_download_environment_table: n_texels %u != the environment's %u x %u", n_texels, ep.size, ep.size); return RPT_ERR_INVALID_ARG; }
    if (!cdf || !exponent) { set_err(ctx, "rpt_download_environment_table: cdf or exponent is NULL"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    const rpthost::EnvLayout el = ep.layout();                      // (SAMPLED: checked above)
    RPT_HIP_CHECK(ctx, hipMemcpy(cdf, static_cast<const unsigned char*>(d.env) + el.off_cdf, 8 * (size_t)n_texels, hipMemcpyDeviceToHost));
    *exponent = ep.exponent;
    return RPT_OK;
}

// ---- the image-map setters: rpt_set_mesh_cutouts, rpt_set_mesh_normal_maps, rpt_set_mesh_material_maps, rpt_set_mesh_emission_maps --
// (include/rpt.h, "mesh cutouts", "mesh normal maps", "mesh material maps", "mesh emission maps").  One path: what a feature adds is
// its MapFeature, its plan and its decode launch.
struct MapFeature {
    void* DevState::*slot;            // its tables on a device
    const char* call;                 // "rpt_set_mesh_normal_maps"
    const char* holds;                // what a table holds per mesh, for a message: "texels", "mask"
    rpthost::MapConsts k;             // host_map.h
    int (*desc_device)(rpt_ctx*, DevState&);
};

extern "C++" {                        // (templates)
// One device's part: wait for its earlier work (a launch may still read the old tables), make the new tables, stage and decode the
// named meshes' images, copy the kept meshes' over from the old tables on the device, wait, drop the old tables and write the
// descriptors: host_map.h's recipe, walked.  `now` is already the context's plan; `old` is the plan the old tables were made by.
// decode(mesh, staged, dst, n, stream) launches the feature's kernel over the n staged texels of `mesh`.  (The refit's tables are
// there: the meshes are textured.)
template <class Plan, class Decode>
static int map_device(rpt_ctx* ctx, DevState& d, const MapFeature& f, const Plan& now, const Plan& old, const std::vector<rpthost::MapNamed>& named, Decode decode)
{
    const auto nl = now.layout();
    const auto ol = old.layout();
    void*& tables = d.*f.slot;
    const rpthost::MapRecipe r = rpthost::map_recipe(now.slots(), old.slots(), tables != nullptr, named, f.k);
    if (r.missing != rpthost::kMapNoMesh) { set_err(ctx, "%s: device %d holds no %s for mesh %u", f.call, d.device, f.holds, r.missing); return RPT_ERR_HIP; }
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_CHECK_RC(ensure_refit(ctx, d));
    void* fresh = nullptr;
    void* stage = nullptr;                                          // the named images' bytes, in one allocation that lives until the decodes have run
    RPT_HIP_CHECK(ctx, hipMalloc(&fresh, nl.total));
    const auto fail = [&](int rc) { (void)hipFree(fresh); if (stage) (void)hipFree(stage); return rc; };
    const auto work = [&]() -> int {
        if (r.stage_bytes) RPT_HIP_CHECK(ctx, hipMalloc(&stage, r.stage_bytes));
        unsigned char* base = static_cast<unsigned char*>(fresh);
        unsigned char* elems = base + nl.off_elems();
        for (const rpthost::MapFill& fl : nl.fills())
            if (fl.bytes) RPT_HIP_CHECK(ctx, hipMemsetAsync(base + fl.off, fl.value, fl.bytes, d.stream));
        for (const rpthost::MapRecipe::Item& it : r.items) {
            unsigned char* staged = static_cast<unsigned char*>(stage) + it.stage;
            RPT_HIP_CHECK(ctx, hipMemcpyAsync(staged + f.k.prefix, named[it.index].src, f.k.src_bytes * (size_t)it.count, hipMemcpyHostToDevice, d.stream));
            RPT_HIP_CHECK(ctx, decode(named[it.index].mesh, staged, elems + f.k.elem_bytes * (size_t)it.dst, (uint32_t)it.count, d.stream));
        }
        for (const rpthost::MapRecipe::Keep& kp : r.keeps)         // a mesh not named keeps its image: it moves on the device
            RPT_HIP_CHECK(ctx, hipMemcpyAsync(elems + f.k.elem_bytes * (size_t)kp.dst,
                                              static_cast<const unsigned char*>(tables) + ol.off_elems() + f.k.elem_bytes * (size_t)kp.src, kp.bytes,
                                              hipMemcpyDeviceToDevice, d.stream));
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
        return RPT_OK;
    };
    const int rc = work();
    if (rc != RPT_OK) return fail(rc);
    if (stage) (void)hipFree(stage);
    if (tables) (void)hipFree(tables);
    tables = fresh;
    return f.desc_device(ctx, d);
}

// A setter after its checks: `entries` is what they made of the items, `plan` the context's, `build` the feature's build_*_plan.
template <class Plan, class Entry, class Decode>
static int set_mesh_maps(rpt_ctx* ctx, const MapFeature& f, Plan& plan, std::vector<Entry> entries, void (*build)(const rpthost::RefitPlan&, std::vector<Entry>, Plan&),
                         const std::vector<rpthost::MapNamed>& named, Decode decode)
{
    if (named.empty()) return RPT_OK;
    bool any = false;
    for (const Entry& c : entries) any = any || c.width != 0u;
    if (!any && !plan.any()) return RPT_OK;                         // every map OFF, as before
    DeviceGuard guard(ctx->devs[0].device);
    int rc_dev = guard.status == hipSuccess ? RPT_OK : RPT_ERR_HIP;
    if (rc_dev != RPT_OK) set_err(ctx, "%s: cannot select device %d", f.call, ctx->devs[0].device);
    if (rc_dev == RPT_OK && !any) {                                 // every map OFF (again): the context is what it was before the first call
        rc_dev = free_tables(ctx, guard, f.slot, f.call);
        if (rc_dev == RPT_OK) { plan = Plan(); return RPT_OK; }
    }
    Plan old;
    if (rc_dev == RPT_OK) {
        old = std::move(plan);
        build(ctx->refit, std::move(entries), plan);
    }
    for (size_t i = 0; rc_dev == RPT_OK && i < ctx->devs.size(); ++i) {
        DevState& d = ctx->devs[i];
        if (guard.to(d.device) != hipSuccess) { set_err(ctx, "%s: cannot select device %d", f.call, d.device); rc_dev = RPT_ERR_HIP; }
        else rc_dev = map_device(ctx, d, f, plan, old, named, decode);
    }
    return rc_dev == RPT_OK ? RPT_OK : fail_without_scene(ctx, rc_dev);
}

// rpt_download_mesh_normal_map, rpt_download_mesh_material_map and rpt_download_mesh_emission_map: `call` is the entry point's name,
// `thing` "normal map", `setter` "rpt_set_mesh_normal_maps".
template <class Plan>
static int download_map(rpt_ctx* ctx, const char* call, const char* thing, const char* setter, Plan rpt_ctx::*plan_of, void* DevState::*slot, uint32_t mesh,
                        float* texels, uint32_t width, uint32_t height)
{
    if (!ctx) { set_err(nullptr, "%s: ctx is NULL", call); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "%s: needs an uploaded scene with meshes", call); return RPT_ERR_NO_SCENE; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (mesh >= plan.n_meshes()) { set_err(ctx, "%s: mesh %u out of range (the scene has %u)", call, mesh, plan.n_meshes()); return RPT_ERR_INVALID_ARG; }
    const void* tables = ctx->devs[0].*slot;
    const Plan& p = ctx->*plan_of;
    if (!p.on(mesh) || !tables) { set_err(ctx, "%s: mesh %u has no %s: the context holds no texels for it (%s)", call, mesh, thing, setter); return RPT_ERR_INVALID_ARG; }
    const auto& c = p.map[mesh];
    if (width != c.width || height != c.height) { set_err(ctx, "%s: mesh %u: %u x %u is not its map's %u x %u", call, mesh, width, height, c.width, c.height); return RPT_ERR_INVALID_ARG; }
    if (!texels) { set_err(ctx, "%s: texels is NULL", call); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, hipMemcpy(texels, static_cast<const unsigned char*>(tables) + p.layout().off_texels + 16 * (size_t)c.first, 16 * (size_t)c.width * c.height, hipMemcpyDeviceToHost));
    return RPT_OK;
}
}  // extern "C++"

int rpt_set_mesh_cutouts(rpt_ctx* ctx, const rpt_mesh_cutout* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_cutouts: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<CutMask> mask;
    std::string why;
    const int rc = check_mesh_cutouts(ctx->refit, ctx->scene.kind == SceneKind::mesh, ctx->tex, ctx->light, items, n_items, ctx->cut.mask, mask, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    static const MapFeature f = {&DevState::cut, "rpt_set_mesh_cutouts", "mask", {4, 1, 0}, cut_desc_device};
    return set_mesh_maps(ctx, f, ctx->cut, std::move(mask), build_cut_plan, map_named(items, n_items, &rpt_mesh_cutout::alpha),
                         [ctx](uint32_t mesh, unsigned char* staged, unsigned char* dst, uint32_t n, hipStream_t st) {
                             return rptlaunch::cut_mask(staged, reinterpret_cast<uint32_t*>(dst), n, ctx->cut.mask[mesh].threshold, st);
                         });
}

int rpt_download_mesh_cutout(rpt_ctx* ctx, uint32_t mesh, uint32_t* bits, uint32_t n_words)
{
    if (!ctx) { set_err(nullptr, "rpt_download_mesh_cutout: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_download_mesh_cutout: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const rpthost::RefitPlan& plan = ctx->refit;
    if (mesh >= plan.n_meshes()) { set_err(ctx, "rpt_download_mesh_cutout: mesh %u out of range (the scene has %u)", mesh, plan.n_meshes()); return RPT_ERR_INVALID_ARG; }
    const DevState& d = ctx->devs[0];
    const rpthost::CutPlan& cp = ctx->cut;
    if (!cp.on(mesh) || !d.cut) { set_err(ctx, "rpt_download_mesh_cutout: mesh %u has no cutout: the context holds no mask for it (rpt_set_mesh_cutouts)", mesh); return RPT_ERR_INVALID_ARG; }
    const rpthost::CutMask& c = cp.mask[mesh];
    const uint64_t want = ((uint64_t)c.width * c.height + 31u) / 32u;
    if (n_words != want) { set_err(ctx, "rpt_download_mesh_cutout: mesh %u: n_words %u != %llu, the words of its %u x %u mask", mesh, n_words, (unsigned long long)want, c.width, c.height); return RPT_ERR_INVALID_ARG; }
    if (!bits) { set_err(ctx, "rpt_download_mesh_cutout: bits is NULL"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    const rpthost::CutLayout cl = cp.layout();
    RPT_HIP_CHECK(ctx, hipMemcpy(bits, static_cast<const unsigned char*>(d.cut) + cl.off_bits + 4 * (size_t)c.first, 4 * (size_t)n_words, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_set_mesh_normal_maps(rpt_ctx* ctx, const rpt_mesh_normal_map* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_normal_maps: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<NrmMap> map;
    std::string why;
    const int rc = check_mesh_normal_maps(ctx->refit, ctx->scene.kind == SceneKind::mesh, ctx->tex, items, n_items, ctx->nrm.map, map, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    static const MapFeature f = {&DevState::nrm, "rpt_set_mesh_normal_maps", "texels", {16, 4, 0}, nrm_desc_device};
    return set_mesh_maps(ctx, f, ctx->nrm, std::move(map), build_nrm_plan, map_named(items, n_items, &rpt_mesh_normal_map::texels),
                         [ctx](uint32_t mesh, unsigned char* staged, unsigned char* dst, uint32_t n, hipStream_t st) {
                             const NrmMap& c = ctx->nrm.map[mesh];
                             return rptlaunch::nrm_decode(staged, reinterpret_cast<TexTexel*>(dst), n, c.strength, nrm_scale_y(c.strength, c.flags), st);
                         });
}

int rpt_download_mesh_normal_map(rpt_ctx* ctx, uint32_t mesh, float* texels, uint32_t width, uint32_t height)
{
    return download_map(ctx, "rpt_download_mesh_normal_map", "normal map", "rpt_set_mesh_normal_maps", &rpt_ctx::nrm, &DevState::nrm, mesh, texels, width, height);
}

int rpt_set_mesh_material_maps(rpt_ctx* ctx, const rpt_mesh_material_map* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_material_maps: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<MmapMap> map;
    std::string why;
    const int rc = check_mesh_material_maps(ctx->refit, ctx->scene.kind == SceneKind::mesh, ctx->tex, items, n_items, ctx->mmap.map, map, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    static const MapFeature f = {&DevState::mmap, "rpt_set_mesh_material_maps", "texels", {16, 4, 0}, mmap_desc_device};
    return set_mesh_maps(ctx, f, ctx->mmap, std::move(map), build_mmap_plan, map_named(items, n_items, &rpt_mesh_material_map::texels),
                         [ctx](uint32_t mesh, unsigned char* staged, unsigned char* dst, uint32_t n, hipStream_t st) {
                             const MmapMap& c = ctx->mmap.map[mesh];
                             return rptlaunch::mmap_decode(staged, reinterpret_cast<TexTexel*>(dst), n, c.roughness_channel, c.metallic_channel, st);
                         });
}

int rpt_download_mesh_material_map(rpt_ctx* ctx, uint32_t mesh, float* texels, uint32_t width, uint32_t height)
{
    return download_map(ctx, "rpt_download_mesh_material_map", "material map", "rpt_set_mesh_material_maps", &rpt_ctx::mmap, &DevState::mmap, mesh, texels, width, height);
}

// The emission maps are decoded by "mesh textures"' own launch, which wants its L table (1024 B) in front of the staged bytes.
int rpt_set_mesh_emission_maps(rpt_ctx* ctx, const rpt_mesh_emission_map* items, uint32_t n_items)
{
    using namespace rpthost;
    if (!ctx) { set_err(nullptr, "rpt_set_mesh_emission_maps: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    std::vector<EmapMap> map;
    std::string why;
    const int rc = check_mesh_emission_maps(ctx->refit, ctx->scene.kind == SceneKind::mesh, ctx->tex, items, n_items, ctx->emap.map, map, why);
    if (rc != RPT_OK) { set_err(ctx, "%s", why.c_str()); return rc; }
    static const MapFeature f = {&DevState::emap, "rpt_set_mesh_emission_maps", "texels", {16, 4, 1024}, emap_desc_device};
    return set_mesh_maps(ctx, f, ctx->emap, std::move(map), build_emap_plan, map_named(items, n_items, &rpt_mesh_emission_map::texels),
                         [ctx](uint32_t mesh, unsigned char* staged, unsigned char* dst, uint32_t n, hipStream_t st) {
                             return rptlaunch::tex_decode(staged + 1024, reinterpret_cast<float*>(staged), reinterpret_cast<TexTexel*>(dst), n, ctx->emap.map[mesh].gamma, st);
                         });
}

int rpt_download_mesh_emission_map(rpt_ctx* ctx, uint32_t mesh, float* texels, uint32_t width, uint32_t height)
{
    return download_map(ctx, "rpt_download_mesh_emission_map", "emission map", "rpt_set_mesh_emission_maps", &rpt_ctx::emap, &DevState::emap, mesh, texels, width, height);
}

uint32_t rpt_tile_row_count(uint32_t height, uint32_t tile_rows, uint32_t rank, uint32_t world)
{
    return tile_row_count(height, tile_rows, rank, world);
}

uint32_t rpt_tile_global_row(uint32_t local_row, uint32_t tile_rows, uint32_t rank, uint32_t world)
{
    if (tile_rows == 0 || world == 0) return 0;
    return tile_global_row(local_row, tile_rows, rank, world);
}

uint32_t rpt_tile_rows_padded(uint32_t height, uint32_t tile_rows, uint32_t world)
{
    if (tile_rows == 0 || world == 0) return 0;
    return rows_padded_for(height, tile_rows, world);
}

int rpt_tile_copy_plan(uint32_t height, uint32_t tile_rows, uint32_t rank, uint32_t world, rpt_tile_plan* out)
{
    return tile_copy_plan(height, tile_rows, rank, world, out);
}

// The launch domain (include/rpt.h, "the launch domain"): the last frame's count, frames_done + spp, fits 64 bits.  One past it the
// blend's frames + 1 wraps to 0, the weight is infinite and the pixel NaN for good.
static bool frames_in_domain(rpt_ctx* ctx, const char* who, uint64_t frames_done, uint32_t spp)
{
    if ((uint64_t)spp <= UINT64_MAX - frames_done) return true;
    set_err(ctx, "%s: frames_done + spp exceeds 2^64 - 1 (frames_done=%llu spp=%u)", who, (unsigned long long)frames_done, spp);
    return false;
}

int rpt_render_device(rpt_ctx* ctx, float* pixels_dev, uint32_t width, uint32_t height, uint64_t frames_done, uint32_t spp,
                      uint64_t seed, uint32_t flags, uint32_t tile_rows, uint32_t rank, uint32_t world, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_render_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind == SceneKind::none) { set_err(ctx, "rpt_render_device: no scene uploaded"); return RPT_ERR_NO_SCENE; }
    if (!pixels_dev || width == 0 || height == 0 || world == 0 || rank >= world || tile_rows == 0) {
        set_err(ctx, "rpt_render_device: invalid argument (pixels=%p width=%u height=%u tile_rows=%u rank=%u world=%u)",
                (void*)pixels_dev, width, height, tile_rows, rank, world);
        return RPT_ERR_INVALID_ARG;
    }
    if ((uint64_t)width * height > 0xFFFFFFFFull) { set_err(ctx, "rpt_render_device: image too large for 32-bit pixel indices"); return RPT_ERR_INVALID_ARG; }
    if (((uintptr_t)pixels_dev & 15u) != 0) { set_err(ctx, "rpt_render_device: pixels must be 16-byte aligned"); return RPT_ERR_INVALID_ARG; }
    if (!frames_in_domain(ctx, "rpt_render_device", frames_done, spp)) return RPT_ERR_INVALID_ARG;
    if (spp == 0) return RPT_OK;
    RPT_ON_DEVICE(ctx);
    return launch_render(ctx, ctx->devs[0], pixels_dev, width, height, frames_done, spp, seed, flags, tile_rows, rank, world, (hipStream_t)stream);
}

int rpt_render(rpt_ctx* ctx, float* pixels, uint32_t width, uint32_t height, uint64_t frames_done, uint32_t spp, uint64_t seed,
               uint32_t flags)
{
    if (!ctx) { set_err(nullptr, "rpt_render: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels || width == 0 || height == 0) { set_err(ctx, "rpt_render: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if ((uint64_t)width * height > 0xFFFFFFFFull) { set_err(ctx, "rpt_render: image too large for 32-bit pixel indices"); return RPT_ERR_INVALID_ARG; }
    if (!frames_in_domain(ctx, "rpt_render", frames_done, spp)) return RPT_ERR_INVALID_ARG;
    if (ctx->scene.kind == SceneKind::none) { set_err(ctx, "rpt_render: no scene uploaded"); return RPT_ERR_NO_SCENE; }
    if ((size_t)ctx->world != ctx->devs.size()) {
        set_err(ctx, "rpt_render: a host ColorBuffer needs every rank in this process (rpt_create / rpt_create_multi); "
                     "with one process per GPU use the resident buffer (rpt_resident_*)");
        return RPT_ERR_UNSUPPORTED;
    }
    // The fan-out of tracer.rs:29-32: every device takes its rows of the caller's buffer (one strided copy each way,
    // each device over its own PCIe link) and all devices render concurrently, driven by one host thread.  Two things make
    // that true on a caller's pageable Vec<f32>: (1) with more than one device the buffer is page-locked for the duration
    // of the call (hipHostRegister), so every copy is a real asynchronous DMA — a copy to or from pageable memory returns
    // only when it is done, i.e. after that device's kernel; (2) the copies back are enqueued in a second pass, after
    // EVERY device has its upload and its launches, so even without the page lock (RPT_PIN_HOST=0, or a registration
    // that fails) no device waits for another one's kernel before it starts.
    DeviceGuard guard(ctx->devs[0].device);
    const uint32_t world = (uint32_t)ctx->world;
    const uint32_t tile_rows = world == 1 ? height : ctx->tile_rows;
    const uint32_t rows_padded = rows_padded_for(height, tile_rows, world);
    HostPin pin;
    if (ctx->devs.size() > 1 && knobs().pin_host) pin.lock(pixels, (size_t)width * height * 16u);
    const auto enqueue = [&]() -> int {
        for (DevState& d : ctx->devs) {
            RPT_HIP_CHECK(ctx, guard.to(d.device));
            int rc = ensure_fb(ctx, d, (size_t)rows_padded * width * 16u);
            if (rc != RPT_OK) return rc;
            RPT_HIP_CHECK(ctx, hipEventRecord(d.ev_begin, d.stream));
            RPT_HIP_CHECK(ctx, copy_rank_rows(true, pixels, d.fb, width, height, tile_rows, (uint32_t)d.rank, world, d.stream));
            rc = launch_render(ctx, d, d.fb, width, height, frames_done, spp, seed, flags, tile_rows, (uint32_t)d.rank, world, d.stream);
            if (rc != RPT_OK) return rc;
            RPT_HIP_CHECK(ctx, hipEventRecord(d.ev_end, d.stream));
        }
        ctx->timed = true;
        for (DevState& d : ctx->devs) {
            RPT_HIP_CHECK(ctx, guard.to(d.device));
            RPT_HIP_CHECK(ctx, copy_rank_rows(false, pixels, d.fb, width, height, tile_rows, (uint32_t)d.rank, world, d.stream));
        }
        return RPT_OK;
    };
    const int rc = enqueue();
    // wait for every device whatever happened: copies already enqueued still use the caller's (page-locked) buffer
    int rc_sync = RPT_OK;
    for (DevState& d : ctx->devs) {
        if (guard.to(d.device) != hipSuccess || hipStreamSynchronize(d.stream) != hipSuccess) {
            if (rc == RPT_OK && rc_sync == RPT_OK) set_err(ctx, "rpt_render: waiting for device %d failed: %s", d.device, hipGetErrorString(hipGetLastError()));
            rc_sync = RPT_ERR_HIP;
        }
    }
    if (rc == RPT_OK && rc_sync == RPT_OK)
        for (DevState& d : ctx->devs) {
            if (guard.to(d.device) != hipSuccess) return RPT_ERR_HIP;
            const int rc_h = check_handoffs(ctx, d);
            if (rc_h != RPT_OK) return rc_h;
        }
    return rc != RPT_OK ? rc : rc_sync;
}

#ifdef RPT_TEST_HOOKS    // include/rpt_test.h: the test build only (librpt_hip_test.so)
// Test / development probe (include/rpt_test.h): device 0's tile costs (4 per tile), dispatch order, development data.
int rpt_debug_sched_read(rpt_ctx* ctx, uint32_t* out, uint32_t capacity_tiles, uint32_t* n_tiles)
{
    if (!ctx || !out || !n_tiles) return RPT_ERR_INVALID_ARG;
    DevState& d = ctx->devs[0];
    *n_tiles = d.sched_tiles;
    if (!d.sched || d.sched_tiles > capacity_tiles) { set_err(ctx, "rpt_debug_sched_read: no launch yet, or %u tiles do not fit", d.sched_tiles); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_HIP_CHECK(ctx, hipMemcpy(out, d.sched, (size_t)d.sched_tiles * 10u * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RPT_OK;
}

// (include/rpt_test.h) the last launch's KernelChoice on device 0
int rpt_debug_kernel_choice(rpt_ctx* ctx, uint32_t* out)
{
    if (!ctx || !out) return RPT_ERR_INVALID_ARG;
    *out = ctx->devs[0].last_choice;
    return RPT_OK;
}

// (include/rpt_test.h) the last launch's mesh form: 0 .. 11 a MeshForm of mesh_args.h, 12 .. 19 a material-mapped one (mesh_args_mmap.h), 20 .. 27 an emission-mapped one (mesh_args_emap.h), 28 .. 35 a media one (mesh_args_med.h)
int rpt_debug_mesh_form(rpt_ctx* ctx, uint32_t* form)
{
    if (!ctx || !form) return RPT_ERR_INVALID_ARG;
    *form = ctx->devs[0].last_form;
    return RPT_OK;
}

// (include/rpt_test.h) read the environment's knobs again
int rpt_debug_reload_knobs(void) { rpthost::reload_knobs(); return RPT_OK; }

// Test probe (include/rpt_test.h): how long before device `a`'s last render ENDED device `b`'s began.
int rpt_debug_render_overlap_ms(rpt_ctx* ctx, int a, int b, float* ms)
{
    if (!ctx || !ms || a < 0 || b < 0 || (size_t)a >= ctx->devs.size() || (size_t)b >= ctx->devs.size()) {
        set_err(ctx, "rpt_debug_render_overlap_ms: invalid argument");
        return RPT_ERR_INVALID_ARG;
    }
    if (!ctx->timed) { set_err(ctx, "rpt_debug_render_overlap_ms: no render yet"); return RPT_ERR_INVALID_ARG; }
    DevState &da = ctx->devs[(size_t)a], &db = ctx->devs[(size_t)b];
    if (da.device != db.device) { set_err(ctx, "rpt_debug_render_overlap_ms: events of two physical devices cannot be compared"); return RPT_ERR_UNSUPPORTED; }
    DeviceGuard guard(da.device);
    RPT_HIP_CHECK(ctx, guard.status);
    RPT_HIP_CHECK(ctx, hipEventSynchronize(da.ev_end));
    RPT_HIP_CHECK(ctx, hipEventSynchronize(db.ev_begin));
    RPT_HIP_CHECK(ctx, hipEventElapsedTime(ms, db.ev_begin, da.ev_end));
    return RPT_OK;
}

#endif  // RPT_TEST_HOOKS

// ---- resident ColorBuffer ------------------------------------------------------------------------------------

int rpt_resident_reset(rpt_ctx* ctx)
{
    if (!ctx) { set_err(nullptr, "rpt_resident_reset: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    for (DevState& d : ctx->devs) {
        DeviceGuard guard(d.device);
        RPT_HIP_CHECK(ctx, guard.status);
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.comm_stream));
    }
    free_resident(ctx);
    return RPT_OK;
}

// whether the resident buffer is one of this size and tiling: resident_begin then keeps it, and its frame counter
static bool resident_matches(const rpt_ctx* ctx, uint32_t width, uint32_t height)
{
    const uint32_t tile_rows = ctx->plain() ? height : ctx->tile_rows;
    return ctx->has_res && ctx->res_w == width && ctx->res_h == height && ctx->res_tile_rows == tile_rows;
}

// ColorBuffer::new(width, height) (buffer.rs:18-26) as per-rank tiles
static int resident_begin(rpt_ctx* ctx, uint32_t width, uint32_t height)
{
    const uint32_t world = (uint32_t)ctx->world;
    const uint32_t tile_rows = ctx->plain() ? height : ctx->tile_rows;
    if (resident_matches(ctx, width, height)) return RPT_OK;
    int rc = rpt_resident_reset(ctx);
    if (rc != RPT_OK) return rc;
    const uint32_t rows_padded = rows_padded_for(height, tile_rows, world);
    const size_t tile_bytes = (size_t)rows_padded * width * 16u;
    DeviceGuard guard(ctx->devs[0].device);
    for (DevState& d : ctx->devs) {
        RPT_HIP_CHECK(ctx, guard.to(d.device));
        RPT_HIP_CHECK(ctx, hipMalloc((void**)&d.tile, tile_bytes));
        RPT_HIP_CHECK(ctx, hipMemsetAsync(d.tile, 0, tile_bytes, d.stream));
    }
    ctx->res_w = width; ctx->res_h = height; ctx->res_tile_rows = tile_rows; ctx->res_rows_padded = rows_padded;
    ctx->res_frames = 0;
    ctx->has_res = true;
    return RPT_OK;
}

int rpt_resident_render(rpt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t seed, uint32_t flags)
{
    if (!ctx) { set_err(nullptr, "rpt_resident_render: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (width == 0 || height == 0) { set_err(ctx, "rpt_resident_render: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if ((uint64_t)width * height > 0xFFFFFFFFull) { set_err(ctx, "rpt_resident_render: image too large for 32-bit pixel indices"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind == SceneKind::none) { set_err(ctx, "rpt_resident_render: no scene uploaded"); return RPT_ERR_NO_SCENE; }
    // against the resident counter, which a buffer of another size starts again from 0; checked before resident_begin touches anything
    if (!frames_in_domain(ctx, "rpt_resident_render", resident_matches(ctx, width, height) ? ctx->res_frames : 0u, spp)) return RPT_ERR_INVALID_ARG;
    int rc = resident_begin(ctx, width, height);
    if (rc != RPT_OK) return rc;
    DeviceGuard guard(ctx->devs[0].device);
    for (DevState& d : ctx->devs) {
        RPT_HIP_CHECK(ctx, guard.to(d.device));
        RPT_HIP_CHECK(ctx, hipEventRecord(d.ev_begin, d.stream));
        rc = launch_render(ctx, d, d.tile, width, height, ctx->res_frames, spp, seed, flags, ctx->res_tile_rows, (uint32_t)d.rank, (uint32_t)ctx->world, d.stream);
        if (rc != RPT_OK) return rc;
        RPT_HIP_CHECK(ctx, hipEventRecord(d.ev_end, d.stream));
    }
    ctx->timed = true;
    ctx->res_frames += spp;                                                      // tracer.rs:121
    return RPT_OK;
}

int rpt_resident_kernel_ms(rpt_ctx* ctx, float* ms)
{
    if (!ctx || !ms) { set_err(ctx, "rpt_resident_kernel_ms: NULL argument"); return RPT_ERR_INVALID_ARG; }
    if (!ctx->timed) { set_err(ctx, "rpt_resident_kernel_ms: no rpt_resident_render yet"); return RPT_ERR_INVALID_ARG; }
    float worst = 0.0f;
    DeviceGuard guard(ctx->devs[0].device);
    for (DevState& d : ctx->devs) {
        RPT_HIP_CHECK(ctx, guard.to(d.device));
        RPT_HIP_CHECK(ctx, hipEventSynchronize(d.ev_end));
        float t = 0.0f;
        RPT_HIP_CHECK(ctx, hipEventElapsedTime(&t, d.ev_begin, d.ev_end));
        worst = t > worst ? t : worst;
    }
    *ms = worst;
    return RPT_OK;
}

int rpt_resident_frames(const rpt_ctx* ctx, uint64_t* frames)
{
    if (!ctx || !frames) return RPT_ERR_INVALID_ARG;
    *frames = ctx->res_frames;
    return RPT_OK;
}

int rpt_resident_upload(rpt_ctx* ctx, const float* pixels, uint32_t width, uint32_t height, uint64_t frames)
{
    if (!ctx) { set_err(nullptr, "rpt_resident_upload: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels || width == 0 || height == 0) { set_err(ctx, "rpt_resident_upload: invalid argument"); return RPT_ERR_INVALID_ARG; }
    int rc = resident_begin(ctx, width, height);
    if (rc != RPT_OK) return rc;
    DeviceGuard guard(ctx->devs[0].device);
    for (DevState& d : ctx->devs) {
        RPT_HIP_CHECK(ctx, guard.to(d.device));
        RPT_HIP_CHECK(ctx, copy_rank_rows(true, const_cast<float*>(pixels), d.tile, width, height, ctx->res_tile_rows, (uint32_t)d.rank, (uint32_t)ctx->world, d.stream));
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));          // the caller may free `pixels` on return
    }
    ctx->res_frames = frames;
    return RPT_OK;
}

// Tiles -> rank-major `gathered` on the root -> top-down image on the root, all enqueued (no host wait), and BESIDE the renders
// that follow: every rank copies its tile into a snapshot on its render stream (a device copy: 16.6 MB for configs[2]'s share,
// ~10 us) and everything else — the RCCL send / receive or the peer copy, the scatter kernel on the root — runs on the rank's
// second stream, `comm_stream`, behind an event.  The next render waits for nothing but that copy; gather k overlaps render k + 1
// and ranks no longer meet at every step (round 4).  The image is complete when the root's comm_stream has drained:
// rpt_resident_sync waits for both streams, the download paths wait for `gather_done` on the device.
// Returns the device pointer of the assembled image in *image_out (root only).
static int gather_to_root(rpt_ctx* ctx, float* image_dst, float** image_out)
{
    const uint32_t w = ctx->res_w, h = ctx->res_h, world = (uint32_t)ctx->world;
    DevState& root = ctx->devs[0];
    DeviceGuard guard(root.device);
    RPT_HIP_CHECK(ctx, guard.status);
    if (ctx->plain()) {                                              // the tile is the image
        if (image_dst && image_dst != root.tile) RPT_HIP_CHECK(ctx, hipMemcpyAsync(image_dst, root.tile, (size_t)w * h * 16u, hipMemcpyDeviceToDevice, root.stream));
        if (image_out) *image_out = image_dst ? image_dst : root.tile;
        return RPT_OK;
    }
    const size_t count = (size_t)ctx->res_rows_padded * w * 4u;      // floats per rank
    if (ctx->is_root()) {
        if (!ctx->gathered) RPT_HIP_CHECK(ctx, hipMalloc((void**)&ctx->gathered, count * 4u * world));
        if (!image_dst && !ctx->image) RPT_HIP_CHECK(ctx, hipMalloc((void**)&ctx->image, (size_t)w * h * 16u));
        if (!ctx->gather_done) RPT_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->gather_done, hipEventDisableTiming));
    }
    // 1. snapshots, on the render streams
    for (DevState& d : ctx->devs) {
        RPT_HIP_CHECK(ctx, guard.to(d.device));
        if (!d.snap) RPT_HIP_CHECK(ctx, hipMalloc((void**)&d.snap, count * 4u));
        if (d.snap_used) RPT_HIP_CHECK(ctx, hipStreamWaitEvent(d.stream, d.snap_free, 0));     // the previous gather still sends from it
        RPT_HIP_CHECK(ctx, hipMemcpyAsync(d.snap, d.tile, count * 4u, hipMemcpyDeviceToDevice, d.stream));
        RPT_HIP_CHECK(ctx, hipEventRecord(d.snap_ready, d.stream));
        RPT_HIP_CHECK(ctx, hipStreamWaitEvent(d.comm_stream, d.snap_ready, 0));
        d.snap_used = true;
    }
    // 2. the exchange, on the comm streams
    if (ctx->peer_gather) {
        // single process: peer copies over xGMI into the root's buffer, each on its source device's comm stream (which is ordered
        // behind the root's previous scatter by `gather_done`: that kernel still reads `gathered`)
        for (DevState& d : ctx->devs) {
            RPT_HIP_CHECK(ctx, guard.to(d.device));
            if (ctx->gather_issued) RPT_HIP_CHECK(ctx, hipStreamWaitEvent(d.comm_stream, ctx->gather_done, 0));
            RPT_HIP_CHECK(ctx, hipMemcpyPeerAsync(ctx->gathered + (size_t)d.rank * count, root.device, d.snap, d.device, count * 4u, d.comm_stream));
            RPT_HIP_CHECK(ctx, hipEventRecord(d.snap_free, d.comm_stream));
        }
        RPT_HIP_CHECK(ctx, guard.to(root.device));
        for (DevState& d : ctx->devs) RPT_HIP_CHECK(ctx, hipStreamWaitEvent(root.comm_stream, d.snap_free, 0));
    } else {
        // RCCL over xGMI: every other rank sends its snapshot to rank 0, which posts one receive per sender; one group, so the 7
        // incoming transfers use 7 links at once.  Rank 0's own tile is a device copy, not a send to itself.
        RcclApi* api = rccl_api();
        if (!api) { set_err(ctx, "gather: cannot load RCCL: %s", rccl_why()); return RPT_ERR_RCCL; }
        RPT_RCCL_CHECK(ctx, api, api->GroupStart());
        // From here to GroupEnd nothing returns: a group left open would swallow every later RCCL call of the process.
        ncclResult_t posted = ncclSuccess;
        const char* what = "";
        for (DevState& d : ctx->devs) {
            if (posted != ncclSuccess) break;
            if (d.rank == 0) {
                for (uint32_t r = 1; r < world && posted == ncclSuccess; ++r) {
                    posted = api->Recv(ctx->gathered + (size_t)r * count, count, ncclFloat, (int)r, d.comm, d.comm_stream);
                    what = "ncclRecv";
                }
            } else {
                posted = api->Send(d.snap, count, ncclFloat, 0, d.comm, d.comm_stream);
                what = "ncclSend";
            }
        }
        const ncclResult_t closed = api->GroupEnd();
        if (posted != ncclSuccess) { set_err(ctx, "gather: %s failed: %s", what, api->GetErrorString(posted)); return RPT_ERR_RCCL; }
        if (closed != ncclSuccess) { set_err(ctx, "gather: ncclGroupEnd failed: %s", api->GetErrorString(closed)); return RPT_ERR_RCCL; }
        if (ctx->is_root()) {
            RPT_HIP_CHECK(ctx, guard.to(root.device));
            RPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->gathered, root.snap, count * 4u, hipMemcpyDeviceToDevice, root.comm_stream));
        }
        for (DevState& d : ctx->devs) {
            RPT_HIP_CHECK(ctx, guard.to(d.device));
            RPT_HIP_CHECK(ctx, hipEventRecord(d.snap_free, d.comm_stream));
        }
    }
    // 3. the scatter into the top-down image, on the root's comm stream
    if (ctx->is_root()) {
        RPT_HIP_CHECK(ctx, guard.to(root.device));
        float* img = image_dst ? image_dst : ctx->image;
        RPT_HIP_CHECK(ctx, rptlaunch::untile(ctx->gathered, img, w, h, ctx->res_tile_rows, world, ctx->res_rows_padded, root.comm_stream));
        RPT_HIP_CHECK(ctx, hipEventRecord(ctx->gather_done, root.comm_stream));
        ctx->gather_issued = true;
        if (image_out) *image_out = img;
    } else if (image_out) *image_out = nullptr;
    return RPT_OK;
}

int rpt_resident_gather_device(rpt_ctx* ctx, float* image_dev)
{
    if (!ctx) { set_err(nullptr, "rpt_resident_gather_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!ctx->has_res) { set_err(ctx, "rpt_resident_gather_device: no resident buffer"); return RPT_ERR_INVALID_ARG; }
    if (((uintptr_t)image_dev & 15u) != 0) { set_err(ctx, "rpt_resident_gather_device: image must be 16-byte aligned"); return RPT_ERR_INVALID_ARG; }
    return gather_to_root(ctx, image_dev, nullptr);
}

int rpt_resident_sync(rpt_ctx* ctx)
{
    if (!ctx) { set_err(nullptr, "rpt_resident_sync: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    DeviceGuard guard(ctx->devs[0].device);
    for (DevState& d : ctx->devs) {
        RPT_HIP_CHECK(ctx, guard.to(d.device));
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.comm_stream));    // (a gather in flight: gather_to_root)
        const int rc = check_handoffs(ctx, d);
        if (rc != RPT_OK) return rc;
    }
    return RPT_OK;
}

int rpt_host_pin(void* buffer, size_t bytes)
{
    if (!buffer || bytes == 0) { set_err(nullptr, "rpt_host_pin: invalid argument"); return RPT_ERR_INVALID_ARG; }
    const hipError_t e = hipHostRegister(buffer, bytes, hipHostRegisterPortable);
    if (e == hipErrorHostMemoryAlreadyRegistered) { (void)hipGetLastError(); return RPT_OK; }
    if (e != hipSuccess) { (void)hipGetLastError(); set_err(nullptr, "rpt_host_pin: hipHostRegister failed: %s", hipGetErrorString(e)); return RPT_ERR_HIP; }
    return RPT_OK;
}

int rpt_host_unpin(void* buffer)
{
    if (!buffer) { set_err(nullptr, "rpt_host_unpin: invalid argument"); return RPT_ERR_INVALID_ARG; }
    const hipError_t e = hipHostUnregister(buffer);
    if (e != hipSuccess) { (void)hipGetLastError(); set_err(nullptr, "rpt_host_unpin: hipHostUnregister failed: %s", hipGetErrorString(e)); return RPT_ERR_HIP; }
    return RPT_OK;
}

// Is `p` page-locked host memory (hipHostMalloc / hipHostRegister)?  Then a copy to it is one DMA.
static bool host_is_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// Device -> the caller's host buffer on the root's stream, then wait.  Page-locked destinations take the copy directly; a
// pageable one goes through the context's page-locked staging buffer (one DMA + one memcpy: the runtime's own staging of
// pageable copies runs at ~7 GB/s on this host, a third of that).
static int download_to_host(rpt_ctx* ctx, void* dst, const void* src_dev, size_t bytes)
{
    DevState& root = ctx->devs[0];
    if (host_is_pinned(dst)) {
        RPT_HIP_CHECK(ctx, hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, root.stream));
        return rpt_resident_sync(ctx);
    }
    if (bytes > ctx->stage_bytes) {
        if (ctx->stage) { RPT_HIP_CHECK(ctx, hipHostFree(ctx->stage)); ctx->stage = nullptr; ctx->stage_bytes = 0; }
        RPT_HIP_CHECK(ctx, hipHostMalloc(&ctx->stage, bytes, hipHostMallocDefault));
        ctx->stage_bytes = bytes;
    }
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->stage, src_dev, bytes, hipMemcpyDeviceToHost, root.stream));
    const int rc = rpt_resident_sync(ctx);
    if (rc != RPT_OK) return rc;
    memcpy(dst, ctx->stage, bytes);
    return RPT_OK;
}

int rpt_resident_download(rpt_ctx* ctx, float* pixels)
{
    if (!ctx) { set_err(nullptr, "rpt_resident_download: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!ctx->has_res || (ctx->is_root() && !pixels)) { set_err(ctx, "rpt_resident_download: no resident buffer or NULL destination"); return RPT_ERR_INVALID_ARG; }
    float* img = nullptr;
    int rc = gather_to_root(ctx, nullptr, &img);
    if (rc != RPT_OK) return rc;
    DevState& root = ctx->devs[0];
    DeviceGuard guard(root.device);
    if (ctx->is_root() && !ctx->plain()) RPT_HIP_CHECK(ctx, hipStreamWaitEvent(root.stream, ctx->gather_done, 0));   // the image is assembled on the comm stream
    if (ctx->is_root()) return download_to_host(ctx, pixels, img, (size_t)ctx->res_w * ctx->res_h * 16u);
    return rpt_resident_sync(ctx);
}

int rpt_resident_download_u8(rpt_ctx* ctx, uint8_t* frame)
{
    if (!ctx) { set_err(nullptr, "rpt_resident_download_u8: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!ctx->has_res || (ctx->is_root() && !frame)) { set_err(ctx, "rpt_resident_download_u8: no resident buffer or NULL destination"); return RPT_ERR_INVALID_ARG; }
    float* img = nullptr;
    int rc = gather_to_root(ctx, nullptr, &img);
    if (rc != RPT_OK) return rc;
    DevState& root = ctx->devs[0];
    DeviceGuard guard(root.device);
    if (ctx->is_root()) {
        const size_t n = (size_t)ctx->res_w * ctx->res_h;
        if (!ctx->plain()) RPT_HIP_CHECK(ctx, hipStreamWaitEvent(root.stream, ctx->gather_done, 0));
        if (!ctx->frame_u8) RPT_HIP_CHECK(ctx, hipMalloc((void**)&ctx->frame_u8, n * 4u));
        RPT_HIP_CHECK(ctx, rptlaunch::convert_to_u8(img, ctx->frame_u8, n, root.stream));
        return download_to_host(ctx, frame, ctx->frame_u8, n * 4u);
    }
    return rpt_resident_sync(ctx);
}

int rpt_untile_device(rpt_ctx* ctx, const float* gathered_dev, float* image_dev, uint32_t width, uint32_t height,
                      uint32_t tile_rows, uint32_t world, uint32_t rows_padded, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_untile_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!gathered_dev || !image_dev || width == 0 || height == 0 || tile_rows == 0 || world == 0) { set_err(ctx, "rpt_untile_device: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if (rows_padded_for(height, tile_rows, world) > rows_padded) { set_err(ctx, "rpt_untile_device: rows_padded %u too small", rows_padded); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::untile(gathered_dev, image_dev, width, height, tile_rows, world, rows_padded, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_convert_to_u8_device(rpt_ctx* ctx, const float* pixels_dev, uint8_t* out_dev, uint32_t width, uint32_t height, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_convert_to_u8_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels_dev || !out_dev || width == 0 || height == 0) { set_err(ctx, "rpt_convert_to_u8_device: invalid argument"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::convert_to_u8(pixels_dev, out_dev, (uint64_t)width * height, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_convert_to_u8_at_device(rpt_ctx* ctx, const float* pixels_dev, uint32_t width, uint32_t height, uint8_t* frame_dev, uint32_t at_x,
                                uint32_t at_y, uint32_t frame_width, uint32_t frame_height, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_convert_to_u8_at_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels_dev || !frame_dev || width == 0 || height == 0 || frame_width == 0 || frame_height == 0) {
        set_err(ctx, "rpt_convert_to_u8_at_device: invalid argument");
        return RPT_ERR_INVALID_ARG;
    }
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::convert_to_u8_at(pixels_dev, width, height, frame_dev, at_x, at_y, frame_width, frame_height, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_denoise_device(rpt_ctx* ctx, const float* pixels_dev, float* out_dev, uint32_t width, uint32_t height, uint32_t iterations,
                       float edge_k, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_denoise_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    const size_t bytes = (size_t)width * height * 16u;
    if (!pixels_dev || !out_dev || width == 0 || height == 0 || iterations < 1u || iterations > 6u || !(edge_k > 0.0f) || !std::isfinite(edge_k)) {
        set_err(ctx, "rpt_denoise_device: invalid argument (iterations 1..6, edge_k > 0)");
        return RPT_ERR_INVALID_ARG;
    }
    if ((((uintptr_t)pixels_dev | (uintptr_t)out_dev) & 15u) != 0) { set_err(ctx, "rpt_denoise_device: buffers must be 16-byte aligned"); return RPT_ERR_INVALID_ARG; }
    const char *a = (const char*)pixels_dev, *b = (const char*)out_dev;
    if (a < b + bytes && b < a + bytes) { set_err(ctx, "rpt_denoise_device: pixels_dev and out_dev overlap"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    if (iterations > 1u && bytes > d.dn_bytes) {
        if (d.dn) { RPT_HIP_CHECK(ctx, hipStreamSynchronize((hipStream_t)stream)); RPT_HIP_CHECK(ctx, hipFree(d.dn)); d.dn = nullptr; d.dn_bytes = 0; }
        RPT_HIP_CHECK(ctx, hipMalloc((void**)&d.dn, bytes));
        d.dn_bytes = bytes;
    }
    const bool uses_scratch = iterations > 1u;
    if (uses_scratch && d.dn_used && d.dn_stream != (hipStream_t)stream) RPT_HIP_CHECK(ctx, hipStreamWaitEvent((hipStream_t)stream, d.dn_done, 0));
    RPT_HIP_CHECK(ctx, rptlaunch::denoise(pixels_dev, out_dev, d.dn, width, height, iterations, edge_k, (hipStream_t)stream));
    if (uses_scratch) {
        RPT_HIP_CHECK(ctx, hipEventRecord(d.dn_done, (hipStream_t)stream));
        d.dn_stream = (hipStream_t)stream;
        d.dn_used = true;
    }
    return RPT_OK;
}

int rpt_denoise(rpt_ctx* ctx, const float* pixels, float* out, uint32_t width, uint32_t height, uint32_t iterations, float edge_k)
{
    if (!ctx) { set_err(nullptr, "rpt_denoise: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels || !out || width == 0 || height == 0) { set_err(ctx, "rpt_denoise: invalid argument"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const size_t bytes = (size_t)width * height * 16u;
    int rc = ensure_fb(ctx, d, 2u * bytes);                           // input and output, one allocation
    if (rc != RPT_OK) return rc;
    float* out_dev = reinterpret_cast<float*>(reinterpret_cast<char*>(d.fb) + bytes);
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(d.fb, pixels, bytes, hipMemcpyHostToDevice, d.stream));
    rc = rpt_denoise_device(ctx, d.fb, out_dev, width, height, iterations, edge_k, d.stream);
    if (rc != RPT_OK) return rc;
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(out, out_dev, bytes, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

// ---- guided denoiser (include/rpt.h, "guided denoiser") ------------------------------------------------------------------------------
// What the pack checks before anything is enqueued: the NULL context, the pointers (NULL with n > 0; misaligned whatever n is, the
// device form only), the batch size.  False: the call returns *rc.  True: there is something to launch.
static bool guides_ready(rpt_ctx* ctx, const char* name, const void* const* ptrs, uint64_t n, bool aligned, int* rc)
{
    *rc = RPT_ERR_INVALID_ARG;
    if (!ctx) { set_err(nullptr, "%s: ctx is NULL", name); return false; }
    for (uint32_t k = 0; k < 4u; ++k) {
        if (n > 0 && !ptrs[k]) { set_err(ctx, "%s: NULL array with n > 0", name); return false; }
        if (aligned && ((uintptr_t)ptrs[k] & 15u) != 0) { set_err(ctx, "%s: device arrays must be 16-byte aligned", name); return false; }
    }
    if (n / 256u + (n % 256u ? 1u : 0u) > 0x7FFFFFFFull) { set_err(ctx, "%s: %llu records are more than a grid of 0x7FFFFFFF workgroups holds", name, (unsigned long long)n); return false; }
    *rc = RPT_OK;
    return n != 0;
}

int rpt_denoise_guides_device(rpt_ctx* ctx, const rpt_ray* rays_dev, const rpt_hit* hits_dev, const rpt_surface* surfaces_dev, uint64_t n,
                              rpt_guide* guides_dev, void* stream)
{
    int rc;
    const void* const ptrs[4] = {rays_dev, hits_dev, surfaces_dev, guides_dev};
    if (!guides_ready(ctx, "rpt_denoise_guides_device", ptrs, n, true, &rc)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::gdn_pack(rays_dev, hits_dev, surfaces_dev, n, guides_dev, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_denoise_guides(rpt_ctx* ctx, const rpt_ray* rays, const rpt_hit* hits, const rpt_surface* surfaces, uint64_t n, rpt_guide* guides)
{
    int rc;
    const void* const ptrs[4] = {rays, hits, surfaces, guides};
    if (!guides_ready(ctx, "rpt_denoise_guides", ptrs, n, false, &rc)) return rc;
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const auto up = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    const size_t off_hits = up(sizeof(rpt_ray) * (size_t)n);
    const size_t off_surfaces = off_hits + up(sizeof(rpt_hit) * (size_t)n);
    const size_t off_guides = off_surfaces + up(sizeof(rpt_surface) * (size_t)n);
    RPT_CHECK_RC(ensure_fb(ctx, d, off_guides + sizeof(rpt_guide) * (size_t)n));
    unsigned char* base = reinterpret_cast<unsigned char*>(d.fb);
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(base, rays, sizeof(rpt_ray) * (size_t)n, hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + off_hits, hits, sizeof(rpt_hit) * (size_t)n, hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(base + off_surfaces, surfaces, sizeof(rpt_surface) * (size_t)n, hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, rptlaunch::gdn_pack(reinterpret_cast<const rpt_ray*>(base), reinterpret_cast<const rpt_hit*>(base + off_hits),
                                           reinterpret_cast<const rpt_surface*>(base + off_surfaces), n, reinterpret_cast<rpt_guide*>(base + off_guides), d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(guides, base + off_guides, sizeof(rpt_guide) * (size_t)n, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

// The filter's arguments, pointers aside: the ranges of include/rpt.h (a NaN fails every comparison).
static bool guided_args_ok(uint32_t width, uint32_t height, uint32_t iterations, float edge_k, float normal_k, float plane_k, uint32_t flags)
{
    return width != 0 && height != 0 && iterations >= 1u && iterations <= 6u && edge_k > 0.0f && std::isfinite(edge_k) &&
           normal_k >= 0.0f && std::isfinite(normal_k) && plane_k >= 0.0f && std::isfinite(plane_k) && flags == 0u;
}

int rpt_denoise_guided_device(rpt_ctx* ctx, const float* pixels_dev, const rpt_guide* guides_dev, float* out_dev, uint32_t width, uint32_t height,
                              uint32_t iterations, float edge_k, float normal_k, float plane_k, uint32_t flags, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_denoise_guided_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels_dev || !guides_dev || !out_dev || !guided_args_ok(width, height, iterations, edge_k, normal_k, plane_k, flags)) {
        set_err(ctx, "rpt_denoise_guided_device: invalid argument (iterations 1..6, edge_k > 0, normal_k and plane_k >= 0, all finite, flags 0)");
        return RPT_ERR_INVALID_ARG;
    }
    if ((((uintptr_t)pixels_dev | (uintptr_t)guides_dev | (uintptr_t)out_dev) & 15u) != 0) {
        set_err(ctx, "rpt_denoise_guided_device: buffers must be 16-byte aligned");
        return RPT_ERR_INVALID_ARG;
    }
    const size_t bytes = (size_t)width * height * 16u;
    const char *a = (const char*)pixels_dev, *b = (const char*)out_dev, *g = (const char*)guides_dev;
    if ((a < b + bytes && b < a + bytes) || (g < b + bytes && b < g + 4u * bytes)) {
        set_err(ctx, "rpt_denoise_guided_device: out_dev overlaps pixels_dev or guides_dev");
        return RPT_ERR_INVALID_ARG;
    }
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const bool uses_scratch = iterations > 1u;                        // (the context's buffer of rpt_denoise_device, and its rule for streams)
    if (uses_scratch && bytes > d.dn_bytes) {
        if (d.dn) { RPT_HIP_CHECK(ctx, hipStreamSynchronize((hipStream_t)stream)); RPT_HIP_CHECK(ctx, hipFree(d.dn)); d.dn = nullptr; d.dn_bytes = 0; }
        RPT_HIP_CHECK(ctx, hipMalloc((void**)&d.dn, bytes));
        d.dn_bytes = bytes;
    }
    if (uses_scratch && d.dn_used && d.dn_stream != (hipStream_t)stream) RPT_HIP_CHECK(ctx, hipStreamWaitEvent((hipStream_t)stream, d.dn_done, 0));
    RPT_HIP_CHECK(ctx, rptlaunch::gdn_filter(pixels_dev, guides_dev, out_dev, d.dn, width, height, iterations, edge_k, normal_k, plane_k, (hipStream_t)stream));
    if (uses_scratch) {
        RPT_HIP_CHECK(ctx, hipEventRecord(d.dn_done, (hipStream_t)stream));
        d.dn_stream = (hipStream_t)stream;
        d.dn_used = true;
    }
    return RPT_OK;
}

int rpt_denoise_guided(rpt_ctx* ctx, const float* pixels, const rpt_guide* guides, float* out, uint32_t width, uint32_t height, uint32_t iterations,
                       float edge_k, float normal_k, float plane_k, uint32_t flags)
{
    if (!ctx) { set_err(nullptr, "rpt_denoise_guided: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels || !guides || !out || !guided_args_ok(width, height, iterations, edge_k, normal_k, plane_k, flags)) {
        set_err(ctx, "rpt_denoise_guided: invalid argument (iterations 1..6, edge_k > 0, normal_k and plane_k >= 0, all finite, flags 0)");
        return RPT_ERR_INVALID_ARG;
    }
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const size_t bytes = (size_t)width * height * 16u;
    RPT_CHECK_RC(ensure_fb(ctx, d, 6u * bytes));                      // input, output and the guides (64 B a pixel), one allocation
    float* out_dev = reinterpret_cast<float*>(reinterpret_cast<char*>(d.fb) + bytes);
    rpt_guide* guides_dev = reinterpret_cast<rpt_guide*>(reinterpret_cast<char*>(d.fb) + 2u * bytes);
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(d.fb, pixels, bytes, hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(guides_dev, guides, 4u * bytes, hipMemcpyHostToDevice, d.stream));
    RPT_CHECK_RC(rpt_denoise_guided_device(ctx, d.fb, guides_dev, out_dev, width, height, iterations, edge_k, normal_k, plane_k, flags, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(out, out_dev, bytes, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

// ---- temporal accumulation (include/rpt.h, "temporal accumulation") ---------------------------------------------------------------------
// Everything but alignment and overlap: the NULL rules, the ranges (a NaN fails every comparison), the cameras.  NULL: acceptable.
static const char* tacc_args_bad(const void* pixels, const void* guides, const rpt_camera* camera, const void* prev_guides, const void* prev_history,
                                 const rpt_camera* prev_camera, const void* out, const void* history, uint32_t width, uint32_t height, float n_max,
                                 float normal_min, float plane_k, uint32_t flags)
{
    if (!pixels || !guides || !camera || !out || !history) return "pixels, guides, camera, out and history must not be NULL";
    const int prevs = (prev_guides ? 1 : 0) + (prev_history ? 1 : 0) + (prev_camera ? 1 : 0);
    if (prevs != 0 && prevs != 3) return "prev_guides, prev_history and prev_camera must be all NULL (the first frame) or all given";
    if (width == 0 || height == 0 || width > 65535u || height > 65535u) return "width and height must be 1..65535";
    if (!(n_max >= 1.0f) || !std::isfinite(n_max) || !(normal_min >= -1.0f && normal_min <= 1.0f) || !(plane_k >= 0.0f) || !std::isfinite(plane_k) || flags != 0u)
        return "invalid argument (n_max >= 1, -1 <= normal_min <= 1, plane_k >= 0, all finite, flags 0)";
    if (!rpthost::tacc_camera_ok(*camera) || (prev_camera && !rpthost::tacc_camera_ok(*prev_camera))) return "a camera's fields must be finite and origin != center";
    return nullptr;
}

int rpt_temporal_accumulate_device(rpt_ctx* ctx, const float* pixels_dev, const rpt_guide* guides_dev, const rpt_camera* camera, const rpt_guide* prev_guides_dev,
                                   const rpt_history* prev_history_dev, const rpt_camera* prev_camera, const float* prev_positions_dev, float* out_dev,
                                   rpt_history* history_dev, uint32_t width, uint32_t height, float n_max, float normal_min, float plane_k, uint32_t flags,
                                   void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_temporal_accumulate_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (const char* why = tacc_args_bad(pixels_dev, guides_dev, camera, prev_guides_dev, prev_history_dev, prev_camera, out_dev, history_dev, width, height, n_max,
                                        normal_min, plane_k, flags)) {
        set_err(ctx, "rpt_temporal_accumulate_device: %s", why);
        return RPT_ERR_INVALID_ARG;
    }
    if ((((uintptr_t)pixels_dev | (uintptr_t)guides_dev | (uintptr_t)prev_guides_dev | (uintptr_t)prev_history_dev | (uintptr_t)prev_positions_dev |
          (uintptr_t)out_dev | (uintptr_t)history_dev) & 15u) != 0) {
        set_err(ctx, "rpt_temporal_accumulate_device: buffers must be 16-byte aligned");
        return RPT_ERR_INVALID_ARG;
    }
    const size_t px = (size_t)width * height;
    const struct { const void* p; size_t bytes; } ins[5] = {{pixels_dev, 16u * px}, {guides_dev, 64u * px}, {prev_guides_dev, 64u * px},
                                                           {prev_history_dev, 32u * px}, {prev_positions_dev, 16u * px}};
    const auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
        const char *x = (const char*)a, *y = (const char*)b;
        return x < y + nb && y < x + na;
    };
    bool clash = overlap(out_dev, 16u * px, history_dev, 32u * px);
    for (const auto& in : ins)
        if (in.p) clash = clash || overlap(in.p, in.bytes, out_dev, 16u * px) || overlap(in.p, in.bytes, history_dev, 32u * px);
    if (clash) { set_err(ctx, "rpt_temporal_accumulate_device: out_dev or history_dev overlaps an input or each other"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    rptscene::TaccArgs args;
    const rptscene::TaccForm form = rpthost::tacc_args(*camera, prev_camera, prev_camera && prev_positions_dev, width, height, n_max, normal_min, plane_k, args);
    RPT_HIP_CHECK(ctx, rptlaunch::tacc_accumulate(form, args, pixels_dev, guides_dev, prev_guides_dev, prev_history_dev,
                                                  form == rptscene::kTaccReproject ? prev_positions_dev : nullptr, out_dev, history_dev, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_temporal_accumulate(rpt_ctx* ctx, const float* pixels, const rpt_guide* guides, const rpt_camera* camera, const rpt_guide* prev_guides,
                            const rpt_history* prev_history, const rpt_camera* prev_camera, const float* prev_positions, float* out, rpt_history* history,
                            uint32_t width, uint32_t height, float n_max, float normal_min, float plane_k, uint32_t flags)
{
    if (!ctx) { set_err(nullptr, "rpt_temporal_accumulate: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (const char* why = tacc_args_bad(pixels, guides, camera, prev_guides, prev_history, prev_camera, out, history, width, height, n_max, normal_min, plane_k, flags)) {
        set_err(ctx, "rpt_temporal_accumulate: %s", why);
        return RPT_ERR_INVALID_ARG;
    }
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const size_t unit = (size_t)width * height * 16u;                 // one 16-byte line per pixel
    // pixels 1, guides 4, prev_guides 4, prev_history 2, prev_positions 1, out 1, history 2 lines per pixel: one allocation
    RPT_CHECK_RC(ensure_fb(ctx, d, 15u * unit));
    char* base = reinterpret_cast<char*>(d.fb);
    char *px_d = base, *g_d = base + unit, *pg_d = base + 5u * unit, *ph_d = base + 9u * unit, *pp_d = base + 11u * unit, *out_d = base + 12u * unit,
         *hist_d = base + 13u * unit;
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(px_d, pixels, unit, hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(g_d, guides, 4u * unit, hipMemcpyHostToDevice, d.stream));
    if (prev_guides) {
        RPT_HIP_CHECK(ctx, hipMemcpyAsync(pg_d, prev_guides, 4u * unit, hipMemcpyHostToDevice, d.stream));
        RPT_HIP_CHECK(ctx, hipMemcpyAsync(ph_d, prev_history, 2u * unit, hipMemcpyHostToDevice, d.stream));
        if (prev_positions) RPT_HIP_CHECK(ctx, hipMemcpyAsync(pp_d, prev_positions, unit, hipMemcpyHostToDevice, d.stream));
    }
    RPT_CHECK_RC(rpt_temporal_accumulate_device(ctx, reinterpret_cast<const float*>(px_d), reinterpret_cast<const rpt_guide*>(g_d), camera,
                                                prev_guides ? reinterpret_cast<const rpt_guide*>(pg_d) : nullptr,
                                                prev_guides ? reinterpret_cast<const rpt_history*>(ph_d) : nullptr, prev_camera,
                                                prev_guides && prev_positions ? reinterpret_cast<const float*>(pp_d) : nullptr, reinterpret_cast<float*>(out_d),
                                                reinterpret_cast<rpt_history*>(hist_d), width, height, n_max, normal_min, plane_k, flags, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(out, out_d, unit, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(history, hist_d, 2u * unit, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

int rpt_convert_to_u8(rpt_ctx* ctx, const float* pixels, uint8_t* frame, uint32_t width, uint32_t height)
{
    if (!ctx) { set_err(nullptr, "rpt_convert_to_u8: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!pixels || !frame || width == 0 || height == 0) { set_err(ctx, "rpt_convert_to_u8: invalid argument"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const size_t n = (size_t)width * height;
    int rc = ensure_fb(ctx, d, n * 16 + n * 4);                       // f32 RGBA in, u8 RGBA out, one allocation
    if (rc != RPT_OK) return rc;
    uint8_t* out_dev = reinterpret_cast<uint8_t*>(d.fb) + n * 16;
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(d.fb, pixels, n * 16, hipMemcpyHostToDevice, d.stream));
    rc = rpt_convert_to_u8_device(ctx, d.fb, out_dev, width, height, d.stream);
    if (rc != RPT_OK) return rc;
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(frame, out_dev, n * 4, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

// ---- ray queries (include/rpt.h, "ray queries") ------------------------------------------------------------------------------------
// What every query checks before anything is enqueued, in this order: the NULL context, the scene (none: RPT_ERR_NO_SCENE; not a mesh
// scene, or a context with several local devices: RPT_ERR_UNSUPPORTED), the reserved flags, the pointers (`ptrs`: NULL with n > 0,
// or not 16-byte aligned; `optional`: may be NULL, aligned like the others), the batch size.  False: the call returns *rc.  True:
// there is something to launch.
static bool query_ready(rpt_ctx* ctx, const char* name, uint32_t flags, const void* const* ptrs, uint32_t n_ptrs, const void* optional, uint64_t n, bool aligned,
                        int* rc)
{
    *rc = RPT_ERR_INVALID_ARG;
    if (!ctx) { set_err(nullptr, "%s: ctx is NULL", name); return false; }
    if (ctx->scene.kind == SceneKind::none) { set_err(ctx, "%s: no scene uploaded", name); *rc = RPT_ERR_NO_SCENE; return false; }
    if (ctx->scene.kind != SceneKind::mesh) {
        set_err(ctx, "%s: ray queries exist for scenes with meshes only (analytical, large and SDF scenes: not yet)", name);
        *rc = RPT_ERR_UNSUPPORTED;
        return false;
    }
    if (ctx->devs.size() != 1) {
        set_err(ctx, "%s: ray queries run on a context with one local device (rpt_create, rpt_create_rank); this one has %zu", name, ctx->devs.size());
        *rc = RPT_ERR_UNSUPPORTED;
        return false;
    }
    if (flags != 0u) { set_err(ctx, "%s: flags 0x%x (reserved: must be 0)", name, flags); return false; }
    for (uint32_t k = 0; k < n_ptrs; ++k) {
        if (n > 0 && !ptrs[k]) { set_err(ctx, "%s: NULL array with n > 0", name); return false; }
        if (aligned && ((uintptr_t)ptrs[k] & 15u) != 0) { set_err(ctx, "%s: device arrays must be 16-byte aligned", name); return false; }
    }
    if (aligned && ((uintptr_t)optional & 15u) != 0) { set_err(ctx, "%s: device arrays must be 16-byte aligned", name); return false; }
    if (n / 256u + (n % 256u ? 1u : 0u) > 0x7FFFFFFFull) { set_err(ctx, "%s: %llu rays are more than a grid of 0x7FFFFFFF workgroups holds", name, (unsigned long long)n); return false; }
    *rc = RPT_OK;
    return n != 0;
}

// Device d's query allocation, made at the first query after an upload (host_query.h): filled on d's stream, and waited for — a
// query may run on any stream.
static int ensure_query(rpt_ctx* ctx, DevState& d)
{
    if (d.query) return RPT_OK;
    const rpthost::RefitPlan& plan = ctx->refit;
    const rpthost::QueryLayout ql(plan.n_meshes(), d.scene.n_tris);
    void* fresh = nullptr;
    RPT_HIP_CHECK(ctx, hipMalloc(&fresh, ql.total));
    unsigned char* base = static_cast<unsigned char*>(fresh);
    hipError_t e = hipMemsetAsync(base, 0, ql.total, d.stream);
    if (e == hipSuccess && d.scene.n_tris) e = hipMemsetAsync(base + ql.off_none, 0xFF, 4u * (size_t)d.scene.n_tris, d.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(base + ql.off_tri_first, plan.tri_first.data(), sizeof(uint32_t) * plan.tri_first.size(), hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    if (e != hipSuccess) {                                          // (a half-filled allocation is never bound: the next query starts over)
        (void)hipFree(fresh);
        set_err(ctx, "ray queries: filling the query tables failed: %s", hipGetErrorString(e));
        return RPT_ERR_HIP;
    }
    d.query = fresh;
    return RPT_OK;
}

// The batch as the kernels take it.
static QueryArgs query_args_of(const DevState& d, const rpthost::RefitPlan& plan, const rpt_ray* rays, uint64_t n, rpt_hit* hits, rpt_surface* surfaces, uint8_t* occluded)
{
    const rpthost::QueryLayout ql(plan.n_meshes(), d.scene.n_tris);
    QueryArgs q{};
    q.rays = rays; q.hits = hits; q.surfaces = surfaces; q.occluded = occluded;
    q.tri_first = rptargs::table_at<const uint32_t>(d.query, ql.off_tri_first);
    q.n_meshes = plan.n_meshes();
    q.n = n;
    return q;
}

// The tables are bound as they are NOW: after a rebuild the slot order has changed, after a setter the features have.
static int launch_query(rpt_ctx* ctx, DevState& d, const rpt_ray* rays, uint64_t n, rpt_hit* hits, rpt_surface* surfaces, uint8_t* occluded, hipStream_t stream)
{
    RPT_CHECK_RC(ensure_query(ctx, d));
    const bool cutouts = d.cut && d.tex && d.refit && ctx->cut.any();
    const bool normal_maps = d.nrm && d.tex && d.refit && ctx->nrm.any();
    const bool material_maps = d.mmap && d.tex && d.refit && ctx->mmap.any();
    const bool emission_maps = d.emap && d.tex && d.refit && ctx->emap.any();
    const QueryArgs q = query_args_of(d, ctx->refit, rays, n, hits, surfaces, occluded);
    if (!surfaces) {
        if (!cutouts) {
            RPT_HIP_CHECK(ctx, occluded ? rptlaunch::query_occluded(d.scene, q, stream) : rptlaunch::query_closest(d.scene, q, stream));
        } else {
            const SceneMeshCut sc = rptargs::mesh_scene_of<SceneMeshCut>(mesh_view_of(ctx, d));
            RPT_HIP_CHECK(ctx, occluded ? rptlaunch::query_occluded_cut(sc, q, stream) : rptlaunch::query_closest_cut(sc, q, stream));
        }
        return RPT_OK;
    }
    if (!d.refit) {                                                 // (the surface kernels' arguments name slot_vertex)
        RPT_CHECK_RC(ensure_refit(ctx, d));
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    }
    const rptargs::MeshView view = mesh_view_of(ctx, d);
    const rptargs::MmapView maps{d.mmap, ctx->mmap};
    const rptargs::EmapView emits{d.emap, ctx->emap};
    const rptargs::QueryView qv{d.query, rpthost::QueryLayout(ctx->refit.n_meshes(), d.scene.n_tris)};
    switch (rptargs::query_surface_kind_of(cutouts, normal_maps)) {
    case 0u: RPT_HIP_CHECK(ctx, rptlaunch::query_surface(rptargs::mesh_query_scene_of<SceneMeshEmit>(view, maps, material_maps, emits, emission_maps, qv), q, stream)); break;
    case rptargs::kQueryCut: RPT_HIP_CHECK(ctx, rptlaunch::query_surface_cut(rptargs::mesh_query_scene_of<SceneMeshEmitCut>(view, maps, material_maps, emits, emission_maps, qv), q, stream)); break;
    case rptargs::kQueryNrm: RPT_HIP_CHECK(ctx, rptlaunch::query_surface_nrm(rptargs::mesh_query_scene_of<SceneMeshEmitNrm>(view, maps, material_maps, emits, emission_maps, qv), q, stream)); break;
    default: RPT_HIP_CHECK(ctx, rptlaunch::query_surface_nrm_cut(rptargs::mesh_query_scene_of<SceneMeshEmitNrmCut>(view, maps, material_maps, emits, emission_maps, qv), q, stream)); break;
    }
    return RPT_OK;
}

int rpt_trace_rays_device(rpt_ctx* ctx, const rpt_ray* rays_dev, uint64_t n, rpt_hit* hits_dev, rpt_surface* surfaces_dev, uint32_t flags, void* stream)
{
    int rc;
    const void* const ptrs[2] = {rays_dev, hits_dev};
    if (!query_ready(ctx, "rpt_trace_rays_device", flags, ptrs, 2, surfaces_dev, n, true, &rc)) return rc;
    RPT_ON_DEVICE(ctx);
    return launch_query(ctx, ctx->devs[0], rays_dev, n, hits_dev, surfaces_dev, nullptr, (hipStream_t)stream);
}

int rpt_occluded_device(rpt_ctx* ctx, const rpt_ray* rays_dev, uint64_t n, uint8_t* occluded_dev, uint32_t flags, void* stream)
{
    int rc;
    const void* const rays[1] = {rays_dev};
    if (!query_ready(ctx, "rpt_occluded_device", flags, rays, 1, nullptr, n, true, &rc)) return rc;
    if (!occluded_dev) { set_err(ctx, "rpt_occluded_device: NULL array with n > 0"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    return launch_query(ctx, ctx->devs[0], rays_dev, n, nullptr, nullptr, occluded_dev, (hipStream_t)stream);
}

int rpt_camera_rays_device(rpt_ctx* ctx, uint32_t width, uint32_t height, rpt_ray* rays_dev, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_camera_rays_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (width == 0 || height == 0) { set_err(ctx, "rpt_camera_rays_device: zero width or height"); return RPT_ERR_INVALID_ARG; }
    int rc;
    const void* const ptrs[1] = {rays_dev};
    if (!query_ready(ctx, "rpt_camera_rays_device", 0u, ptrs, 1, nullptr, (uint64_t)width * height, true, &rc)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::query_camera_rays(make_camera(ctx->scene.camera, (float)width, (float)height), width, height, rays_dev, (hipStream_t)stream));
    return RPT_OK;
}

// The host forms: the rays up, the records down, through the context's staging buffer on its own stream; they block.
static int query_host(rpt_ctx* ctx, const char* name, const rpt_ray* rays, uint64_t n, rpt_hit* hits, rpt_surface* surfaces, uint8_t* occluded, uint32_t flags)
{
    int rc;
    const void* const ptrs[2] = {rays, occluded ? (const void*)occluded : (const void*)hits};
    if (!query_ready(ctx, name, flags, ptrs, 2, nullptr, n, false, &rc)) return rc;
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const auto up = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    const size_t off_hits = up(sizeof(rpt_ray) * (size_t)n);
    const size_t off_surfaces = off_hits + up(occluded ? (size_t)n : sizeof(rpt_hit) * (size_t)n);
    const size_t total = off_surfaces + (surfaces ? up(sizeof(rpt_surface) * (size_t)n) : 0u);
    RPT_CHECK_RC(ensure_fb(ctx, d, total));
    unsigned char* base = reinterpret_cast<unsigned char*>(d.fb);
    rpt_ray* rays_dev = reinterpret_cast<rpt_ray*>(base);
    rpt_hit* hits_dev = occluded ? nullptr : reinterpret_cast<rpt_hit*>(base + off_hits);
    uint8_t* occluded_dev = occluded ? base + off_hits : nullptr;
    rpt_surface* surfaces_dev = surfaces ? reinterpret_cast<rpt_surface*>(base + off_surfaces) : nullptr;
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(rays_dev, rays, sizeof(rpt_ray) * (size_t)n, hipMemcpyHostToDevice, d.stream));
    RPT_CHECK_RC(launch_query(ctx, d, rays_dev, n, hits_dev, surfaces_dev, occluded_dev, d.stream));
    if (occluded) RPT_HIP_CHECK(ctx, hipMemcpyAsync(occluded, occluded_dev, (size_t)n, hipMemcpyDeviceToHost, d.stream));
    else RPT_HIP_CHECK(ctx, hipMemcpyAsync(hits, hits_dev, sizeof(rpt_hit) * (size_t)n, hipMemcpyDeviceToHost, d.stream));
    if (surfaces) RPT_HIP_CHECK(ctx, hipMemcpyAsync(surfaces, surfaces_dev, sizeof(rpt_surface) * (size_t)n, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

int rpt_trace_rays(rpt_ctx* ctx, const rpt_ray* rays, uint64_t n, rpt_hit* hits, rpt_surface* surfaces, uint32_t flags)
{
    return query_host(ctx, "rpt_trace_rays", rays, n, hits, surfaces, nullptr, flags);
}

int rpt_occluded(rpt_ctx* ctx, const rpt_ray* rays, uint64_t n, uint8_t* occluded, uint32_t flags)
{
    if (ctx && n > 0 && !occluded) { set_err(ctx, "rpt_occluded: NULL array with n > 0"); return RPT_ERR_INVALID_ARG; }
    return query_host(ctx, "rpt_occluded", rays, n, nullptr, nullptr, occluded, flags);
}

// ---- radiance queries (include/rpt.h, "radiance queries") --------------------------------------------------------------------------
// Device d's radiance allocation, made at the first radiance query after an upload (host_rad.h): filled on d's stream, and waited for —
// a query may run on any stream.
static int ensure_rad(rpt_ctx* ctx, DevState& d)
{
    if (d.rad) return RPT_OK;
    rpthost::build_rad_plan(ctx->refit, ctx->rad);
    const rpthost::MedLayout ml = ctx->rad.layout();
    void* fresh = nullptr;
    RPT_HIP_CHECK(ctx, hipMalloc(&fresh, ml.total ? ml.total : 16u));
    unsigned char* base = static_cast<unsigned char*>(fresh);
    hipError_t e = ml.total ? hipMemsetAsync(base, 0, ml.total, d.stream) : hipSuccess;
    for (const rpthost::RadFill& f : rpthost::rad_fills(ml))
        if (e == hipSuccess) e = hipMemsetAsync(base + f.off, f.value, f.bytes, d.stream);
    if (e == hipSuccess && !ctx->rad.tri_medium.empty())
        e = hipMemcpyAsync(base + ml.off_tri_medium, ctx->rad.tri_medium.data(), sizeof(uint32_t) * ctx->rad.tri_medium.size(), hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    if (e != hipSuccess) {                                          // (a half-filled allocation is never bound: the next query starts over)
        (void)hipFree(fresh);
        set_err(ctx, "radiance queries: filling the query's tables failed: %s", hipGetErrorString(e));
        return RPT_ERR_HIP;
    }
    ctx->rad.release_staging();
    d.rad = fresh;
    return RPT_OK;
}

// The tables are bound as they are NOW, as launch_query does; the call's samples go out as launches of at most kMaxSppPerLaunch.
// Nothing of the render's dispatch state is read or written: last_form and last_choice stay the last render's.
static int launch_radiance(rpt_ctx* ctx, DevState& d, const rpt_ray* rays, uint64_t n, float* out, uint64_t frames_done, uint32_t spp, uint64_t seed,
                           uint32_t first_index, hipStream_t stream)
{
    RPT_CHECK_RC(ensure_rad(ctx, d));
    if (!d.refit) {                                                 // (the forms' arguments name slot_vertex and the vertices)
        RPT_CHECK_RC(ensure_refit(ctx, d));
        RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    }
    const bool environment = d.env && d.refit && ctx->env.any();
    const bool cutouts = d.cut && d.tex && d.refit && ctx->cut.any();
    const bool normal_maps = d.nrm && d.tex && d.refit && ctx->nrm.any();
    const bool material_maps = d.mmap && d.tex && d.refit && ctx->mmap.any();
    const bool emission_maps = d.emap && d.tex && d.refit && ctx->emap.any();
    const bool media = d.med && d.refit && ctx->med.any();
    const rptargs::MeshView view = mesh_view_of(ctx, d);
    const rptargs::MmapView maps{d.mmap, ctx->mmap};
    const rptargs::EmapView emits{d.emap, ctx->emap};
    const rptargs::MedView meds{d.med, ctx->med};
    const rptargs::RadView rv{d.rad, ctx->rad};
    const uint32_t form = rpthost::rad_form_of(normal_maps, cutouts, environment);
    const uint32_t max_spp = rptlaunch::radiance_max_spp();
    RadArgs a{};
    a.rays = rays; a.out = out; a.n = n;
    a.seed = seed; a.first_index = first_index;
    a.shade_threshold = knobs().shade_threshold;
    const auto scene_of = [&](auto tag) {
        using S = typename decltype(tag)::type;
        return rptargs::mesh_rad_scene_of<S>(view, maps, material_maps, emits, emission_maps, meds, media, rv);
    };
    for (uint32_t k = 0; k < rpthost::rad_launches(spp, max_spp); ++k) {
        a.frames_done = frames_done + (uint64_t)k * max_spp;
        a.spp = rpthost::rad_launch_spp(spp, max_spp, k);
        using rpthost::kRadCut; using rpthost::kRadEnv; using rpthost::kRadNrm;
        switch (form) {
        case 0u: RPT_HIP_CHECK(ctx, rptlaunch::radiance(scene_of(std::common_type<SceneMeshMed>{}), a, stream)); break;
        case kRadEnv: RPT_HIP_CHECK(ctx, rptlaunch::radiance_env(scene_of(std::common_type<SceneMeshMedEnv>{}), a, stream)); break;
        case kRadCut: RPT_HIP_CHECK(ctx, rptlaunch::radiance_cut(scene_of(std::common_type<SceneMeshMedCut>{}), a, stream)); break;
        case kRadCut | kRadEnv: RPT_HIP_CHECK(ctx, rptlaunch::radiance_cut_env(scene_of(std::common_type<SceneMeshMedCutEnv>{}), a, stream)); break;
        case kRadNrm: RPT_HIP_CHECK(ctx, rptlaunch::radiance_nrm(scene_of(std::common_type<SceneMeshMedNrm>{}), a, stream)); break;
        case kRadNrm | kRadEnv: RPT_HIP_CHECK(ctx, rptlaunch::radiance_nrm_env(scene_of(std::common_type<SceneMeshMedNrmEnv>{}), a, stream)); break;
        case kRadNrm | kRadCut: RPT_HIP_CHECK(ctx, rptlaunch::radiance_nrm_cut(scene_of(std::common_type<SceneMeshMedNrmCut>{}), a, stream)); break;
        default: RPT_HIP_CHECK(ctx, rptlaunch::radiance_nrm_cut_env(scene_of(std::common_type<SceneMeshMedNrmCutEnv>{}), a, stream)); break;
        }
    }
    return RPT_OK;
}

int rpt_radiance_device(rpt_ctx* ctx, const rpt_ray* rays_dev, uint64_t n, float* out_dev, uint64_t frames_done, uint32_t spp, uint64_t seed, uint32_t first_index,
                        uint32_t flags, void* stream)
{
    int rc;
    const void* const ptrs[2] = {rays_dev, out_dev};
    if (!query_ready(ctx, "rpt_radiance_device", flags, ptrs, 2, nullptr, n, true, &rc)) return rc;
    if (!frames_in_domain(ctx, "rpt_radiance_device", frames_done, spp)) return RPT_ERR_INVALID_ARG;
    if (spp == 0) return RPT_OK;
    RPT_ON_DEVICE(ctx);
    return launch_radiance(ctx, ctx->devs[0], rays_dev, n, out_dev, frames_done, spp, seed, first_index, (hipStream_t)stream);
}

// The host form: the rays and the pixels up, the pixels down, through the context's staging buffer on its own stream; it blocks.
int rpt_radiance(rpt_ctx* ctx, const rpt_ray* rays, uint64_t n, float* out, uint64_t frames_done, uint32_t spp, uint64_t seed, uint32_t first_index, uint32_t flags)
{
    int rc;
    const void* const ptrs[2] = {rays, out};
    if (!query_ready(ctx, "rpt_radiance", flags, ptrs, 2, nullptr, n, false, &rc)) return rc;
    if (!frames_in_domain(ctx, "rpt_radiance", frames_done, spp)) return RPT_ERR_INVALID_ARG;
    if (spp == 0) return RPT_OK;
    RPT_ON_DEVICE(ctx);
    DevState& d = ctx->devs[0];
    const auto up = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    const size_t off_out = up(sizeof(rpt_ray) * (size_t)n);
    RPT_CHECK_RC(ensure_fb(ctx, d, off_out + up(16u * (size_t)n)));
    unsigned char* base = reinterpret_cast<unsigned char*>(d.fb);
    rpt_ray* rays_dev = reinterpret_cast<rpt_ray*>(base);
    float* out_dev = reinterpret_cast<float*>(base + off_out);
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(rays_dev, rays, sizeof(rpt_ray) * (size_t)n, hipMemcpyHostToDevice, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(out_dev, out, 16u * (size_t)n, hipMemcpyHostToDevice, d.stream));
    RPT_CHECK_RC(launch_radiance(ctx, d, rays_dev, n, out_dev, frames_done, spp, seed, first_index, d.stream));
    RPT_HIP_CHECK(ctx, hipMemcpyAsync(out, out_dev, 16u * (size_t)n, hipMemcpyDeviceToHost, d.stream));
    RPT_HIP_CHECK(ctx, hipStreamSynchronize(d.stream));
    return RPT_OK;
}

int rpt_camera_sample_rays_device(rpt_ctx* ctx, uint32_t width, uint32_t height, uint64_t frame, uint64_t seed, rpt_ray* rays_dev, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_camera_sample_rays_device: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (width == 0 || height == 0) { set_err(ctx, "rpt_camera_sample_rays_device: zero width or height"); return RPT_ERR_INVALID_ARG; }
    int rc;
    const void* const ptrs[1] = {rays_dev};
    if (!query_ready(ctx, "rpt_camera_sample_rays_device", 0u, ptrs, 1, nullptr, (uint64_t)width * height, true, &rc)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::radiance_camera_rays(make_camera(ctx->scene.camera, (float)width, (float)height), width, height, frame_key_hd(seed, frame), rays_dev,
                                                       (hipStream_t)stream));
    return RPT_OK;
}

int rpt_synchronize(rpt_ctx* ctx, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_synchronize: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return check_handoffs_all(ctx);
}

#ifdef RPT_TEST_HOOKS    // include/rpt_test.h: the test build only
int rpt_probe_rays(rpt_ctx* ctx, const float* rays_dev, uint32_t* out_dev, uint64_t n, uint32_t use_grid, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_probe_rays: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::large) { set_err(ctx, "rpt_probe_rays: needs an uploaded large scene"); return RPT_ERR_NO_SCENE; }
    if (!rays_dev || !out_dev) { set_err(ctx, "rpt_probe_rays: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if (n == 0) return RPT_OK;
    RPT_ON_DEVICE(ctx);
    SceneLarge sc = ctx->devs[0].scene;
    if (!use_grid) sc.use_accel = 0;
    RPT_HIP_CHECK(ctx, rptlaunch::probe_rays(sc, rays_dev, out_dev, n, (hipStream_t)stream));
    return RPT_OK;
}

// The mesh and environment probes' shared prefix, in this order: the NULL context, the scene kind, the pointers and the flag bits
// outside `allowed`, the feature the probe needs (`missing`: what to say of a scene without it, or NULL when it is there or the probe
// needs none), n == 0.  False: the hook returns *rc.  True: it sets the device (RPT_ON_DEVICE) and launches.
typedef const char* (*ProbeNeed)(const rpt_ctx*);
static bool probe_ready(rpt_ctx* ctx, const char* name, const void* in_dev, const void* out_dev, uint32_t flags, uint32_t allowed, uint64_t n, int* rc,
                        ProbeNeed missing = nullptr)
{
    *rc = RPT_ERR_INVALID_ARG;
    if (!ctx) { set_err(nullptr, "%s: ctx is NULL", name); return false; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "%s: needs an uploaded scene with meshes", name); *rc = RPT_ERR_NO_SCENE; return false; }
    if (!in_dev || !out_dev || (flags & ~allowed)) { set_err(ctx, "%s: invalid argument", name); return false; }
    if (const char* what = missing ? missing(ctx) : nullptr) { set_err(ctx, "%s: %s", name, what); return false; }
    *rc = RPT_OK;
    return n != 0;
}
static const char* probe_needs_smooth(const rpt_ctx* c) { return !c->smooth.any() || !c->devs[0].smooth ? "no mesh is SMOOTH" : nullptr; }
static const char* probe_needs_lights(const rpt_ctx* c) { return !c->light.any() || !c->devs[0].light ? "no mesh is ON" : nullptr; }
static const char* probe_needs_tex(const rpt_ctx* c) { return !c->tex.any() || !c->devs[0].tex ? "no mesh is textured" : nullptr; }
static const char* probe_needs_cut(const rpt_ctx* c) { return !c->cut.any() || !c->devs[0].cut || !c->devs[0].tex ? "no mesh has a cutout" : nullptr; }
static const char* probe_needs_nrm(const rpt_ctx* c) { return !c->nrm.any() || !c->devs[0].nrm || !c->devs[0].tex ? "no mesh has a normal map" : nullptr; }
static const char* probe_needs_mmap(const rpt_ctx* c) { return !c->mmap.any() || !c->devs[0].mmap || !c->devs[0].tex ? "no mesh has a material map" : nullptr; }
static const char* probe_needs_emap(const rpt_ctx* c) { return !c->emap.any() || !c->devs[0].emap || !c->devs[0].tex ? "no mesh has an emission map" : nullptr; }
static const char* probe_needs_emap_and_lights(const rpt_ctx* c) { const char* what = probe_needs_emap(c); return what ? what : probe_needs_lights(c); }
static const char* probe_needs_env(const rpt_ctx* c) { return !c->env.any() || !c->devs[0].env ? "no environment is set" : nullptr; }

int rpt_debug_mesh_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_USE_MAX | RPT_MESH_QUERY_BRUTE, n, &rc)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_query(ctx->devs[0].scene, rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_normal_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_normal_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_BRUTE, n, &rc, probe_needs_smooth)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_normal_query(rptargs::mesh_scene_of<SceneMeshSmooth>(mesh_view_of(ctx, ctx->devs[0])), rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_light_sample(rpt_ctx* ctx, const float* in_dev, uint64_t n, uint32_t* out_dev, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_light_sample", in_dev, out_dev, 0u, 0u, n, &rc, probe_needs_lights)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_light_sample(rptargs::mesh_scene_of<SceneMeshLight>(mesh_view_of(ctx, ctx->devs[0])), in_dev, out_dev, n, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_texture_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_texture_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_BRUTE, n, &rc, probe_needs_tex)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_texture_query(rptargs::mesh_scene_of<SceneMeshTex>(mesh_view_of(ctx, ctx->devs[0])), rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_cutout_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_cutout_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_USE_MAX | RPT_MESH_QUERY_BRUTE, n, &rc, probe_needs_cut)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_cutout_query(rptargs::mesh_scene_of<SceneMeshCut>(mesh_view_of(ctx, ctx->devs[0])), rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_normal_map_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_normal_map_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_BRUTE, n, &rc, probe_needs_nrm)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_normal_map_query(rptargs::mesh_scene_of<SceneMeshNrm>(mesh_view_of(ctx, ctx->devs[0])), rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_material_map_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_material_map_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_BRUTE, n, &rc, probe_needs_mmap)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_material_map_query(rptargs::mesh_map_scene_of<SceneMeshMap>(mesh_view_of(ctx, ctx->devs[0]), rptargs::MmapView{ctx->devs[0].mmap, ctx->mmap}), rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

// The argument of the emission-map probes: the form over the textured mesh-light tables, bound as a launch binds it.
static SceneMeshEmit emit_probe_scene_of(rpt_ctx* ctx, const DevState& d)
{
    const bool material_maps = d.mmap && ctx->mmap.any();
    return rptargs::mesh_emit_scene_of<SceneMeshEmit>(mesh_view_of(ctx, d), rptargs::MmapView{d.mmap, ctx->mmap}, material_maps, rptargs::EmapView{d.emap, ctx->emap});
}

int rpt_debug_mesh_emission_map_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_emission_map_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_BRUTE, n, &rc, probe_needs_emap)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_emission_map_query(emit_probe_scene_of(ctx, ctx->devs[0]), rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_emission_map_sample(rpt_ctx* ctx, const float* in_dev, uint64_t n, uint32_t* out_dev, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_emission_map_sample", in_dev, out_dev, 0u, 0u, n, &rc, probe_needs_emap_and_lights)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_emission_map_sample(emit_probe_scene_of(ctx, ctx->devs[0]), in_dev, out_dev, n, (hipStream_t)stream));
    return RPT_OK;
}

static const char* probe_needs_med(const rpt_ctx* c) { return !c->med.any() || !c->devs[0].med || !c->devs[0].refit ? "no mesh carries a medium" : nullptr; }

int rpt_debug_mesh_media_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_mesh_media_query", rays_dev, out_dev, flags, RPT_MESH_QUERY_BRUTE, n, &rc, probe_needs_med)) return rc;
    RPT_ON_DEVICE(ctx);
    const DevState& d = ctx->devs[0];
    const bool material_maps = d.mmap && d.tex && ctx->mmap.any(), emission_maps = d.emap && d.tex && ctx->emap.any();
    const SceneMeshMed sc = rptargs::mesh_med_scene_of<SceneMeshMed>(mesh_view_of(ctx, d), rptargs::MmapView{d.mmap, ctx->mmap}, material_maps,
                                                                    rptargs::EmapView{d.emap, ctx->emap}, emission_maps, rptargs::MedView{d.med, ctx->med});
    RPT_HIP_CHECK(ctx, rptlaunch::mesh_media_query(sc, rays_dev, out_dev, n, flags, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_env_query(rpt_ctx* ctx, const float* dirs_dev, uint64_t n, uint32_t* out_dev, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_env_query", dirs_dev, out_dev, 0u, 0u, n, &rc, probe_needs_env)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::env_query(rptargs::mesh_scene_of<SceneMeshEnv>(mesh_view_of(ctx, ctx->devs[0])), dirs_dev, out_dev, n, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_env_sample(rpt_ctx* ctx, const float* in_dev, uint64_t n, uint32_t* out_dev, void* stream)
{
    int rc;
    if (!probe_ready(ctx, "rpt_debug_env_sample", in_dev, out_dev, 0u, 0u, n, &rc, probe_needs_env)) return rc;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::env_sample(rptargs::mesh_scene_of<SceneMeshEnv>(mesh_view_of(ctx, ctx->devs[0])), in_dev, out_dev, n, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_debug_mesh_stats(rpt_ctx* ctx, uint32_t* n_nodes, uint32_t* depth, float* build_ms)
{
    if (!ctx || !n_nodes || !depth || !build_ms) { set_err(ctx, "rpt_debug_mesh_stats: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_debug_mesh_stats: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    *n_nodes = ctx->scene.mesh_nodes; *depth = ctx->scene.mesh_depth; *build_ms = ctx->scene.mesh_build_ms;
    return RPT_OK;
}

int rpt_debug_mesh_walk(rpt_ctx* ctx, uint32_t* walk)
{
    if (!ctx || !walk) { set_err(ctx, "rpt_debug_mesh_walk: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_debug_mesh_walk: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    *walk = 0u;
    for (const DevState& d : ctx->devs) *walk += d.scene.use_bvh ? 1u : 0u;
    return RPT_OK;
}

int rpt_debug_mesh_tables(rpt_ctx* ctx, uint32_t which, void* out, uint64_t capacity_bytes, uint64_t* bytes)
{
    if (!ctx || !bytes || which > 1u) { set_err(ctx, "rpt_debug_mesh_tables: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if (ctx->scene.kind != SceneKind::mesh) { set_err(ctx, "rpt_debug_mesh_tables: needs an uploaded scene with meshes"); return RPT_ERR_NO_SCENE; }
    const DevState& d = ctx->devs[0];
    *bytes = which == 0u ? 48ull * d.scene.n_tris : 64ull * ctx->scene.mesh_nodes;
    if (!out || capacity_bytes < *bytes) { set_err(ctx, "rpt_debug_mesh_tables: %llu bytes do not fit", (unsigned long long)*bytes); return RPT_ERR_INVALID_ARG; }
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, hipDeviceSynchronize());
    RPT_HIP_CHECK(ctx, hipMemcpy(out, which == 0u ? d.scene.tris : d.scene.nodes, (size_t)*bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_probe_math(rpt_ctx* ctx, uint32_t fn, const float* a_dev, const float* b_dev, float* out_dev, uint64_t n, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_probe_math: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    const bool relaxed = (fn & RPT_PROBE_RELAXED) != 0u;
    fn &= ~(uint32_t)RPT_PROBE_RELAXED;
    if (!a_dev || !b_dev || !out_dev || fn > RPT_PROBE_DIV3) { set_err(ctx, "rpt_probe_math: invalid argument"); return RPT_ERR_INVALID_ARG; }
    if (n == 0) return RPT_OK;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, relaxed ? rptlaunch_fast::probe_math(fn, a_dev, b_dev, out_dev, n, (hipStream_t)stream)
                               : rptlaunch::probe_math(fn, a_dev, b_dev, out_dev, n, (hipStream_t)stream));
    return RPT_OK;
}

int rpt_probe_fn(rpt_ctx* ctx, uint32_t fn, const float* in_dev, float* out_dev, uint64_t n, const float* params, void* stream)
{
    if (!ctx) { set_err(nullptr, "rpt_probe_fn: ctx is NULL"); return RPT_ERR_INVALID_ARG; }
    if (!in_dev || !out_dev || fn >= RPT_PROBE_FN_COUNT) { set_err(ctx, "rpt_probe_fn: invalid argument"); return RPT_ERR_INVALID_ARG; }
    DevCamera cam;
    memset(&cam, 0, sizeof(cam));
    if (fn == RPT_PROBE_FN_GEN_RAY) {
        if (ctx->scene.kind == SceneKind::none) { set_err(ctx, "rpt_probe_fn: GEN_RAY uses the uploaded scene's camera"); return RPT_ERR_NO_SCENE; }
        if (!params) { set_err(ctx, "rpt_probe_fn: GEN_RAY needs params = {width, height}"); return RPT_ERR_INVALID_ARG; }
        cam = make_camera(ctx->scene.camera, params[0], params[1]);
    }
    if (n == 0) return RPT_OK;
    RPT_ON_DEVICE(ctx);
    RPT_HIP_CHECK(ctx, rptlaunch::probe_fn(fn, cam, in_dev, out_dev, n, (hipStream_t)stream));
    return RPT_OK;
}

#endif  // RPT_TEST_HOOKS

}  // extern "C"
#pragma GCC visibility pop

#ifdef RPT_PROFILE_BLOCKS
// Development build only (dev_prof.h, tools/block_profile.py): not part of include/rpt.h.  Every kernel class's object keeps its own
// counters; a profiled run uses one class, so their sum is that class's table.
extern "C" __attribute__((visibility("default"))) int rpt_prof_read(unsigned long long* out)
{
    unsigned long long part[rptdev::PB_COUNT * 3];
    for (uint32_t i = 0; i < rptdev::PB_COUNT * 3; ++i) out[i] = 0;
    hipError_t (*const readers[3])(unsigned long long*) = {rptlaunch::prof_read_small, rptlaunch::prof_read_sdf, rptlaunch::prof_read_large};
    for (auto rd : readers) {
        if (rd(part) != hipSuccess) return RPT_ERR_HIP;
        for (uint32_t i = 0; i < rptdev::PB_COUNT * 3; ++i) out[i] += part[i];
    }
    return RPT_OK;
}
#endif
