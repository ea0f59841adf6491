// svo_rt.hip -- MI355X (gfx950) sparse-voxel-octree primary-ray caster.
//
// C-ABI plugin (include/svo_rt.h) replacing the reference's Unity host driver
// RaytracingMaster.cs + the HLSL compute kernel RaytraceCompute.compute /
// NVIDIASVO.compute / AttachmentLookup.compute (reference repo paths).
//
// Device data layout (DESIGN.md "Data layout in HBM"):
//   nodes : uint2[N]  .x = valid8 << 8 | nonleaf8,  .y = absolute index of the
//           first non-leaf child.  One 8-byte load per descriptor fetch.  The
//           reference's 16-bit RELATIVE pointer (NaiveCreator.cs:164-165) is
//           resolved to absolute at upload, so pools deeper than 16-bit
//           pointers allow use the same kernel.
//   att   : uint2[N]  .x = colorA565 | colorB565 << 16, .y = choices16 | normal16 << 16
//           (NaiveCreator.cs:189-191), one 8-byte load per hit.
//
// Multi-device contexts (svo_create_multi): one node-pool replica per device;
// a frame is split into band_rows-row bands dealt round-robin to the devices;
// the display device (devices[0]) renders its bands straight into the caller's
// frame, every other device into a band-contiguous payload (12-byte compact
// records, or RGBA8 for display-only frames), and one assemble kernel on the
// display device pulls the payloads over xGMI (peer access) and rebuilds the
// frame's rows.  All of it is enqueued on streams; nothing blocks the host.
//
// Numerics: compiled with -ffp-contract=off and correctly rounded f32 div/sqrt
// so every expression rounds exactly as the strict-IEEE oracle (oracle/).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "svo_rt.h"
#include "svo_ambient.h"
#include "svo_light.h"
#include "svo_object.h"
#include "svo_beam.h"
#include "svo_lod.h"
#include "svo_sched.h"
#include "svo_traverse.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return fail(SVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct Upload {
    size_t offset, count;
    int depth;
    bool external;   // has child links outside its own range (sub-SVO linking)
    bool tree;       // every node reached once from the upload's first node (no sharing, no cycles)
    // beam starts: the splat list of a self-contained tree at offset 0, built from the
    // host arrays at upload (null: none; a pool of several uploads is walked on the device copy)
    std::shared_ptr<const std::vector<uint2>> boxes;
    int boxes_back;      // the config's beam_back it was built with
    std::shared_ptr<const std::vector<uint2>> boxes_held;   // ... and the held view's (beam_back_held)
    int boxes_held_back;
};

// The device copy of a splat list (a context holds two: a moving camera's and a held view's)
struct DevBoxes {
    uint2 *d = nullptr;
    size_t cap = 0;
    uint32_t n = 0;
    uint64_t id = 0;   // made from the list with this id (0: none)
};

enum { STAGE_KERNEL = 0, STAGE_ASSEMBLE = 1, N_STAGES = 2 };

using svo_sched::Geo;   // the tile-order cache key (svo_sched.h)
using svo_beam::beam_camera;   // the host side of the beam starts (svo_beam.h)
using svo_beam::build_beam_boxes;
using svo_beam::finest_box_depth;

// Cost-ordered dispatch state of the renders on one stream: every launch records each
// 8x8 tile's trip count; the order kernel, enqueued right behind it, turns them into
// the heaviest-first dispatch order of the next launch at the same geometry.  One set
// per stream (up to MAX_SCHED streams), so renders on different streams -- frames in
// flight -- share nothing mutable and run concurrently.
constexpr int MAX_SCHED = 4;
struct Sched {
    hipStream_t stream = nullptr;
    bool used = false;
    bool idle = false;               // nothing enqueued on `stream` since the last svo_synchronize
    unsigned long long last_use = 0;
    hipEvent_t done = nullptr;       // eviction: recorded on this stream when another takes the set over
    // The dispatch order is built OFF the render stream (round 5): after launch n
    // the order kernel runs on `side` (behind an event on the render stream) from the costs launch n
    // wrote, into one of two order buffers, and the first launch to dispatch in it is n + 2 -- so
    // launch n + 1 never waits for it.  Launch n writes its costs into buffer n % 2 (the build
    // after launch n reads them while launch n + 1 writes the other one); a launch waits on the
    // build event of a build it follows by >= 2 launches once, before its kernel, and only if the
    // host has not already seen that build complete (a held view: never).
    uint16_t *cost_buf[2] = {};
    uint16_t *part_buf[2] = {};          // segmented tiles: per tile and part (SEG_KMAX x cap)
    uint32_t *order_buf[2] = {};
    hipStream_t side = nullptr;
    hipEvent_t render_done = nullptr;    // recorded on the render stream behind a launch a build follows
    hipEvent_t build_ev[2] = {};
    long long build_at[2] = {-1, -1};    // the launch after which buffer i's order was built (-1: none)
    bool build_seen[2] = {};             // the render stream already waits for it (or it completed)
    Geo build_key[2];
    int next_buf = 0;
    uint16_t *shadow_cost = nullptr;   // the two-pass shadow form's own costs and order
    uint32_t *shadow_order = nullptr;
    size_t cap = 0;
    size_t order_cap = 0;              // order_buf entries allocated
    float4 *seg_hint = nullptr;        // segmented tiles: per pixel the segment starts (svo_traverse.h)
    size_t hint_cap = 0;
    unsigned long long *tile_start = nullptr;   // beam starts of this stream's launches (svo_traverse.h)
    size_t ts_cap = 0;
    uint32_t ts_gen = 0;               // the generation of the last launch's keys ...
    unsigned long long ts_view = ~0ull; // ... splatted for this view, splat list and frame size
    uint64_t ts_boxes = 0;
    int ts_w = -1, ts_h = -1;
    bool held_splat = false;           // this launch re-splatted a held view finer: its costs are new
    Geo order_key;                   // the newest build's key (width -1: none)
    Geo shadow_key;
    unsigned long long launches = 0, shadow_launches = 0;
    unsigned long long built_view = 0;   // the context's view generation the order was built under
    unsigned long long view_prev = ~0ull;   // the view generation of this stream's last launch ...
    float off_prev[2] = {-1.0f, -1.0f};     // ... and its pixel offset
    unsigned long long built_cost = ~0ull;  // the context's cost generation the order was built under
    unsigned long long last_build = 0;      // the launch count at the last order build
    int built_mode = -1;                 // shadows | stack_mode << 2 of the costs it was built from
    // loop-form choice (see launch): a ring of the last STATS_RING order builds' statistics
    // (host-visible: per XCD max / sum of the tile costs the order kernel saw, 16 words each),
    // each read only once its build has completed (its event); the decision it gives is kept
    // with the geometry, view and render mode it was measured at.  A ring rather than one slot:
    // while the camera moves every launch rebuilds the order, and one slot would be re-recorded
    // before the host ever found it complete.
    static constexpr int STATS_RING = 4;
    uint32_t *stats = nullptr;           // STATS_RING x 16 words
    hipEvent_t stats_ev[STATS_RING] = {};
    bool stats_pending[STATS_RING] = {};
    Geo stats_key[STATS_RING];
    unsigned long long stats_view[STATS_RING] = {};
    int stats_mode[STATS_RING] = {};
    int stats_head = 0;                  // the slot the next build writes
    bool relayout_pending = false;       // a launch ran in an order of another class layout (see launch)
    int lat_cache = 0;                   // the decision of the last completed build ...
    bool lat_short = false;              // ... and whether its heaviest tile's chain was short
    bool lat_thin = false;               // ... and whether its work was thin against that chain (svo_config.seg_table_thin)
    Geo lat_key;                         // ... made at this geometry / view / mode (width -1: none)
    unsigned long long lat_view = 0;
    int lat_mode = -1;
};

struct Peer {                       // one per member of a multi-device context (index 0: the display device)
    void *buf[2] = {nullptr, nullptr};   // band payload, double-buffered across frames
    size_t cap_bytes = 0;
    hipEvent_t rendered[2] = {nullptr, nullptr};
    void *dense = nullptr;               // sparse payload: the band's dense RGB before the pack
    size_t dense_cap = 0;
    float4 *accum = nullptr;             // svo_render_samples: this member's band accumulation (band layout)
    int accum_w = 0, accum_rows = -1;
    uint64_t accum_deal = 0;             // the band deal its rows belong to
    int link = SVO_LINK_SELF;            // how the payload reaches the display device (svo_get_member_link)
    int native_link = SVO_LINK_SELF;     // ... without svo_config.peer_copy (what svo_create_multi found)
    void *local[2] = {nullptr, nullptr}; // SVO_LINK_COPY: the payload's copy on the display device
    size_t local_cap = 0;
};


// Host threads that move svo_render's outputs from the plugin's pinned staging into the
// caller's (pageable) arrays, chunk by chunk, while the DMA of the next chunk runs.
class CopyPool {
  public:
    explicit CopyPool(int n) {
        for (int i = 0; i < n; ++i) th_.emplace_back([this] { run(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    int size() const { return (int)th_.size(); }
    void submit(void *dst, const void *src, size_t n) {
        {
            std::lock_guard<std::mutex> l(m_);
            q_.push_back(Job{static_cast<char *>(dst), static_cast<const char *>(src), n});
            ++pending_;
        }
        cv_.notify_one();
    }
    void wait() {
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
    }

  private:
    struct Job { char *dst; const char *src; size_t n; };
    void run() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                j = q_.front();
                q_.pop_front();
            }
            std::memcpy(j.dst, j.src, j.n);
            {
                std::lock_guard<std::mutex> l(m_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::deque<Job> q_;
    size_t pending_ = 0;
    bool stop_ = false;
};

}  // namespace

struct svo_ctx {
    int device = 0;
    size_t capacity = 0;
    size_t n_nodes = 0;
    uint2 *d_nodes = nullptr;
    uint2 *d_att = nullptr;
    int32_t *d_stage = nullptr;   // staging for V1 descriptor conversion
    size_t stage_cap = 0;
    hipStream_t stream = nullptr;
    svo::Camera cam{};
    bool cam_set = false;
    std::vector<Upload> uploads;
    int depth = 0;
    bool depth_exact = false;        // see recompute_pool
    // the splat list of the whole pool (beam starts; null: none) and its unique id
    std::shared_ptr<const std::vector<uint2>> pool_boxes;
    uint64_t pool_boxes_id = 0;
    int pool_boxes_back = -1;
    // ... and the finer one a held view re-splats with (beam_back_held; the same list when equal)
    std::shared_ptr<const std::vector<uint2>> pool_boxes_held;
    uint64_t pool_boxes_held_id = 0;
    // the finest box of each list as its depth (side 2^-depth; recompute_pool): the LOD floor's s_min
    int pool_boxes_fine = 0, pool_boxes_held_fine = 0;
    // level of detail of the primary rays (svo_set_lod; 0, 0: off -- DESIGN.md 3.1f)
    float lod_coef = 0.0f, lod_bias = 0.0f;
    // specular reflection bounces of the renders (svo_set_reflection; max_bounces 0 or specular 0: off --
    // DESIGN.md 3.2c) and the pass's voxel-key scratch (the records and the hit list reuse the shadow
    // forms' scratch: the two never run together)
    float specular[3] = {0.0f, 0.0f, 0.0f};
    int max_bounces = 0;
    unsigned long long *d_refl_voxel = nullptr;
    size_t refl_voxel_cap = 0;
    uint8_t *d_object_ids = nullptr;     // the object pass's per-pixel ids for the scene-aware light pass (grow-only)
    size_t object_ids_cap = 0;
    // skybox (svo_set_skybox; texels null: the procedural gradient -- DESIGN.md 3.2d): the texture on this
    // device, one float4 per texel; the sky pass reads the tile hit masks from the caller's array or from
    // the head of d_shadow_list (the shadow forms' and the reflection pass's scratch)
    svo_sky::Texture sky{nullptr, 0, 0, 0u};
    // ambient term of the renders (svo_set_ambient; n_rays 0 or ambient 0: off -- DESIGN.md 3.2e): the pass
    // shares the reflection pass's scratch (the two never run together).  ambient_step: the sample index a
    // progressive render adds to the variant for its one launch, 0 elsewhere
    float ambient[3] = {0.0f, 0.0f, 0.0f};
    int ambient_rays = 0;
    float ambient_radius = std::numeric_limits<float>::infinity();
    uint32_t ambient_variant = 0, ambient_step = 0;
    // point lights of the renders (svo_set_lights; none: off -- DESIGN.md 3.2g): the pass shares the
    // reflection pass's scratch (the two never run together); the list travels as a kernel argument
    svo_lights::Light lights[svo_lights::MAX_LIGHTS] = {};
    int n_lights = 0;
    // placed sub-SVOs of the renders (svo_set_objects; none: off -- DESIGN.md 3.2h): the list travels as a
    // kernel argument of the object pass
    svo_objects::Object objects[svo_objects::MAX_OBJECTS] = {};
    int n_objects = 0;
    // diagnostics (the library's only environment switches, read once at svo_create):
    // SVO_DEBUG bit 0 the loop-form / class-table decision trace, bit 1 the order each launch
    // takes; SVO_WAVE_LOG=<file> the per-wave record; SVO_BEAM_DIAG the splat's timing variants
    int debug = 0;
    std::string wave_log_path;
    uint32_t beam_diag = 0;
    // host-path output scratch
    void *d_out_hits = nullptr;
    void *d_shadow_list = nullptr;   // compacted shadow pass: hit masks, offsets, hit list (svo_kernel.hip)
    size_t shadow_list_cap = 0;
    void *d_out_rgba = nullptr;
    size_t out_cap_px = 0;
    // svo_render: pinned staging of the outputs, its per-chunk events, and the host copy threads
    void *h_stage = nullptr;
    size_t h_stage_cap = 0;
    static constexpr int STAGE_CHUNKS = 16;
    hipEvent_t stage_ev[STAGE_CHUNKS] = {};
    std::unique_ptr<CopyPool> copy_pool;
    // svo_render_progressive: the accumulated frame (RGBA32F, zeroed on a size
    // change) and its RGBA8 display words
    float4 *d_accum = nullptr;
    uint32_t *d_accum8 = nullptr;
    int accum_w = 0, accum_h = 0;
    // svo_render_progressive_async: the accumulated frame's RGBA8 words packed into one of
    // PIN_SLOTS device slots and copied on copy_stream into plugin-owned pinned host memory
    // (the D2H of frame k overlaps the render of frame k + 1)
    static constexpr int PIN_SLOTS = 3;
    uint32_t *h_pin[PIN_SLOTS] = {};
    uint32_t *d_pin[PIN_SLOTS] = {};
    hipEvent_t pin_packed[PIN_SLOTS] = {}, pin_copied[PIN_SLOTS] = {};
    bool pin_used[PIN_SLOTS] = {};
    hipStream_t copy_stream = nullptr;
    int pin_w = 0, pin_h = 0, pin_next = 0;
    int pin_format = SVO_PIXELS_RGBA8;   // the slots' pixel format (svo_render_progressive_async)
    int pin_push = 0;                    // svo_config.readback: 0 hipMemcpyAsync (DMA), 1 a kernel writes the
                                         // mapped pinned buffer, 2 the DMA split over two copy streams
    int host_copy_threads = 0;           // svo_config.host_copy_threads (0: half the hardware threads)
    hipStream_t copy_stream2 = nullptr;
    hipEvent_t pin_copied2[PIN_SLOTS] = {};
    unsigned long long pin_frames = 0;   // frames enqueued since the slots were (re)allocated
    int num_cus = 256;
    size_t lds_per_block = 160 * 1024;   // hipDeviceProp.sharedMemPerBlock
    int xcd_remap = 2;               // svo_config.xcd_strips: 2 interleaved column strips (default), 0 raster
    uint32_t options = 0;            // svo_set_options
    // SVO_OPT_KERNEL_TIMING: event pairs around the primary kernel / the assemble kernel
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timing_events[N_STAGES];   // recorded, not yet read
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timing_free;               // reusable
    uint32_t *d_wave_log = nullptr;  // diagnostics: env SVO_WAVE_LOG=<file>
    size_t wave_log_cap = 0;
    // cost-ordered tile dispatch (svo_rt.hip Sched): switches and per-stream state
    int tile_order = 1;              // svo_config.tile_order (0: strip order)
    int prio = 1;                    // svo_config.issue_priority 0: no issue priority by cost class
    int shadow_order_enabled = 1;    // svo_config.shadow_order 0: shadow tiles in plain strip order
    int fetch_all = -1;              // svo_config.fetch_all 0|1 (default: by pool size, see launch)
    int fused_shadows = 1;           // svo_config.shadow_form 1: shadow rays as a second launch
    int shadow_compact = 0;          // svo_config.shadow_form 2: that launch over the compacted hit list
    int lat_mode = -1;               // svo_config.loop_form: 0 never, 1 always, unset: by the last launch's costs (see launch)
    int seg_mode = 1;                // svo_config.segments 0: never trace heavy tiles as segmented rays (see launch)
    int seg_kpack_lat = 0x444;       // svo_config.seg_table_latency: the K of each cost class (nibble c: class c, >= 7/8,
                                     // 3/4, 1/2, 1/4, 1/8 of the max, rest; 0 none, 4 or 8) in a latency-bound launch
    int seg_kpack_issue = 0x4;       // svo_config.seg_table_issue: the same in an issue-bound launch
    int seg_kpack_thin = 0x888;      // svo_config.seg_table_thin: ... and in a latency-bound launch whose summed trips
    float thin_ratio = 0.083f;       // are below svo_config.seg_thin_ratio x slots x its heaviest tile's: C3 8-way bands
                                     // (flyover 0.045, Main.unity 0.079) and the overview frame (0.063) run faster
                                     // with every heavy class in eighths, the flyover 4-way band (0.087) with 444
                                     // (profiles/r05_thin_ab.json)
    int seg_cap = 96;                // svo_config.seg_cap: at most this many segmented tiles per XCD
    int seg_all = 0;                 // svo_config.seg_all 4|8 (tests): every tile segmented with that K
    uint32_t seg_scramble = 0;       // svo_config.seg_scramble (tests): arbitrary segment starts
    uint32_t seg_launches = 0;
    int beam = 1;                    // svo_config.beam: beam starts
    int beam_back = 2;               // svo_config.beam_back: a new view's splat, this many levels above the leaves
    int beam_back_held = 0;          // svo_config.beam_back_held: a held view's (-1: beam_back)
    DevBoxes dev_boxes[2];           // device copies of pool_boxes / pool_boxes_held
    unsigned long long *count_ts = nullptr;   // beam starts of an instrumented launch (SVO_OPT_COUNT_BEAM)
    size_t count_ts_cap = 0;
    uint32_t count_ts_gen = 0;
    float lat_ratio = 0.3f;          // svo_config.lat_ratio: the auto rule's threshold ...
    // the stored segment starts are those of the pixel's ray in the previous launch: of another
    // sub-pixel ray after a jittered launch, of another view while the camera moves.  Such a launch
    // splits its segments evenly from the beam start instead (segments past an earlier segment's
    // record end early; trace_seg): C3 one-sample route 94.6 against 97.9 us (overview 84.3 / 88.8),
    // a slow pan 91.2 / 93.0 us (profiles/r05_stale_starts.txt).  1: the stored starts, 0 (jittered
    // launches only): no segments
    int seg_move = 2;                // svo_config.seg_move: a launch at a new view
    int seg_jitter = 2;              // svo_config.seg_jitter: a jittered launch (the one-sample samples route)
    int spread = 1;                  // svo_config.move_spread 0: a moving camera's order classes tiles by their own costs only
    int relayout = 1;                // svo_config.relayout 0: keep an order built from costs of another class layout
    int seg_min_chain = 160;         // svo_config.seg_min_chain: a latency-bound launch whose heaviest tile costs fewer
                                     // trips takes the latency form, unsegmented, without beam starts
    float seg_ratio = 0.28f;         // svo_config.seg_ratio: ... and the same with beam starts (class table only)
    int move_every = 4;              // svo_config.move_every: while the camera moves every launch, rebuild the
                                     // order only every k-th launch (see launch; 1 = at every new view).
                                     // C3 pan: 118.8 us per frame at 1, 110.7 at 4, 111.9 at 8
    int order_every = 32;            // svo_config.order_every: rebuild the order every k-th launch (and after
                                     // every camera move or change of render mode)
    unsigned long long view_gen = 0; // bumped when svo_set_camera changes the matrices
    unsigned long long cost_gen = 0; // bumped by whatever else changes the tiles' costs: a new pixel
                                     // offset or light, an upload
    Sched sched[MAX_SCHED];
    unsigned long long sched_clock = 0;
    // The one piece of state renders on different streams still share: the host-path /
    // two-pass-shadow scratch outputs.  A render that uses them waits for the previous
    // such render's stream (an event recorded at the switch; no host sync).
    hipStream_t scratch_stream = nullptr;
    bool scratch_valid = false;
    hipEvent_t switch_event = nullptr;
    // Ray queries (svo_trace_rays): render state is never touched; the only state is scratch,
    // grow-only, handed from stream to stream like the host-path scratch above (an event recorded
    // on the previous user's stream at the switch).  Ordered mode: keys and indices (in, out) and
    // the radix sort's temporary storage; the host path: the staged rays and outputs.
    uint32_t *q_keys = nullptr;          // 4 x q_cap words: keys, sorted keys, indices, sorted indices
    size_t q_cap = 0;
    void *q_temp = nullptr;
    size_t q_temp_cap = 0;
    void *q_host = nullptr;              // device staging of the _host ray-batch calls (HostStage lays out the parts)
    size_t q_host_cap = 0;               // its size in bytes
    hipStream_t q_stream = nullptr;
    bool q_valid = false;
    hipEvent_t q_event = nullptr;
    // multi-device context (svo_create_multi); empty for a single-device one
    std::vector<svo_ctx *> members;
    std::vector<Peer> peers;
    hipEvent_t gathered[2] = {nullptr, nullptr};
    bool gathered_used[2] = {false, false};
    int parity = 0;
    int band_rows = 8;
    int deal_cycle = 0;                  // svo_set_band_deal: weighted deal over the members (0: round-robin)
    int sparse_payload = 0;              // svo_config.sparse_payload: display-only frames travel as sparse parts
    int peer_copy = 0;                   // svo_config.peer_copy: every member's payload copied, not pulled
    uint8_t deal_owner[svo::MAX_CYCLE] = {};
    uint64_t samples_deal = 0;           // the deal of the last svo_render_samples (band accumulations' rows)
    bool samples_deal_set = false;
};

namespace {

bool is_multi(const svo_ctx *ctx) { return !ctx->members.empty(); }

// V1 (relative, int32) -> device node (absolute, uint2).  NaiveCreator.cs:184-187.
__global__ void convert_v1_kernel(const int32_t *__restrict__ desc, uint2 *__restrict__ nodes,
                                  size_t n, uint32_t base) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t cd = (uint32_t)desc[i];
    uint32_t self = base + (uint32_t)i;
    uint2 o;
    o.x = cd & 0xFFFFu;
    o.y = cd ? self + (cd >> 16) : 0u;   // node == 0 <=> descriptor word == 0 (HLSL re-fetch test)
    nodes[base + i] = o;
}

// Make stream s wait for the work the previous scratch user enqueued on another stream.
int order_scratch(svo_ctx *ctx, hipStream_t s) {
    if (ctx->scratch_valid && ctx->scratch_stream != s) {
        // the previous stream is alive: a caller keeps its streams until svo_forget_stream /
        // svo_synchronize / svo_destroy (svo_rt.h)
        if (!ctx->switch_event) HIP_TRY(hipEventCreateWithFlags(&ctx->switch_event, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->switch_event, ctx->scratch_stream));
        HIP_TRY(hipStreamWaitEvent(s, ctx->switch_event, 0));
    }
    ctx->scratch_stream = s;
    ctx->scratch_valid = true;
    return SVO_OK;
}

// Forget every order build of the set (the buffers stay; the caller has synchronised).
void reset_builds(Sched &q) {
    for (int i = 0; i < 2; ++i) {
        q.build_at[i] = -1;
        q.build_seen[i] = false;
        q.build_key[i] = Geo();
    }
    q.order_key = q.shadow_key = Geo();
}

void free_sched(Sched &q) {
    for (int i = 0; i < 2; ++i) {
        if (q.cost_buf[i]) hipFree(q.cost_buf[i]);
        if (q.part_buf[i]) hipFree(q.part_buf[i]);
        if (q.order_buf[i]) hipFree(q.order_buf[i]);
        q.cost_buf[i] = q.part_buf[i] = nullptr;
        q.order_buf[i] = nullptr;
    }
    if (q.shadow_cost) hipFree(q.shadow_cost);
    if (q.shadow_order) hipFree(q.shadow_order);
    q.shadow_cost = nullptr;
    q.shadow_order = nullptr;
    q.cap = 0;
    q.order_cap = 0;
    reset_builds(q);
}

// The grow-only device buffer: replace *buf by one of `bytes` bytes; *cap, in the owner's own unit,
// is 0 while there is none and new_cap afterwards.  The caller has waited for whatever may still
// use the old buffer (its stream, or the device).
template <class T>
int regrow(T **buf, size_t *cap, size_t new_cap, size_t bytes) {
    if (*buf) hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(buf, bytes));
    *cap = new_cap;
    return SVO_OK;
}

// The scheduling state of stream s: its own set, or a free one, or the least recently
// used one -- taken over only after the stream that used it has finished its renders.
int sched_for(svo_ctx *ctx, hipStream_t s, Sched **out) {
    Sched *pick = nullptr;
    for (Sched &q : ctx->sched)
        if (q.used && q.stream == s) pick = &q;
    if (!pick) {
        for (Sched &q : ctx->sched)
            if (!q.used) { pick = &q; break; }
    }
    if (!pick) {
        pick = &ctx->sched[0];
        for (Sched &q : ctx->sched)
            if (q.last_use < pick->last_use) pick = &q;
        // s takes over the set only after the renders the evicted stream was given: an event
        // recorded on that stream NOW stands behind all of them (host order = stream order).
        // Recorded here, at the rare eviction, not behind every launch: a marker packet
        // between two renders of one stream cost ~2-3 us of GPU time per frame.  The evicted
        // stream is alive: callers keep a stream until svo_forget_stream (svo_rt.h).
        // After svo_synchronize nothing is pending there and the stream may be gone (svo_rt.h):
        // record nothing on it.
        if (!pick->idle) {
            if (!pick->done) HIP_TRY(hipEventCreateWithFlags(&pick->done, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(pick->done, pick->stream));
            HIP_TRY(hipStreamWaitEvent(s, pick->done, 0));
        }
        if (pick->side) HIP_TRY(hipStreamSynchronize(pick->side));   // its order builds (rare: an eviction)
        reset_builds(*pick);   // built for another stream's frames
        pick->launches = pick->shadow_launches = 0;
        pick->view_prev = ~0ull;
        pick->built_cost = ~0ull;
        pick->last_build = 0;
        for (int r = 0; r < Sched::STATS_RING; ++r) pick->stats_pending[r] = false;
        pick->lat_key = Geo();
        pick->lat_mode = -1;
    }
    pick->stream = s;
    pick->used = true;
    pick->idle = false;
    pick->last_use = ++ctx->sched_clock;
    *out = pick;
    return SVO_OK;
}

// Host-side level walk: validates every non-leaf child index and returns the
// number of descriptor levels reachable from the upload's first node.  A
// breadth-first walk with a seen set: exact for a tree; for a DAG it is the
// shallowest depth and on a cycle it still terminates (the upload is accepted),
// so for anything but one tree at offset 0 the stack is sized by recompute_pool's
// longest-path walk of the whole pool, not from this depth.
int walk_depth(const uint32_t *lo, const uint32_t *first, size_t n, size_t base, size_t pool_n,
               int *depth_out, bool *external_out, bool *tree_out, std::string *err) {
    *tree_out = true;
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> cur{0}, nxt;
    int depth = 0;
    bool external = false;
    if (n == 0) { *depth_out = 0; *external_out = false; return 0; }
    seen[0] = 1;
    while (!cur.empty()) {
        ++depth;
        if (depth > 22) { *err = "node pool deeper than 22 levels (s_max = 23)"; return -1; }
        nxt.clear();
        for (uint32_t li : cur) {
            uint32_t m = lo[li] & 0xFFu;
            uint32_t f = first[li];
            int rank = 0;
            for (int c = 0; c < 8; ++c) {
                if (!((m >> c) & 1u)) continue;
                uint64_t child = (uint64_t)f + (uint64_t)rank++;
                if (child >= pool_n) {
                    *err = "child pointer of node " + std::to_string(base + li) + " -> " +
                           std::to_string(child) + " outside the node-pool capacity (" + std::to_string(pool_n) + ")";
                    return -1;
                }
                if (child < base || child >= base + n) { external = true; continue; }
                uint32_t cl = (uint32_t)(child - base);
                if (seen[cl]) { *tree_out = false; continue; }   // shared subtrees are legal (DAG)
                seen[cl] = 1;
                nxt.push_back(cl);
            }
        }
        cur.swap(nxt);
    }
    *depth_out = depth;
    *external_out = external;
    return 0;
}

// The splat depth of a held view (svo_config.beam_back_held; -1: a new view's)
int held_back(const svo_ctx *ctx) { return ctx->beam_back_held < 0 ? ctx->beam_back : ctx->beam_back_held; }

int validate_upload(svo_ctx *ctx, const uint32_t *lo, const uint32_t *first, size_t n, size_t base, Upload *out) {
    std::string err;
    int depth = 0;
    bool ext = false, tree = true;
    // links may point past what is uploaded so far (the reference uploads the trunk
    // before the sub-SVO it links to, Clipmap.cs:158,168): any index inside the
    // capacity is legal; the pool is zero-filled at svo_create, so a link into a
    // region not uploaded yet reads empty descriptors
    if (walk_depth(lo, first, n, base, ctx->capacity, &depth, &ext, &tree, &err) != 0) return fail(SVO_ERR_FORMAT, err);
    *out = Upload{base, n, depth, ext, tree, nullptr, -1, nullptr, -1};
    if (base == 0 && tree && !ext && ctx->beam) {   // the common case: the splat lists from the host arrays
        const int hb = held_back(ctx);
        out->boxes = build_beam_boxes(lo, first, n, depth, ctx->beam_back);
        out->boxes_back = ctx->beam_back;
        out->boxes_held = hb == ctx->beam_back ? out->boxes : build_beam_boxes(lo, first, n, depth, hb);
        out->boxes_held_back = hb;
    }
    return SVO_OK;
}

uint64_t next_boxes_id() {
    static std::atomic<uint64_t> next_id{0};
    return ++next_id;
}

// The pool's traversal facts and its splat list, after every upload and beam config change.
//  * One self-contained tree uploaded at offset 0 (the reference's SetSVOBuffer(data)): its own
//    upload walk; the splat list built from its host arrays then.
//  * Anything else -- a trunk whose leaves link to sub-SVOs uploaded elsewhere (Clipmap.cs:153-169
//    via SetSVOBuffer(data, offset), RaytracingMaster.cs:118-135), several uploads, a shared
//    subtree: the pool as the device holds it is walked from the root (node 0) across the uploads.
//    A child index past the uploaded nodes reads as the zero-filled empty descriptor (no
//    children).  The walk finds the longest descriptor path from the root.  An acyclic pool --
//    a tree or a DAG with shared subtrees -- of at most 22 levels is exact: the stack needs
//    depth - 1 slots and cannot overflow, the launch is unguarded, and the splat list comes from
//    this walk, so a linked pool gets beam starts too.  A pool with a cycle, or one whose longest
//    path exceeds 22 levels, has no proven depth: depth = 22, the guarded loop with its 21-slot
//    stack (scales 2..22; a PUSH below scale 2 ends the ray with flag bit 2, svo_kernel.hip
//    trace_lean) and no beam starts.
int recompute_pool(svo_ctx *ctx) {
    ctx->depth_exact = false;
    ctx->depth = 22;
    std::shared_ptr<const std::vector<uint2>> boxes, held;
    const int hb = held_back(ctx);
    const bool simple = ctx->uploads.size() == 1 && ctx->uploads[0].offset == 0 && !ctx->uploads[0].external &&
                        ctx->uploads[0].tree && ctx->uploads[0].depth <= 22;
    if (simple) {
        ctx->depth_exact = true;
        ctx->depth = ctx->uploads[0].depth;
        if (ctx->beam && ctx->uploads[0].boxes_back == ctx->beam_back && ctx->uploads[0].boxes_held_back == hb) {
            boxes = ctx->uploads[0].boxes;
            held = ctx->uploads[0].boxes_held;
        }
    }
    const bool have = boxes || !ctx->beam;
    if ((!simple || !have) && ctx->n_nodes > 0 && ctx->n_nodes < 0xFFFFFFFFull) {
        // the device copy of the pool (the host arrays of earlier uploads are gone)
        const size_t n = ctx->n_nodes;
        std::vector<uint2> pool(n);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(pool.data(), ctx->d_nodes, n * sizeof(uint2), hipMemcpyDeviceToHost));
        std::vector<uint32_t> lo(n), first(n);
        for (size_t i = 0; i < n; ++i) {
            lo[i] = pool[i].x;
            first[i] = pool[i].y;
        }
        if (!simple) {
            // the longest descriptor path from the root, depth(v) = 1 + the max depth of v's non-leaf
            // children (a child past the uploads reads as an empty descriptor: depth 1): an iterative
            // depth-first walk, each node finished once, so shared subtrees (every trunk leaf linking
            // the same sub-SVO, Clipmap.cs:158-159) cost nothing extra; a cycle has no depth
            std::vector<uint8_t> state(n, 0), dep(n, 0), acc(n, 0);   // state: 0 new, 1 open, 2 done
            struct Frame { uint32_t v; uint32_t slot; };
            std::vector<Frame> st{{0u, 0u}};
            state[0] = 1;
            bool ok = true;
            while (!st.empty() && ok) {
                Frame &f = st.back();
                const uint32_t v = f.v, m = lo[v] & 0xFFu;
                bool pushed = false;
                while (f.slot < 8) {
                    const uint32_t c = f.slot++;
                    if (!((m >> c) & 1u)) continue;
                    const uint64_t child = (uint64_t)first[v] + (uint32_t)__builtin_popcount(m & ((1u << c) - 1u));
                    if (child >= n) { acc[v] = std::max<uint8_t>(acc[v], 1); continue; }
                    if (state[child] == 1) { ok = false; break; }   // a cycle
                    if (state[child] == 2) { acc[v] = std::max(acc[v], dep[child]); continue; }
                    state[child] = 1;
                    st.push_back({(uint32_t)child, 0u});
                    pushed = true;
                    break;
                }
                if (!ok || pushed) continue;
                dep[v] = (uint8_t)std::min(1 + (int)acc[v], 23);   // 23: deeper than the stack allows
                state[v] = 2;
                st.pop_back();
                if (!st.empty()) acc[st.back().v] = std::max(acc[st.back().v], dep[v]);
            }
            if (ok && dep[0] <= 22) {
                ctx->depth_exact = true;
                ctx->depth = dep[0];
            }
        }
        if (ctx->depth_exact && ctx->beam) {
            boxes = build_beam_boxes(lo.data(), first.data(), n, ctx->depth, ctx->beam_back);
            held = hb == ctx->beam_back ? boxes : build_beam_boxes(lo.data(), first.data(), n, ctx->depth, hb);
        }
    }
    if (boxes != ctx->pool_boxes) {
        ctx->pool_boxes = boxes;
        ctx->pool_boxes_id = boxes ? next_boxes_id() : 0;
        ctx->pool_boxes_fine = finest_box_depth(boxes);
    }
    if (held != ctx->pool_boxes_held) {
        ctx->pool_boxes_held = held;
        ctx->pool_boxes_held_id = !held ? 0 : held == boxes ? ctx->pool_boxes_id : next_boxes_id();
        ctx->pool_boxes_held_fine = finest_box_depth(held);
    }
    ctx->pool_boxes_back = ctx->beam_back;
    return SVO_OK;
}

// Commit an upload's metadata -- only after its device copies have completed.
int commit_upload(svo_ctx *ctx, const Upload &u) {
    ctx->uploads.erase(std::remove_if(ctx->uploads.begin(), ctx->uploads.end(),
                                      [&](const Upload &v) { return v.offset == u.offset; }),
                       ctx->uploads.end());
    ctx->uploads.push_back(u);
    ctx->n_nodes = std::max(ctx->n_nodes, u.offset + u.count);
    ++ctx->cost_gen;   // another pool: other costs
    return recompute_pool(ctx);
}

int ensure_out(svo_ctx *ctx, size_t px) {
    if (px <= ctx->out_cap_px) return SVO_OK;
    HIP_TRY(hipDeviceSynchronize());   // an earlier asynchronous launch may still use the old scratch
    if (ctx->d_out_hits) hipFree(ctx->d_out_hits);
    if (ctx->d_out_rgba) hipFree(ctx->d_out_rgba);
    ctx->d_out_hits = ctx->d_out_rgba = nullptr;
    ctx->out_cap_px = 0;
    HIP_TRY(hipMalloc(&ctx->d_out_hits, px * sizeof(svo_hit)));
    HIP_TRY(hipMalloc(&ctx->d_out_rgba, px * 4 * sizeof(float)));
    ctx->out_cap_px = px;
    return SVO_OK;
}

// *fresh = true when the frame was (re)allocated: the caller's sample counter then
// describes a frame that no longer exists, so the next blend must replace it (sample 0)
int ensure_accum(svo_ctx *ctx, int width, int height, bool *fresh) {
    *fresh = false;
    if (ctx->d_accum && ctx->accum_w == width && ctx->accum_h == height) return SVO_OK;
    *fresh = true;
    HIP_TRY(hipDeviceSynchronize());   // an earlier asynchronous launch may still use the old frame
    if (ctx->d_accum) hipFree(ctx->d_accum);
    if (ctx->d_accum8) hipFree(ctx->d_accum8);
    ctx->d_accum = nullptr;
    ctx->d_accum8 = nullptr;
    ctx->accum_w = ctx->accum_h = 0;
    const size_t px = (size_t)width * (size_t)height;
    HIP_TRY(hipMalloc(&ctx->d_accum, px * sizeof(float4)));
    HIP_TRY(hipMalloc(&ctx->d_accum8, px * sizeof(uint32_t)));
    HIP_TRY(hipMemset(ctx->d_accum, 0, px * sizeof(float4)));   // a fresh render target
    ctx->accum_w = width;
    ctx->accum_h = height;
    return SVO_OK;
}

void free_pinned(svo_ctx *ctx) {
    for (int i = 0; i < svo_ctx::PIN_SLOTS; ++i) {
        if (ctx->h_pin[i]) hipHostFree(ctx->h_pin[i]);
        if (ctx->d_pin[i]) hipFree(ctx->d_pin[i]);
        if (ctx->pin_packed[i]) hipEventDestroy(ctx->pin_packed[i]);
        if (ctx->pin_copied[i]) hipEventDestroy(ctx->pin_copied[i]);
        if (ctx->pin_copied2[i]) hipEventDestroy(ctx->pin_copied2[i]);
        ctx->pin_copied2[i] = nullptr;
        ctx->h_pin[i] = nullptr;
        ctx->d_pin[i] = nullptr;
        ctx->pin_packed[i] = ctx->pin_copied[i] = nullptr;
        ctx->pin_used[i] = false;
    }
    ctx->pin_w = ctx->pin_h = 0;
    ctx->pin_next = 0;
    ctx->pin_frames = 0;
}

// The pinned readback slots for a width x height frame (reallocated on a size change: the
// previous frames' pointers die with them).
int ensure_pinned(svo_ctx *ctx, int width, int height) {
    if (ctx->h_pin[0] && ctx->pin_w == width && ctx->pin_h == height) return SVO_OK;
    if (ctx->copy_stream) HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
    if (ctx->copy_stream2) HIP_TRY(hipStreamSynchronize(ctx->copy_stream2));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    free_pinned(ctx);
    if (!ctx->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (ctx->pin_push == 2 && !ctx->copy_stream2)
        HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream2, hipStreamNonBlocking));
    // 16-byte multiple (the push kernel moves 16 B per lane); the frame is the first W * H words
    const size_t bytes = ((size_t)width * (size_t)height * sizeof(uint32_t) + 15) & ~(size_t)15;
    const unsigned host_flags = ctx->pin_push == 1 ? (hipHostMallocMapped | hipHostMallocCoherent) : hipHostMallocDefault;
    for (int i = 0; i < svo_ctx::PIN_SLOTS; ++i) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_pin[i]), bytes, host_flags));
        HIP_TRY(hipMalloc(&ctx->d_pin[i], bytes));
        HIP_TRY(hipEventCreateWithFlags(&ctx->pin_packed[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->pin_copied[i], hipEventDisableTiming));
        if (ctx->pin_push == 2) HIP_TRY(hipEventCreateWithFlags(&ctx->pin_copied2[i], hipEventDisableTiming));
    }
    ctx->pin_w = width;
    ctx->pin_h = height;
    return SVO_OK;
}

// A validated svo_band, the owner table copied (the caller's pointer is not kept).
struct Deal {
    int rows = 1, rank = 0, count = 1, cycle = 0;
    uint8_t owner[svo::MAX_CYCLE] = {};
    int owner_of(int band) const { return cycle ? owner[band % cycle] : band % count; }
    uint64_t key() const {   // identifies the deal (tile-order cache key)
        uint64_t h = 1469598103934665603ull;
        for (int i = 0; i < cycle; ++i) h = (h ^ owner[i]) * 1099511628211ull;
        return h ^ (uint64_t)cycle;
    }
};

int band_rows_local(int height, const Deal &d) {
    // rows y whose band y / rows belongs to this rank
    int rows = 0;
    if (d.cycle == 0) {
        for (int y0 = d.rank * d.rows; y0 < height; y0 += d.rows * d.count) rows += std::min(d.rows, height - y0);
        return rows;
    }
    for (int b = 0; b * d.rows < height; ++b)
        if (d.owner[b % d.cycle] == d.rank) rows += std::min(d.rows, height - b * d.rows);
    return rows;
}

int check_band(const svo_band *band, int height, Deal *out) {
    Deal d;
    if (band) {
        d.rows = band->band_rows;
        d.rank = band->band_rank;
        d.count = band->band_count;
        d.cycle = band->cycle;
    }
    if (d.rows <= 0 || d.count <= 0 || d.rank < 0 || d.rank >= d.count) return fail(SVO_ERR_ARG, "invalid svo_band");
    if (d.cycle < 0 || d.cycle > svo::MAX_CYCLE) return fail(SVO_ERR_ARG, "svo_band.cycle must be in [0, 256]");
    if (d.cycle > 0) {
        if (!band->owner) return fail(SVO_ERR_ARG, "svo_band.owner is null");
        for (int i = 0; i < d.cycle; ++i) {
            if (band->owner[i] >= d.count) return fail(SVO_ERR_ARG, "svo_band.owner entry out of range");
            d.owner[i] = band->owner[i];
        }
    }
    if (d.count == 1) {
        d.rows = height > 0 ? height : 1;
        d.cycle = 0;
    }
    *out = d;
    return SVO_OK;
}

int take_events(svo_ctx *ctx, int stage, hipEvent_t *ev0, hipEvent_t *ev1) {
    *ev0 = *ev1 = nullptr;
    if (!(ctx->options & SVO_OPT_KERNEL_TIMING)) return SVO_OK;
    if (ctx->timing_free.empty()) {
        HIP_TRY(hipEventCreate(ev0));
        if (hipEventCreate(ev1) != hipSuccess) {
            hipEventDestroy(*ev0);
            *ev0 = nullptr;
            return fail(SVO_ERR_HIP, "hipEventCreate");
        }
    } else {
        *ev0 = ctx->timing_free.back().first;
        *ev1 = ctx->timing_free.back().second;
        ctx->timing_free.pop_back();
    }
    ctx->timing_events[stage].emplace_back(*ev0, *ev1);
    return SVO_OK;
}

svo::Outputs outputs_of(const svo_frame *f) {
    svo::Outputs o{};
    if (!f) return o;
    o.hits = reinterpret_cast<svo::Hit *>(f->hits);
    o.rgba = reinterpret_cast<float4 *>(f->rgba);
    o.rgba8 = f->rgba8;
    o.compact = reinterpret_cast<uint32_t *>(f->compact);
    o.position = reinterpret_cast<float4 *>(f->position);
    o.voxel = reinterpret_cast<unsigned long long *>(f->voxel);
    o.rgb8 = f->rgb8;
    o.hitmask = reinterpret_cast<unsigned long long *>(f->hitmask);
    o.frame_layout = f->layout == SVO_LAYOUT_FRAME ? 1 : 0;
    return o;
}

// svo_render_samples' arguments (launch's optional last parameter)
struct SampleArgs {
    int n;
    const float *offsets;   // 2 n floats
    uint32_t first;
    float4 *accum;
    uint32_t *rgba8;
    uint8_t *rgb8;
    int layout;
};

// What the phases of one launch (below, in launch's order) share.
struct LaunchPlan {
    Deal b;
    int stack_mode = 0;
    hipStream_t s = nullptr;
    Sched *q = nullptr;   // the stream's scheduling state (null: strip order, or an instrumented launch)
    Geo key;              // the geometry (seg 0): the key of the costs and of the loop-form decision
    Geo okey;             // the order's key: key + the seg_cap and class table its order was built with
    int seg_cap = 0, n_tiles = 0;
    int mode_now = 0;     // the render mode the costs are keyed on: shadows | stack_mode << 2
    int used_kpack = 0;   // the class layout of the order this launch dispatches in
    bool instr = false;   // instrumented: svo_count_fetches / svo_beam_starts
    bool jittered = false;       // per-launch pixel offsets: the tiles' costs drift without a new view
    bool latency_bound = false;
    bool beam_planned = false;   // this launch's primary rays get beam starts (less the per-launch camera checks)
    size_t n_wave = 0;    // wave-log records: one per workgroup
};

// The launch parameters every form starts from.
void base_params(const svo_ctx *ctx, const LaunchPlan &L, int width, int height, const svo::Outputs &out,
                 svo::LaunchParams &p) {
    const Deal &b = L.b;
    const int stack_mode = L.stack_mode;
    std::memset(&p, 0, sizeof p);
    p.nodes = ctx->d_nodes;
    p.att = ctx->d_att;
    p.n_nodes = (uint32_t)std::min<size_t>(ctx->n_nodes, 0xFFFFFFFFu);
    p.cam = ctx->cam;
    p.width = width;
    p.height = height;
    p.band_rows = b.rows;
    p.band_rank = b.rank;
    p.band_count = b.count;
    p.band_cycle = b.cycle;
    for (int i = 0; i < b.cycle; ++i)
        if (b.owner[i] == b.rank) p.band_pos[p.band_cnt++] = (uint8_t)i;
    p.local_rows = band_rows_local(height, b);
    p.slots = std::max(ctx->depth - 1, 1);
    // guard: stack-overflow test + HLSL parent round trip, needed unless the pool's longest
    // path is proven (depth_exact: a tree or an acyclic DAG of at most 22 levels -- a cycle or
    // a deeper pool gets the guarded 21-slot stack, recompute_pool), its parent indices are
    // exact in f32 and the lean loop's 32-bit node byte offsets fit (fewer than 2^29 nodes)
    p.guard = !ctx->depth_exact || (stack_mode == 0 && ctx->n_nodes > ((size_t)1 << 24)) ||
              ctx->n_nodes >= ((size_t)1 << 29);
    // unpredicated node loads pay off on pools below 2^24 nodes (C2, C3: 5-9 %) and
    // cost 6-12 % on the 25 M / 100 M-node C4 / C5 pools (svo_kernel.hip trace_lean)
    p.fetch_all = ctx->fetch_all >= 0 ? ctx->fetch_all : (ctx->n_nodes < ((size_t)1 << 24) ? 1 : 0);
    p.out = out;
    if (b.count == 1) p.out.frame_layout = 0;   // the whole frame: both layouts coincide
    p.xcd_remap = ctx->xcd_remap;
    if (p.xcd_remap == 2 && ((width + 7) / 8) % (8 * svo::STRIP_K) != 0) p.xcd_remap = 0;
    p.shadows = (ctx->options & SVO_OPT_SHADOW_RAYS) ? (ctx->shadow_compact ? 3 : ctx->fused_shadows ? 2 : 1) : 0;
}

// svo_render_samples' two forms: one sample folded into the one-sample launch, or samples in flight.
int sample_forms(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p, const SampleArgs *sa) {
    const Deal &b = L.b;
    if (sa && sa->n == 1) {
        // one sample: the one-sample launch itself with AddShader's blend in its store epilogue (the
        // samples kernel's S waves per tile, barrier and blend loop cost S = 1 ~13 %)
        std::memset(&p.out, 0, sizeof p.out);
        p.out.accum = sa->accum;
        p.out.acc_a = 1.0f / ((float)sa->first + 1.0f);   // launch_accumulate's a and b, _Sample = first
        p.out.acc_b = 1.0f - p.out.acc_a;
        p.out.rgba8 = sa->rgba8;
        p.out.rgb8 = sa->rgb8;
        p.out.frame_layout = sa->layout == SVO_LAYOUT_FRAME && b.count > 1 ? 1 : 0;
        p.cam.px_off[0] = sa->offsets[0];   // this sample's _PixelOffset
        p.cam.px_off[1] = sa->offsets[1];
        p.shadows = 0;
        L.jittered = true;
        sa = nullptr;
    }
    if (sa) {   // samples in flight: primary rays only, the blend replaces every other output
        // S stack regions of max(slots, 2) x 64 x 8 bytes in one workgroup (svo_kernel.hip)
        const size_t lds = (size_t)std::max(p.slots, 2) * svo::TILE * sizeof(uint2) * (size_t)sa->n;
        if (lds > ctx->lds_per_block)
            return fail(SVO_ERR_ARG, "svo_render_samples: " + std::to_string(sa->n) + " samples of a depth-" +
                                         std::to_string(ctx->depth) + " pool need " + std::to_string(lds) +
                                         " bytes of LDS per workgroup, the device allows " +
                                         std::to_string(ctx->lds_per_block) + ": use fewer samples per launch");
        p.samples = sa->n;
        for (int k = 0; k < sa->n; ++k) {
            p.sample_off[k][0] = sa->offsets[2 * k];
            p.sample_off[k][1] = sa->offsets[2 * k + 1];
            // launch_accumulate's a and b (host float arithmetic), _Sample = first + k
            p.blend_a[k] = 1.0f / ((float)(sa->first + (uint32_t)k) + 1.0f);
            p.blend_b[k] = 1.0f - p.blend_a[k];
        }
        p.accum = sa->accum;
        p.accum8 = sa->rgba8;
        p.accum_rgb8 = sa->rgb8;
        std::memset(&p.out, 0, sizeof p.out);
        p.out.rgba = sa->accum;   // only tells `record` to shade; the samples kernel stores the blend itself
        p.out.frame_layout = sa->layout == SVO_LAYOUT_FRAME && b.count > 1 ? 1 : 0;
        p.shadows = 0;
    }
    return SVO_OK;
}

// The mask scratch: the primary launch writes its tile hit masks to the head of
// d_shadow_list, sized for the hit list a list pass packs behind them.  Shared between the streams
// (order_scratch).
int mask_scratch(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    const size_t need = svo::shadow_list_bytes(p.width, p.local_rows);
    if (ctx->shadow_list_cap < need) {
        HIP_TRY(hipDeviceSynchronize());   // an earlier launch may still read the old list
        const int rc = regrow(&ctx->d_shadow_list, &ctx->shadow_list_cap, need, need);
        if (rc) return rc;
    }
    const int rc = order_scratch(ctx, L.s);
    if (rc) return rc;
    p.out.hitmask = reinterpret_cast<unsigned long long *>(ctx->d_shadow_list);
    return SVO_OK;
}

// The two-pass shadow forms' scratch (shared between the streams: order_scratch).
int shadow_scratch(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    if ((p.shadows == 1 || p.shadows == 3) && !p.out.hits && !p.out.compact) {   // the second pass reads the records
        int rc = ensure_out(ctx, (size_t)(p.out.frame_layout ? p.height : p.local_rows) * (size_t)p.width);
        if (rc) return rc;
        rc = order_scratch(ctx, L.s);
        if (rc) return rc;
        p.out.hits = reinterpret_cast<svo::Hit *>(ctx->d_out_hits);
    }
    // the compacted pass's masks + hit list (ordered like d_out_hits)
    return p.shadows == 3 ? mask_scratch(ctx, L, p) : SVO_OK;
}

bool reflection_on(const svo_ctx *ctx) {
    return ctx->max_bounces > 0 && (ctx->specular[0] != 0.0f || ctx->specular[1] != 0.0f || ctx->specular[2] != 0.0f);
}

// The list passes' inputs (reflection, DESIGN.md 3.2c, and ambient, 3.2e): per hit pixel the record and
// the voxel key -- the caller's outputs where it asked for them, else context-owned scratch -- and the
// mask scratch.  *caller_mask: a caller's own masks, which the primary launch fills where they are and
// the pass copies to the scratch head (copy_caller_mask); null when the masks already lie there (the
// primary launch writes them there for this pass, or the compacted shadow form already made it).
int list_scratch(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p, unsigned long long **caller_mask) {
    int rc;
    const size_t px = (size_t)(p.out.frame_layout ? p.height : p.local_rows) * (size_t)p.width;
    if (!p.out.hits) {
        rc = ensure_out(ctx, px);
        if (rc) return rc;
        p.out.hits = reinterpret_cast<svo::Hit *>(ctx->d_out_hits);
    }
    if (!p.out.voxel) {
        if (ctx->refl_voxel_cap < px) {
            HIP_TRY(hipDeviceSynchronize());   // an earlier launch may still read the old keys
            rc = regrow(&ctx->d_refl_voxel, &ctx->refl_voxel_cap, px, px * sizeof(unsigned long long));
            if (rc) return rc;
        }
        p.out.voxel = ctx->d_refl_voxel;
    }
    unsigned long long *given = p.out.hitmask;
    if (given == reinterpret_cast<unsigned long long *>(ctx->d_shadow_list)) given = nullptr;   // shadow form 2's
    rc = mask_scratch(ctx, L, p);
    if (rc) return rc;
    if (given) p.out.hitmask = given;
    *caller_mask = given;
    return SVO_OK;
}

// A caller's own masks to the scratch head, behind the primary launch that filled them.
int copy_caller_mask(svo_ctx *ctx, LaunchPlan &L, const unsigned long long *caller_mask) {
    if (caller_mask)
        HIP_TRY(hipMemcpyAsync(ctx->d_shadow_list, caller_mask, (size_t)L.n_tiles * sizeof(unsigned long long),
                               hipMemcpyDeviceToDevice, L.s));
    return SVO_OK;
}

// Behind the primary launch: compact its hit pixels and follow each one's specular path.
int reflect_pass(svo_ctx *ctx, LaunchPlan &L, const svo::LaunchParams &p, unsigned long long *caller_mask) {
    const int rc = copy_caller_mask(ctx, L, caller_mask);
    if (rc) return rc;
    svo::ReflectArgs ra;
    std::memset(&ra, 0, sizeof ra);
    ra.scratch = ctx->d_shadow_list;
    for (int k = 0; k < 3; ++k) ra.specular[k] = ctx->specular[k];
    ra.max_bounces = ctx->max_bounces;
    ra.sky = ctx->sky;   // texels null: bounce rays that miss keep the gradient
    const hipError_t e = svo::launch_reflect(p, ra, L.stack_mode, L.s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("reflection launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

bool ambient_on(const svo_ctx *ctx) {
    return ctx->ambient_rays > 0 && (ctx->ambient[0] != 0.0f || ctx->ambient[1] != 0.0f || ctx->ambient[2] != 0.0f);
}

// Behind the primary launch and its shadow pass: compact the hit pixels and add each one's ambient term.
int ambient_pass(svo_ctx *ctx, LaunchPlan &L, const svo::LaunchParams &p, unsigned long long *caller_mask) {
    const int rc = copy_caller_mask(ctx, L, caller_mask);
    if (rc) return rc;
    svo::AmbientArgs aa;
    std::memset(&aa, 0, sizeof aa);
    aa.scratch = ctx->d_shadow_list;
    for (int k = 0; k < 3; ++k) aa.ambient[k] = ctx->ambient[k];
    aa.n_rays = ctx->ambient_rays;
    aa.radius = ctx->ambient_radius;
    aa.variant = (ctx->ambient_variant + ctx->ambient_step) & 7u;
    aa.sky = ctx->sky;   // texels null: open rays take the gradient
    const hipError_t e = svo::launch_ambient(p, aa, L.stack_mode, L.s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("ambient launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

// Behind the primary launch and its shadow pass: compact the hit pixels and add each one's point lights.
int light_pass(svo_ctx *ctx, LaunchPlan &L, const svo::LaunchParams &p, unsigned long long *caller_mask) {
    const int rc = copy_caller_mask(ctx, L, caller_mask);
    if (rc) return rc;
    svo::LightArgs la;
    la.scratch = ctx->d_shadow_list;
    la.lights = ctx->lights;
    la.n_lights = ctx->n_lights;
    const hipError_t e = svo::launch_lights(p, la, L.stack_mode, L.s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("light launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

// The object pass's input: the primary records.  A caller's hits or compact records are
// read (and rewritten) where they are; a launch that asked for neither writes them to context scratch.
int object_scratch(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    if (p.out.hits || p.out.compact) return SVO_OK;
    int rc = ensure_out(ctx, (size_t)(p.out.frame_layout ? p.height : p.local_rows) * (size_t)p.width);
    if (rc) return rc;
    rc = order_scratch(ctx, L.s);
    if (rc) return rc;
    p.out.hits = reinterpret_cast<svo::Hit *>(ctx->d_out_hits);
    return SVO_OK;
}

// Behind the primary launch, before the sky pass: every pixel where a placed object is nearer.  ids: null, or
// id_scratch's bytes for the scene-aware light pass.
int object_pass(svo_ctx *ctx, LaunchPlan &L, const svo::LaunchParams &p, uint8_t *ids) {
    const hipError_t e = svo::launch_objects(p, ctx->objects, ctx->n_objects, L.stack_mode, L.s, ids);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("object launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

// The scene-aware light pass's third input: one byte per pixel, indexed as the launch's
// outputs, shared between the streams like the other list scratch (list_scratch has called order_scratch).
int id_scratch(svo_ctx *ctx, const svo::LaunchParams &p) {
    const size_t px = (size_t)(p.out.frame_layout ? p.height : p.local_rows) * (size_t)p.width;
    if (ctx->object_ids_cap < px) {
        HIP_TRY(hipDeviceSynchronize());   // an earlier launch may still read the old ids
        return regrow(&ctx->d_object_ids, &ctx->object_ids_cap, px, px);
    }
    return SVO_OK;
}

// SVO_OPT_SCENE_SHADOWS, behind the object pass: the directional shadow ray of every hit pixel of the finished
// records, over the terrain and the objects.
int scene_shadow_pass(svo_ctx *ctx, LaunchPlan &L, const svo::LaunchParams &p, unsigned long long *caller_mask) {
    const int rc = copy_caller_mask(ctx, L, caller_mask);
    if (rc) return rc;
    const hipError_t e = svo::launch_scene_shadows(p, ctx->d_shadow_list, ctx->objects, ctx->n_objects, L.stack_mode, L.s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("scene shadow launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

// ... and the point lights, with the scene-light rule and scene-wide occlusion.
int scene_light_pass(svo_ctx *ctx, LaunchPlan &L, const svo::LaunchParams &p, unsigned long long *caller_mask) {
    const int rc = copy_caller_mask(ctx, L, caller_mask);
    if (rc) return rc;
    svo::LightArgs la;
    la.scratch = ctx->d_shadow_list;
    la.lights = ctx->lights;
    la.n_lights = ctx->n_lights;
    const hipError_t e = svo::launch_scene_lights(p, la, ctx->objects, ctx->n_objects, ctx->d_object_ids, L.stack_mode, L.s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("scene light launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

// The sky pass's input: the launch's tile hit masks.  A caller's own masks are read
// where they are; so are shadow form 2's and the reflection pass's, which already made the primary launch
// write them to the head of the shared scratch (their list builds leave the head alone).  Otherwise the
// primary launch writes them there for this pass.
int sky_scratch(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    return p.out.hitmask ? SVO_OK : mask_scratch(ctx, L, p);
}

// Behind the primary launch (and the reflection pass): every miss pixel's colour from the texture.
int sky_pass(svo_ctx *ctx, LaunchPlan &L, const svo::LaunchParams &p) {
    const hipError_t e = svo::launch_sky_fill(p, ctx->sky, p.out.hitmask, L.s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("sky launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

// Cost-ordered dispatch: take the stream's Sched, key this launch's geometry and grow the buffers.
int take_sched(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    const Deal &b = L.b;
    const hipStream_t s = L.s;
    const int n_tiles = L.n_tiles;
    Geo &key = L.key;
    int rc = sched_for(ctx, s, &L.q);
    if (rc) return rc;
    Sched *q = L.q;
    // a new _PixelOffset at the same view (the reference's frame loop draws one every frame,
    // RaytracingMaster.cs:35): the stored segment starts belong to another sub-pixel ray
    if (!p.samples && q->view_prev == ctx->view_gen &&
        (p.cam.px_off[0] != q->off_prev[0] || p.cam.px_off[1] != q->off_prev[1]))
        L.jittered = true;
    // field by field (a hash of overlapping shifted fields could match another geometry
    // and reuse a permutation of a different tile count)
    key.width = p.width;
    key.local_rows = p.local_rows;
    key.rows = b.rows;
    key.rank = b.rank;
    key.count = b.count;
    key.xcd = p.xcd_remap;
    key.n_tiles = n_tiles;
    key.deal = b.key();
    // segmented heavy tiles: primary rays of a tree pool in XCD-strip order
    const int seg_cap = L.seg_cap =
        (ctx->seg_mode || ctx->seg_all) && p.xcd_remap == 2 && !p.guard && p.shadows == 0 && !p.samples && !p.lod
            ? (ctx->seg_all ? (n_tiles + 7) / 8 : ctx->seg_cap) : 0;
    const size_t order_need = svo::order_strips_entries(n_tiles, seg_cap);
    if (!q->side) {
        HIP_TRY(hipStreamCreateWithFlags(&q->side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&q->render_done, hipEventDisableTiming));
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&q->build_ev[i], hipEventDisableTiming));
    }
    if (q->cap < (size_t)n_tiles || q->order_cap < order_need) {
        HIP_TRY(hipStreamSynchronize(s));   // a pending launch on this stream may still use the old buffers
        HIP_TRY(hipStreamSynchronize(q->side));   // ... or an order build
        free_sched(*q);
        const size_t cap = svo::order_cost_capacity(n_tiles);
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(hipMalloc(&q->cost_buf[i], cap * sizeof(uint16_t)));
            HIP_TRY(hipMemset(q->cost_buf[i], 0, cap * sizeof(uint16_t)));
            HIP_TRY(hipMalloc(&q->part_buf[i], svo::SEG_KMAX * cap * sizeof(uint16_t)));
            HIP_TRY(hipMemset(q->part_buf[i], 0, svo::SEG_KMAX * cap * sizeof(uint16_t)));
            HIP_TRY(hipMalloc(&q->order_buf[i], order_need * sizeof(uint32_t)));
        }
        HIP_TRY(hipMalloc(&q->shadow_cost, cap * sizeof(uint16_t)));
        HIP_TRY(hipMemset(q->shadow_cost, 0, cap * sizeof(uint16_t)));
        HIP_TRY(hipMalloc(&q->shadow_order, ((size_t)n_tiles + 36) * sizeof(uint32_t)));
        q->cap = (size_t)n_tiles;
        q->order_cap = order_need;
    }
    if (seg_cap) {
        const size_t px = (size_t)p.width * (size_t)p.local_rows;
        if (q->hint_cap < px) {
            HIP_TRY(hipStreamSynchronize(s));
            rc = regrow(&q->seg_hint, &q->hint_cap, 0, 2 * px * sizeof(float4));   // (the cap once it is filled)
            if (rc) return rc;
            HIP_TRY(hipMemset(q->seg_hint, 0xFF, 2 * px * sizeof(float4)));   // NaN: no starts yet
            q->hint_cap = px;
        }
    }
    if (!q->stats) {
        const size_t words = 16 * Sched::STATS_RING;
        HIP_TRY(hipHostMalloc(&q->stats, words * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped));
        std::memset(q->stats, 0, words * sizeof(uint32_t));
        for (int r = 0; r < Sched::STATS_RING; ++r)
            HIP_TRY(hipEventCreateWithFlags(&q->stats_ev[r], hipEventDisableTiming));
    }
    p.tile_cost = q->cost_buf[q->launches & 1];   // this launch's costs (see Sched)
    p.part_cost = q->part_buf[q->launches & 1];
    if (p.shadows == 1 && ctx->shadow_order_enabled) {
        p.shadow_cost = q->shadow_cost;
        p.shadow_order = q->shadow_key == key ? q->shadow_order : nullptr;
    }
    return SVO_OK;
}

// Loop form (L.latency_bound).  A launch whose total work is small against its heaviest wave -- a strong
// split's per-GPU band, a sky-heavy pose, a lone tile row -- is bound by that wave's serial
// chain, and the latency form (svo_kernel.hip trace_lat: the node kept in the stack entry,
// the next node loaded mid-trip, half the occupancy) runs it faster; a launch that fills
// the chip's wave slots many times over is bound by issue, and the lean loop's full
// occupancy wins.  Measured: latency form faster when the wave trips T
// (sum over tiles) and heaviest tile M satisfy T < 0.3 * slots * M, slots = the lean
// loop's resident waves on the chip.  T and M come from the order kernel of the last
// COMPLETED order build at this geometry (stats_ev; the host may be many launches ahead
// of the GPU).  Decisions of an earlier view are kept while the camera moves (one launch
// per view: the last frame's costs); once a build for the current view is in flight --
// the second launch after a move -- the host waits for it (once per view), so a jump to
// a different pose is never rendered with another pose's choice.
// The costs (and so the decision) are keyed on the render mode too: a shadowed launch's
// tile costs include its shadow trips.  The wait can block the host for up to a frame,
// once per new view (svo_rt.h, svo_render_device).
// The same statistics decide whether the heaviest tiles are traced as segmented rays
// (segments on: exactly when the launch is latency-bound, i.e. its heaviest chain and not
// its issued work bounds it -- a strong split's band).
int decide_loop_form(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    Sched *q = L.q;
    const Geo &key = L.key;
    const int mode_now = L.mode_now;
    p.lat = 0;
    const bool have_order = q && [&] { Geo g = q->order_key; g.seg = g.kpack = 0; return g == key; }();
    if (!p.guard && p.shadows == 0 && !L.instr && !p.samples && !p.lod && (ctx->lat_mode != 0 || L.seg_cap)) {
        if (ctx->lat_mode == 1) {
            L.latency_bound = true;
        } else if (q && q->stats && have_order) {
            // the newest pending build first: wait for it if it is this view's and this view has
            // no decision yet (once per view), else take the newest build that has completed
            // (stream order: then every older one has too) and drop the older ones
            const bool decided = q->lat_key == key && q->lat_view == ctx->view_gen && q->lat_mode == mode_now;
            for (int i = 1; i <= Sched::STATS_RING; ++i) {
                const int r = (q->stats_head + Sched::STATS_RING - i) % Sched::STATS_RING;
                if (!q->stats_pending[r]) continue;
                const bool wait = i == 1 && !decided && q->stats_key[r] == key && q->stats_view[r] == ctx->view_gen &&
                                  q->stats_mode[r] == mode_now;
                const hipError_t st = wait ? hipEventSynchronize(q->stats_ev[r]) : hipEventQuery(q->stats_ev[r]);
                if (st == hipErrorNotReady) continue;
                if (st != hipSuccess) return fail(SVO_ERR_HIP, std::string("order build event: ") + hipGetErrorString(st));
                for (int j = i; j <= Sched::STATS_RING; ++j)   // r and every older build (newer ones stay pending)
                    q->stats_pending[(q->stats_head + Sched::STATS_RING - j) % Sched::STATS_RING] = false;
                if (q->stats_key[r] == key && q->stats_mode[r] == mode_now) {
                    const svo_sched::Stats tm = svo_sched::reduce_stats(q->stats + 16 * r);
                    const double slots = svo_sched::lean_slots(ctx->num_cus, (size_t)p.slots * svo::TILE * sizeof(uint2));
                    // with beam starts the rule picks only the class table (the loop stays lean); measured
                    // boundary 0.28: C3 bands at N = 2 (flyover 0.18, terrain-facing 0.23, Main.unity 0.27)
                    // run faster with the latency table, the flyover frame (0.30, 0.30-0.33 panning),
                    // terrain-facing (0.45) and Main.unity (0.49) with the issue table
                    const double ratio = L.beam_planned ? ctx->seg_ratio : ctx->lat_ratio;
                    // hysteresis of 15 % around it once this geometry and mode have a decision: costs
                    // measured under one class table (or with jittered rays) move T a little, and a
                    // flip near the boundary costs more than either table (the next launches find no
                    // order built for the other table's class layout)
                    const bool prior = q->lat_key == q->stats_key[r] && q->lat_mode == q->stats_mode[r];
                    // thin: far fewer summed trips than resident slots x the heaviest chain (a band of an 8-way
                    // split): the chain alone bounds the launch and eight segments shorten it most.  No
                    // hysteresis: the second build at a new geometry reads costs of the fallback order's
                    // layout (C3 Main.unity 8-way band: 0.118 once, 0.079 from then on), and a sticky
                    // decision would keep that transient (0.0417 ms against 0.0378 with eighths)
                    const svo_sched::LoopForm f = svo_sched::loop_form(tm.T, tm.M, slots, ratio, ctx->thin_ratio,
                                                                       ctx->seg_min_chain, prior, q->lat_cache != 0);
                    q->lat_cache = f.lat ? 1 : 0;
                    q->lat_short = f.is_short;
                    q->lat_thin = f.thin;
                    q->lat_key = q->stats_key[r];
                    q->lat_view = q->stats_view[r];
                    q->lat_mode = q->stats_mode[r];
                    if (ctx->debug & 1)   // diagnostics (SVO_DEBUG bit 0): the decision and its inputs
                        std::fprintf(stderr, "svo lat: view %llu T %llu M %u slots %.0f ratio %.6f bound %.6f thin %.6f "
                                     "beam %d -> %s%s\n", q->lat_view, (unsigned long long)tm.T, tm.M, slots,
                                     tm.M ? (double)tm.T / (slots * (double)tm.M) : 0.0, f.bound, (double)ctx->thin_ratio,
                                     L.beam_planned ? 1 : 0, q->lat_cache ? "latency" : "lean", q->lat_thin ? " thin" : "");
                }
                break;
            }
            L.latency_bound = q->lat_key == key && q->lat_mode == mode_now && q->lat_cache;
        }
    }
    return SVO_OK;
}

// The order this launch dispatches in (with segmented heavy tiles if so decided): the class table it
// asks for (L.okey) and which of the two built orders it takes.
int choose_order(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    Sched *q = L.q;
    Geo &okey = L.okey;
    okey = L.key;
    // a latency-bound launch whose heaviest chain is short (C1, C2: 76 and 111 trips) runs faster in
    // the latency form without segments or beam starts (C2 0.041 against 0.047 ms, C1 0.025 / 0.031)
    const svo_sched::ClassTable ct =
        svo_sched::class_table(ctx->seg_all, L.seg_cap, L.latency_bound, q->lat_short, q->lat_thin, L.jittered,
                               ctx->seg_jitter, ctx->seg_kpack_lat, ctx->seg_kpack_issue, ctx->seg_kpack_thin);
    okey.kpack = ct.kpack;
    okey.seg = ct.seg;
    // the newest build it follows by >= 2 launches (Sched): a build that launch n - 2 was
    // followed by read the cost buffer this launch writes, so it is waited for whatever its key
    const long long n = (long long)q->launches;
    for (int i = 0; i < 2; ++i) {
        if (q->build_at[i] < 0 || q->build_at[i] > n - 2 || q->build_seen[i]) continue;
        const hipError_t st = hipEventQuery(q->build_ev[i]);
        if (st == hipErrorNotReady) HIP_TRY(hipStreamWaitEvent(L.s, q->build_ev[i], 0));
        else if (st != hipSuccess) return fail(SVO_ERR_HIP, std::string("order build: ") + hipGetErrorString(st));
        q->build_seen[i] = true;
    }
    const int use = svo_sched::pick_build(n, q->build_at, q->build_key, okey, L.key);
    p.tile_order = use >= 0 ? q->order_buf[use] : nullptr;
    if (ctx->debug & 2)   // diagnostics (SVO_DEBUG bit 1): the order and class table each launch takes
        std::fprintf(stderr, "svo order: launch %lld view %llu latency %d kpack %x use %d built_at %lld/%lld keys %d/%d\n",
                     n, ctx->view_gen, (int)L.latency_bound, okey.kpack, use, q->build_at[0], q->build_at[1],
                     (int)(q->build_key[0] == okey), (int)(q->build_key[1] == okey));
    const Geo &bk = use >= 0 ? q->build_key[use] : okey;   // the class layout the order was built with
    L.used_kpack = bk.kpack;
    if (p.tile_order && bk.seg) {   // the order lists part entries: the segmented kernel
        p.seg = bk.seg;
        p.seg_kmax = svo::seg_kmax_of(bk.kpack);
        const bool even = (L.jittered && ctx->seg_jitter == 2) || (q->view_prev != ctx->view_gen && ctx->seg_move == 2);
        p.seg_hint = even ? nullptr : q->seg_hint;
        if (ctx->seg_scramble) p.seg_scramble = ctx->seg_scramble * 0x9E3779B9u + ++ctx->seg_launches;
    }
    return SVO_OK;
}

// The per-wave record's buffer (diagnostics: SVO_WAVE_LOG; dumped after the launch, finish_launch).
int wave_log_buffer(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    // one record per workgroup: the tile kernel's grid, or the segmented kernel's (its part entries)
    const size_t n_wave = L.n_wave = p.seg ? (size_t)svo::order_strips_grid(L.n_tiles, p.seg, p.seg_kmax) : (size_t)L.n_tiles;
    if (!ctx->wave_log_path.empty() && !L.instr) {
        if (ctx->wave_log_cap < n_wave) {
            HIP_TRY(hipDeviceSynchronize());
            int rc = regrow(&ctx->d_wave_log, &ctx->wave_log_cap, n_wave, n_wave * 4 * svo::WAVE_LOG_WORDS);
            if (rc) return rc;
        }
        HIP_TRY(hipMemsetAsync(ctx->d_wave_log, 0, n_wave * 4 * svo::WAVE_LOG_WORDS, L.s));
        p.wave_log = ctx->d_wave_log;
    }
    return SVO_OK;
}

// Beam starts: a tree pool's primary rays start at a per-tile lower bound of
// their hit t, splatted from the pool's boxes right before the render, on its stream.  The
// bounds are a function of the camera matrices, the pool and the frame size only (pixel offsets
// in [0, 1] are covered), so a launch at the view of this stream's previous one reuses them --
// a held view (the reference's accumulating camera) splats once; a moving camera every frame.
int beam_starts(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    Sched *q = L.q;
    const hipStream_t s = L.s;
    const int width = p.width, height = p.height;
    int rc;
    // an instrumented launch with the beam: SVO_OPT_COUNT_BEAM's fetch count, or svo_beam_starts
    const bool count_beam = (p.out.fetches && (ctx->options & SVO_OPT_COUNT_BEAM)) || p.out.starts;
    if (ctx->beam && (q || count_beam) && !p.guard && (!L.instr || count_beam) && ctx->depth_exact && !p.lat) {
        auto in01 = [](float v) { return v >= 0.0f && v <= 1.0f; };
        bool offs = in01(p.cam.px_off[0]) && in01(p.cam.px_off[1]);
        if (p.samples) {
            offs = true;
            for (int k = 0; k < p.samples; ++k) offs = offs && in01(p.sample_off[k][0]) && in01(p.sample_off[k][1]);
        }
        svo::BeamParams bp;
        std::memset(&bp, 0, sizeof bp);
        const int tx = (width + 7) / 8, ty = (height + 7) / 8, sx = (width + 63) / 64, sy = (height + 63) / 64;
        const size_t need = (size_t)tx * ty + (size_t)sx * sy + 1;
        // the stream's own buffer; an instrumented launch (no scheduling state) the shared scratch
        unsigned long long *&buf = q ? q->tile_start : ctx->count_ts;
        size_t &cap = q ? q->ts_cap : ctx->count_ts_cap;
        uint32_t &gen = q ? q->ts_gen : ctx->count_ts_gen;
        // A new view splats the moving camera's list; the view's next launch on this stream (a held
        // view: the reference's accumulating camera, the drop-in's jittered frames) re-splats once with
        // the finer held list and every later one reuses that.  An instrumented launch (the fetch count
        // of the walk the render runs, svo_beam_starts) takes the held list.
        const bool same_view = q && q->ts_view == ctx->view_gen && q->ts_w == width && q->ts_h == height &&
                               cap >= need && gen != 0;
        const int li = !q || same_view ? 1 : 0;
        const std::shared_ptr<const std::vector<uint2>> &boxes = li ? ctx->pool_boxes_held : ctx->pool_boxes;
        const uint64_t bid = li ? ctx->pool_boxes_held_id : ctx->pool_boxes_id;
        DevBoxes &db = ctx->dev_boxes[li];
        // a LOD launch: no start may pass the floor of the list it splats (svo_lod.h lod_floor);
        // -inf: nothing to gain, no splat and no beam starts
        const float floor = p.lod ? svo_lod::lod_floor((double)p.lod_coef, (double)p.lod_bias,
                                                         li ? ctx->pool_boxes_held_fine : ctx->pool_boxes_fine)
                                  : std::numeric_limits<float>::infinity();
        if (boxes && !boxes->empty() && offs && !(floor < 0.0f) && beam_camera(p.cam, width, height, &bp)) {
            p.lod_floor = floor;
            if (db.id != bid) {   // the device copy of this splat list
                const size_t nb = boxes->size();
                HIP_TRY(hipDeviceSynchronize());   // launches on any stream may still read the old one
                if (db.cap < nb) {
                    rc = regrow(&db.d, &db.cap, nb, nb * sizeof(uint2));
                    if (rc) return rc;
                }
                HIP_TRY(hipMemcpy(db.d, boxes->data(), nb * sizeof(uint2), hipMemcpyHostToDevice));
                db.n = (uint32_t)nb;
                db.id = bid;
            }
            if (!q) {
                rc = order_scratch(ctx, s);
                if (rc) return rc;
            }
            const bool reuse = same_view && q->ts_boxes == bid;
            if (!reuse && (cap < need || gen == 0xFFFFFFFEu)) {   // (re)filled with all-ones keys: generation 0, stale
                HIP_TRY(hipDeviceSynchronize());   // a pending launch may still read the old buffer
                if (cap < need) {
                    rc = regrow(&buf, &cap, need, need * sizeof(unsigned long long));
                    if (rc) return rc;
                }
                HIP_TRY(hipMemset(buf, 0xFF, cap * sizeof(unsigned long long)));
                gen = 0;
            }
            if (!reuse) ++gen;
            bp.boxes = db.d;
            bp.n_boxes = db.n;
            bp.tile_start = buf;
            bp.gen = gen;
            bp.diag = ctx->beam_diag;   // timing diagnostics only
            bp.tiles_x = tx;
            bp.tiles_y = ty;
            bp.super_x = sx;
            bp.super_y = sy;
            bp.super_off = tx * ty;
            bp.global_off = tx * ty + sx * sy;
            bp.width = width;
            bp.height = height;
            if (!reuse) {
                hipError_t eb = svo::launch_beam_splat(bp, s);
                if (eb != hipSuccess) return fail(SVO_ERR_HIP, std::string("beam splat launch: ") + hipGetErrorString(eb));
                if (q) {
                    q->held_splat = li == 1;
                    q->ts_view = ctx->view_gen;
                    q->ts_boxes = bid;
                    q->ts_w = width;
                    q->ts_h = height;
                }
            }
            p.tile_start = buf;
            p.ts_gen = gen;
            p.ts_tiles_x = tx;
            p.ts_super_x = sx;
            p.ts_super_off = bp.super_off;
            p.ts_global_off = bp.global_off;
        }
    }
    return SVO_OK;
}

// The render launch itself, and behind it -- by the refresh rule -- the build of the order of the
// launch after next, on the side stream.
int render_and_reorder(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    Sched *q = L.q;
    const hipStream_t s = L.s;
    const Geo &key = L.key, &okey = L.okey;
    const int mode_now = L.mode_now;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (!L.instr) {
        int rc = take_events(ctx, STAGE_KERNEL, &ev0, &ev1);
        if (rc) return rc;
    }
    hipError_t e = svo::launch_render(p, L.stack_mode, s, ev0, ev1);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("render launch: ") + hipGetErrorString(e));
    // refresh: a new geometry, every order_every-th launch while costs can drift, a change of
    // render mode, and a camera move -- right after the first launch at a view the camera then
    // holds (that launch still uses the old order, a permutation of the same tiles, placement
    // only, and records fresh costs), but while the camera moves every launch only every
    // move_every-th launch: each build is an order kernel plus an event on the render stream, and
    // the last few frames' costs order a slowly moving view almost as well as its own
    bool refresh = false;
    bool moving_build = false;   // the build follows a launch at a new view (a moving camera)
    if (q && p.tile_cost) {
        const unsigned long long n = q->launches++;   // (p.tile_cost is cost_buf[n % 2])
        const bool moving = q->view_prev != ctx->view_gen;   // a new view since this stream's last launch
        q->view_prev = ctx->view_gen;
        q->off_prev[0] = p.cam.px_off[0];
        q->off_prev[1] = p.cam.px_off[1];
        // the periodic rebuild only when costs can have changed without a new view (a jittered
        // pixel offset, a new light or pool, per-launch sample offsets): a held view with nothing
        // else changed records the same costs every launch, so its order stays exact
        const bool drift = q->built_cost != ctx->cost_gen || p.samples != 0 || L.jittered;
        // a launch dispatched in an order of another class layout (the first at a new class table)
        // recorded its costs under that layout: the next build at this table comes from a launch in
        // its own layout (C3 N = 2 band: 0.059 ms with the first build kept, 0.050 with its own)
        const bool relayout = svo_sched::other_layout(ctx->relayout != 0, p.tile_order != nullptr, p.seg, p.seg_kmax, L.used_kpack,
                                                      okey.seg, svo::seg_kmax_of(okey.kpack), okey.kpack);
        if (relayout) q->relayout_pending = true;
        const bool own_layout = !relayout && q->relayout_pending;
        // (a held view's finer re-splat shortens its rays: the order is rebuilt from that launch's costs)
        refresh = svo_sched::needs_refresh(q->order_key != okey, n, ctx->order_every, drift, q->built_mode != mode_now, own_layout,
                                           q->held_splat, q->built_view != ctx->view_gen, moving, n - q->last_build,
                                           ctx->move_every);
        q->held_splat = false;
        if (own_layout) q->relayout_pending = false;
        if (refresh) q->last_build = n;
        moving_build = moving;
    }
    if (refresh) {   // the launch after next at this geometry dispatches the heaviest tiles first
        const int r = q->stats_head;
        uint32_t *st16 = q->stats ? q->stats + 16 * r : nullptr;
        const int bi = q->next_buf;
        q->next_buf ^= 1;
        // on the side stream, behind this launch (its costs; and every launch that read buffer bi)
        HIP_TRY(hipEventRecord(q->render_done, s));
        HIP_TRY(hipStreamWaitEvent(q->side, q->render_done, 0));
        e = p.xcd_remap == 2 ? svo::launch_order_strips(p.tile_cost, q->order_buf[bi], L.n_tiles, (p.width + 7) / 8, q->side,
                                                        st16, okey.seg, p.part_cost, okey.kpack,
                                                        moving_build && ctx->spread ? 1 : 0)
                             : svo::launch_order_tiles(p.tile_cost, q->order_buf[bi], L.n_tiles, q->side, st16);
        if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("tile order launch: ") + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(q->build_ev[bi], q->side));
        q->build_at[bi] = (long long)q->launches - 1;   // launches was incremented above
        q->build_seen[bi] = false;
        q->build_key[bi] = okey;
        q->order_key = okey;
        q->built_view = ctx->view_gen;
        q->built_cost = ctx->cost_gen;
        q->built_mode = mode_now;
        if (st16) {   // slot r: a build still pending there (ring full) is simply superseded
            HIP_TRY(hipEventRecord(q->stats_ev[r], q->side));
            q->stats_pending[r] = true;
            q->stats_key[r] = key;
            q->stats_view[r] = ctx->view_gen;
            q->stats_mode[r] = mode_now;
            q->stats_head = (r + 1) % Sched::STATS_RING;
        }
    }
    return SVO_OK;
}

// Behind the launch: the two-pass shadow form's own order, and the wave log's dump.
int finish_launch(svo_ctx *ctx, LaunchPlan &L, svo::LaunchParams &p) {
    Sched *q = L.q;
    const hipStream_t s = L.s;
    const Geo &key = L.key;
    if (q && p.shadow_cost && (q->shadow_key != key || q->shadow_launches++ % ctx->order_every == 0)) {
        hipError_t e = p.xcd_remap == 2
                           ? svo::launch_order_strips(q->shadow_cost, q->shadow_order, L.n_tiles, (p.width + 7) / 8, s)
                           : svo::launch_order_tiles(q->shadow_cost, q->shadow_order, L.n_tiles, s);
        if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("shadow order launch: ") + hipGetErrorString(e));
        q->shadow_key = key;
    }
    if (p.wave_log) {   // blocking dump of the last launch's per-wave record
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<uint32_t> h(L.n_wave * svo::WAVE_LOG_WORDS);
        HIP_TRY(hipMemcpy(h.data(), ctx->d_wave_log, h.size() * 4, hipMemcpyDeviceToHost));
        if (FILE *f = std::fopen(ctx->wave_log_path.c_str(), "wb")) {
            std::fwrite(h.data(), 4 * svo::WAVE_LOG_WORDS, L.n_wave, f);
            std::fclose(f);
        }
    }
    return SVO_OK;
}

// One render launch (every entry point's, and each member's of a multi-device frame): its phases.
int launch(svo_ctx *ctx, int width, int height, int stack_mode, const svo_band *band, svo::Outputs out,
           hipStream_t stream, const SampleArgs *sa = nullptr) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
    if ((size_t)width * (size_t)height > ((size_t)1 << 31)) return fail(SVO_ERR_ARG, "frame larger than 2^31 pixels");
    if (stack_mode != SVO_STACK_HLSL && stack_mode != SVO_STACK_EXACT)
        return fail(SVO_ERR_ARG, "unknown stack mode");
    if (ctx->n_nodes == 0) return fail(SVO_ERR_STATE, "no node pool uploaded (svo_set_buffer)");
    if (!ctx->cam_set) return fail(SVO_ERR_STATE, "camera not set (svo_set_camera)");
    // level of detail (svo_set_lod) applies to every launch's primary rays but svo_beam_starts' diagnostics
    const bool lod = (ctx->lod_coef != 0.0f || ctx->lod_bias != 0.0f) && !out.starts;
    if (lod && (ctx->options & SVO_OPT_SHADOW_RAYS))
        return fail(SVO_ERR_STATE, "shadow rays with LOD are not supported");
    // reflection bounces (svo_set_reflection): a second pass behind every render launch's primary rays; the
    // instrumented launches (svo_count_fetches, svo_beam_starts) trace primary rays only
    const bool refl_on = reflection_on(ctx) && !out.fetches && !out.starts;
    if (refl_on && sa) return fail(SVO_ERR_STATE, "svo_render_samples with reflection is not supported");
    if (refl_on && (ctx->options & SVO_OPT_SHADOW_RAYS))
        return fail(SVO_ERR_STATE, "shadow rays with reflection are not supported");
    if (refl_on && lod) return fail(SVO_ERR_STATE, "reflection with LOD is not supported");
    // ambient term (svo_set_ambient): a pass behind the primary rays and their shadow pass
    const bool amb_on = ambient_on(ctx) && !out.fetches && !out.starts;
    if (amb_on && sa) return fail(SVO_ERR_STATE, "svo_render_samples with an ambient term is not supported");
    if (amb_on && refl_on) return fail(SVO_ERR_STATE, "an ambient term with reflection is not supported");
    if (amb_on && lod) return fail(SVO_ERR_STATE, "an ambient term with LOD is not supported");
    // point lights (svo_set_lights): a pass behind the primary rays and their shadow pass
    const bool lights_on = ctx->n_lights > 0 && !out.fetches && !out.starts;
    if (lights_on && sa) return fail(SVO_ERR_STATE, "svo_render_samples with lights is not supported");
    if (lights_on && refl_on) return fail(SVO_ERR_STATE, "lights with reflection are not supported");
    if (lights_on && lod) return fail(SVO_ERR_STATE, "lights with LOD are not supported");
    if (lights_on && amb_on) return fail(SVO_ERR_STATE, "lights with an ambient term are not supported");
    // placed objects (svo_set_objects): a pass behind the primary rays that takes every pixel where an object
    // is nearer; of the other passes only the shadow and the light pass know the objects, and only with
    // SVO_OPT_SCENE_SHADOWS
    const bool objects_on = ctx->n_objects > 0 && !out.fetches && !out.starts;
    const bool scene_opt = (ctx->options & SVO_OPT_SCENE_SHADOWS) != 0;
    if (objects_on && sa) return fail(SVO_ERR_STATE, "svo_render_samples with objects is not supported");
    if (objects_on && !scene_opt && (ctx->options & SVO_OPT_SHADOW_RAYS))
        return fail(SVO_ERR_STATE, "objects with shadow rays are not supported");
    if (objects_on && refl_on) return fail(SVO_ERR_STATE, "objects with reflection are not supported");
    if (objects_on && amb_on) return fail(SVO_ERR_STATE, "objects with an ambient term are not supported");
    if (objects_on && !scene_opt && lights_on) return fail(SVO_ERR_STATE, "objects with lights are not supported");
    if (objects_on && lod) return fail(SVO_ERR_STATE, "objects with LOD are not supported");
    // skybox (svo_set_skybox): a pass behind the primary rays (and the bounces) that recolours the misses;
    // svo_render_samples blends in its own launch's epilogue, before any pass could run
    const bool sky_on = ctx->sky.texels && !out.fetches && !out.starts;
    if (sky_on && sa) return fail(SVO_ERR_STATE, "svo_render_samples with a skybox texture is not supported");
    LaunchPlan L;
    L.stack_mode = stack_mode;
    int rc = check_band(band, height, &L.b);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    svo::LaunchParams p;
    base_params(ctx, L, width, height, out, p);
    // a LOD launch takes the LOD kernels: no segmented tiles and no latency form whatever svo_config
    // says (take_sched, decide_loop_form), beam starts floored (beam_starts)
    p.lod = lod ? 1 : 0;
    p.lod_coef = lod ? ctx->lod_coef : 0.0f;
    p.lod_bias = lod ? ctx->lod_bias : 0.0f;
    p.lod_floor = std::numeric_limits<float>::infinity();
    rc = sample_forms(ctx, L, p, sa);
    if (rc) return rc;
    if (p.shadows == 3 && out.hitmask) p.shadows = 1;   // the caller's masks are not a list scratch
    if (p.local_rows == 0) return SVO_OK;
    L.instr = out.fetches || out.starts;
    if (L.instr) p.shadows = 0;
    // objects in shadow and light: the primary launch takes the path it takes with neither (no fused shadows,
    // whatever shadow_form says), and both passes run behind the object pass on the finished records
    const bool scene_shadows = objects_on && (ctx->options & SVO_OPT_SHADOW_RAYS) != 0;
    if (scene_shadows) p.shadows = 0;
    L.s = stream ? stream : ctx->stream;
    rc = shadow_scratch(ctx, L, p);
    if (rc) return rc;
    // only the colours change: a launch that writes none has no reflection pass
    const bool reflect = refl_on && (p.out.rgba || p.out.rgba8 || p.out.rgb8);
    unsigned long long *caller_mask = nullptr;
    const bool ambient = amb_on && (p.out.rgba || p.out.rgba8 || p.out.rgb8);
    const bool lights = lights_on && (p.out.rgba || p.out.rgba8 || p.out.rgb8);
    const bool scene_lights = objects_on && lights;
    if (reflect || ambient || lights || scene_shadows) {   // of the first three never two (refused above)
        rc = list_scratch(ctx, L, p, &caller_mask);
        if (rc) return rc;
    }
    if (scene_lights) {
        rc = id_scratch(ctx, p);
        if (rc) return rc;
    }
    if (objects_on) {   // the records change too: every launch has the pass
        rc = object_scratch(ctx, L, p);
        if (rc) return rc;
    }
    // the same for the sky pass: only a launch that writes a colour has one
    const bool sky = sky_on && (p.out.rgba || p.out.rgba8 || p.out.rgb8);
    if (sky) {
        rc = sky_scratch(ctx, L, p);
        if (rc) return rc;
    }
    p.prio = ctx->prio;
    L.n_tiles = ((width + 7) / 8) * ((p.local_rows + 7) / 8);
    if (ctx->tile_order && !L.instr) {
        rc = take_sched(ctx, L, p);
        if (rc) return rc;
    }
    L.mode_now = p.shadows | (stack_mode << 2);
    // whether this launch's primary rays get beam starts (beam_starts' test, less the per-launch camera checks)
    L.beam_planned = ctx->beam && L.q && !p.guard && !L.instr && ctx->depth_exact && ctx->pool_boxes &&
                     !ctx->pool_boxes->empty();
    rc = decide_loop_form(ctx, L, p);
    if (rc) return rc;
    if (L.q) {
        rc = choose_order(ctx, L, p);
        if (rc) return rc;
    }
    // with segmented tiles the whole tiles keep the lean loop: the latency form's doubled LDS halves
    // the resident waves of the quarters too (C3 flyover bands, profiles/r05b_seg_ab.json: N = 2
    // 0.0804 ms with it against 0.0629 without, N = 4 0.0500 / 0.0457, N = 8 0.0388 / 0.0395)
    p.lat = L.latency_bound && ctx->lat_mode != 0 && (!p.seg || ctx->lat_mode == 1) ? 1 : 0;
    rc = wave_log_buffer(ctx, L, p);
    if (rc) return rc;
    rc = beam_starts(ctx, L, p);
    if (rc) return rc;
    rc = render_and_reorder(ctx, L, p);
    if (rc) return rc;
    if (reflect) {
        rc = reflect_pass(ctx, L, p, caller_mask);
        if (rc) return rc;
    }
    if (ambient) {
        rc = ambient_pass(ctx, L, p, caller_mask);
        if (rc) return rc;
    }
    if (lights && !scene_lights) {
        rc = light_pass(ctx, L, p, caller_mask);
        if (rc) return rc;
    }
    if (objects_on) {
        rc = object_pass(ctx, L, p, scene_lights ? ctx->d_object_ids : nullptr);
        if (rc) return rc;
    }
    if (scene_shadows) {
        rc = scene_shadow_pass(ctx, L, p, caller_mask);
        if (rc) return rc;
    }
    if (scene_lights) {
        rc = scene_light_pass(ctx, L, p, caller_mask);
        if (rc) return rc;
    }
    if (sky) {
        rc = sky_pass(ctx, L, p);
        if (rc) return rc;
    }
    return finish_launch(ctx, L, p);
}

// Enqueue the assemble kernel on this context's device (svo_assemble_frame, and
// the gather of a multi-device frame).
int assemble(svo_ctx *ctx, int width, int height, const Deal &deal, int n_parts, const void *const *parts,
             int part_format, int skip_part, const svo::Outputs &out, hipStream_t s) {
    svo::AssembleParams a;
    std::memset(&a, 0, sizeof a);
    a.att = ctx->d_att;
    a.n_nodes = (uint32_t)std::min<size_t>(ctx->n_nodes, 0xFFFFFFFFu);
    a.cam = ctx->cam;
    a.width = width;
    a.height = height;
    a.band_rows = deal.rows;
    a.n_parts = n_parts;
    a.cycle = deal.cycle;
    for (int i = 0; i < deal.cycle; ++i) {
        const int m = deal.owner[i];
        a.owner[i] = (uint8_t)m;
        a.idx[i] = (uint8_t)a.cnt[m]++;
    }
    a.part_format = part_format;
    a.skip_part = skip_part;
    for (int i = 0; i < n_parts; ++i) a.parts[i] = parts[i];
    a.out = out;
    a.out.frame_layout = 1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int rc = take_events(ctx, STAGE_ASSEMBLE, &ev0, &ev1);
    if (rc) return rc;
    if (ev0) HIP_TRY(hipEventRecord(ev0, s));
    if (part_format == SVO_PART_SPARSE_RGB8) {   // the parts' tile counts (their offsets travel in them)
        const int tiles_x = (width + 7) / 8;
        for (int m = 0; m < n_parts; ++m) {
            Deal dm = deal;
            dm.rank = m;
            a.n_tiles[m] = (uint32_t)(tiles_x * ((band_rows_local(height, dm) + 7) / 8));
        }
    }
    hipError_t e = svo::launch_assemble(a, s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("assemble launch: ") + hipGetErrorString(e));
    if (ev1) HIP_TRY(hipEventRecord(ev1, s));
    return SVO_OK;
}

int check_assemble_args(svo_ctx *ctx, int width, int height, int n_parts, int part_format, int skip_part,
                        const svo::Outputs &o) {
    if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
    if (n_parts < 1 || n_parts > svo::MAX_PARTS) return fail(SVO_ERR_ARG, "n_parts must be in [1, 64]");
    if (skip_part < -1 || skip_part >= n_parts) return fail(SVO_ERR_ARG, "skip_part out of range");
    if (o.position || o.voxel || o.fetches) return fail(SVO_ERR_ARG, "position / voxel outputs are not assembled");
    if (o.rgb8 || o.hitmask) return fail(SVO_ERR_ARG, "the assembled frame is RGBA8 (rgb8 / hitmask are band payloads)");
    if (part_format == SVO_PART_RGBA8 || part_format == SVO_PART_RGB8 || part_format == SVO_PART_SPARSE_RGB8) {
        if (!o.rgba8 || o.hits || o.rgba || o.compact)
            return fail(SVO_ERR_ARG, "RGBA8 / RGB8 / sparse parts rebuild only an RGBA8 frame");
        if (part_format == SVO_PART_SPARSE_RGB8 && !ctx->cam_set)
            return fail(SVO_ERR_STATE, "camera not set (svo_set_camera): sparse parts need it for the sky");
    } else if (part_format == SVO_PART_COMPACT) {
        if ((o.hits || o.rgba || o.rgba8) && ctx->n_nodes == 0)
            return fail(SVO_ERR_STATE, "no node pool uploaded: compact parts need the SVO replica");
        if ((o.rgba || o.rgba8) && !ctx->cam_set) return fail(SVO_ERR_STATE, "camera not set (svo_set_camera)");
    } else {
        return fail(SVO_ERR_ARG, "unknown part format");
    }
    return SVO_OK;
}

// ------------------------------------------------------ multi-device frame
// sa (svo_render_samples): every member traces S samples of its bands and blends them into its
// own band accumulation (the display member into the caller's frame-layout accum); the members'
// payloads are the blended bands' 3-byte RGB, assembled into the caller's rgba8 frame.
int multi_render(svo_ctx *ctx, int width, int height, int stack_mode, const svo_frame *frame, hipStream_t stream,
                 const SampleArgs *sa = nullptr) {
    const int n = (int)ctx->members.size();
    svo::Outputs out = outputs_of(frame);
    out.frame_layout = 1;
    if (out.position || out.voxel) return fail(SVO_ERR_ARG, "position / voxel outputs are not gathered across devices");
    if (out.rgb8 || out.hitmask) return fail(SVO_ERR_ARG, "a multi-device frame is assembled as rgba8, not rgb8 / hitmask");
    if (!out.hits && !out.rgba && !out.rgba8 && !out.compact) return fail(SVO_ERR_ARG, "no output requested");
    // display-only frames travel as 3-byte RGB (the RGBA8 word without its constant alpha), or
    // (SVO_SPARSE_PAYLOAD=1) as sparse parts: tile hit masks + offsets + the hits' RGB, pulled by the
    // assemble kernel with no host round trip (the offsets travel in the part)
    const int fmt = sa ? SVO_PART_RGB8
                    : (out.hits || out.rgba || out.compact) ? SVO_PART_COMPACT
                    : ctx->sparse_payload ? SVO_PART_SPARSE_RGB8 : SVO_PART_RGB8;
    const size_t elem = fmt == SVO_PART_COMPACT ? 12 : 3;
    // the band accumulations hold the rows of the deal they were blended under: a continued
    // accumulation (first sample > 0) under another deal would blend into other members' rows
    uint64_t dkey = 1469598103934665603ull ^ (uint64_t)n ^ ((uint64_t)ctx->band_rows << 16);
    for (int i = 0; i < ctx->deal_cycle; ++i) dkey = (dkey ^ ctx->deal_owner[i]) * 1099511628211ull;
    dkey ^= (uint64_t)ctx->deal_cycle << 40;
    if (sa) {
        if (sa->first > 0 && ctx->samples_deal_set && ctx->samples_deal != dkey)
            return fail(SVO_ERR_STATE, "the band deal changed since the last svo_render_samples: restart the "
                                       "accumulation at first_sample 0");
        ctx->samples_deal = dkey;
        ctx->samples_deal_set = true;
    }
    const int k = ctx->parity;
    ctx->parity ^= 1;
    svo_ctx *m0 = ctx->members[0];
    hipStream_t s0 = stream ? stream : m0->stream;
    // the display device renders its own bands straight into the caller's frame
    svo_band b0{ctx->band_rows, 0, n, ctx->deal_cycle, ctx->deal_cycle ? ctx->deal_owner : nullptr};
    int rc = launch(m0, width, height, stack_mode, &b0, out, s0, sa);
    if (rc) return rc;
    std::vector<const void *> parts(n, nullptr);
    for (int i = 1; i < n; ++i) {
        svo_ctx *m = ctx->members[i];
        Peer &pr = ctx->peers[i];
        svo_band bi{ctx->band_rows, i, n, ctx->deal_cycle, ctx->deal_cycle ? ctx->deal_owner : nullptr};
        Deal di;
        rc = check_band(&bi, height, &di);
        if (rc) return rc;
        const int rows_i = band_rows_local(height, di);
        const int tiles_i = ((width + 7) / 8) * ((rows_i + 7) / 8);
        const size_t bytes = fmt == SVO_PART_SPARSE_RGB8 ? SVO_SPARSE_PART_BYTES(tiles_i, (size_t)rows_i * width)
                                                         : (size_t)rows_i * (size_t)width * elem;
        HIP_TRY(hipSetDevice(m->device));
        if (pr.cap_bytes < bytes) {
            // the assembles of earlier frames read the old payloads, possibly on another caller
            // stream than this call's: wait for the last assemble of each payload slot
            HIP_TRY(hipSetDevice(m0->device));
            for (int j = 0; j < 2; ++j)
                if (ctx->gathered_used[j]) HIP_TRY(hipEventSynchronize(ctx->gathered[j]));
            HIP_TRY(hipSetDevice(m->device));
            HIP_TRY(hipStreamSynchronize(m->stream));
            for (int j = 0; j < 2; ++j) {
                if (pr.buf[j]) hipFree(pr.buf[j]);
                pr.buf[j] = nullptr;
            }
            pr.cap_bytes = 0;
            for (int j = 0; j < 2; ++j) HIP_TRY(hipMalloc(&pr.buf[j], std::max<size_t>(bytes, 16)));
            pr.cap_bytes = bytes;
        }
        if (fmt == SVO_PART_SPARSE_RGB8 && pr.dense_cap < (size_t)rows_i * width * 3) {
            HIP_TRY(hipStreamSynchronize(m->stream));   // an earlier pack may still read the old scratch
            rc = regrow(&pr.dense, &pr.dense_cap, (size_t)rows_i * width * 3, std::max<size_t>((size_t)rows_i * width * 3, 16));
            if (rc) return rc;
        }
        if (sa && (pr.accum_w != width || pr.accum_rows != rows_i || pr.accum_deal != dkey)) {   // this member's band accumulation
            HIP_TRY(hipStreamSynchronize(m->stream));
            if (pr.accum) hipFree(pr.accum);
            pr.accum = nullptr;
            pr.accum_w = 0;
            pr.accum_rows = -1;
            const size_t abytes = std::max<size_t>((size_t)rows_i * (size_t)width * sizeof(float4), 16);
            HIP_TRY(hipMalloc(&pr.accum, abytes));
            HIP_TRY(hipMemsetAsync(pr.accum, 0, abytes, m->stream));   // a fresh render target
            pr.accum_w = width;
            pr.accum_rows = rows_i;
            pr.accum_deal = dkey;
        }
        if (ctx->gathered_used[k]) HIP_TRY(hipStreamWaitEvent(m->stream, ctx->gathered[k], 0));   // payload k is free
        svo::Outputs oi{};
        if (fmt == SVO_PART_COMPACT) {
            oi.compact = reinterpret_cast<uint32_t *>(pr.buf[k]);
        } else if (fmt == SVO_PART_SPARSE_RGB8) {
            oi.rgb8 = reinterpret_cast<uint8_t *>(pr.dense);
            oi.hitmask = reinterpret_cast<unsigned long long *>(pr.buf[k]);
        } else {
            oi.rgb8 = reinterpret_cast<uint8_t *>(pr.buf[k]);
        }
        SampleArgs sai{};
        if (sa) {
            sai = *sa;
            sai.accum = pr.accum;
            sai.rgba8 = nullptr;
            sai.rgb8 = reinterpret_cast<uint8_t *>(pr.buf[k]);
            sai.layout = SVO_LAYOUT_BAND;
        }
        rc = launch(m, width, height, stack_mode, &bi, oi, m->stream, sa ? &sai : nullptr);
        if (rc) return rc;
        if (fmt == SVO_PART_SPARSE_RGB8) {
            hipError_t e = svo::launch_pack_hits(reinterpret_cast<const uint8_t *>(pr.dense), width, rows_i, pr.buf[k],
                                                 m->stream);
            if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("pack hits launch: ") + hipGetErrorString(e));
        }
        parts[i] = pr.buf[k];
        if (pr.link == SVO_LINK_COPY) {
            // no peer access to this member: its stream copies the payload into a buffer on the
            // display device (the whole capacity for a sparse part, whose size only the device
            // knows).  local[k] is reused only after frame k's assemble: the member's stream
            // waited for gathered[k] above, before this frame's render
            if (pr.local_cap < bytes) {
                HIP_TRY(hipSetDevice(m0->device));
                for (int j = 0; j < 2; ++j)
                    if (ctx->gathered_used[j]) HIP_TRY(hipEventSynchronize(ctx->gathered[j]));
                for (int j = 0; j < 2; ++j) {
                    if (pr.local[j]) hipFree(pr.local[j]);
                    pr.local[j] = nullptr;
                }
                pr.local_cap = 0;
                for (int j = 0; j < 2; ++j) HIP_TRY(hipMalloc(&pr.local[j], std::max<size_t>(bytes, 16)));
                pr.local_cap = bytes;
                HIP_TRY(hipSetDevice(m->device));
            }
            HIP_TRY(hipMemcpyPeerAsync(pr.local[k], m0->device, pr.buf[k], m->device, bytes, m->stream));
            parts[i] = pr.local[k];
        }
        HIP_TRY(hipEventRecord(pr.rendered[k], m->stream));
    }
    HIP_TRY(hipSetDevice(m0->device));
    for (int i = 1; i < n; ++i) HIP_TRY(hipStreamWaitEvent(s0, ctx->peers[i].rendered[k], 0));
    Deal deal;
    rc = check_band(&b0, height, &deal);
    if (rc) return rc;
    rc = assemble(m0, width, height, deal, n, parts.data(), fmt, 0, out, s0);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->gathered[k], s0));
    ctx->gathered_used[k] = true;
    return SVO_OK;
}

// Multi-device upload: the region [offset, offset + n) was validated and uploaded on
// the display member; copy its nodes and attachments to every other member's pool
// device to device (xGMI / SDMA, no second host validation walk or PCIe copy) and
// commit the same upload record there.
int replicate_upload(svo_ctx *g, size_t offset, size_t n) {
    svo_ctx *m0 = g->members[0];
    if (n == 0) return SVO_OK;
    const Upload *u0 = nullptr;
    for (const Upload &u : m0->uploads)
        if (u.offset == offset) u0 = &u;
    if (!u0) return fail(SVO_ERR_STATE, "replicate_upload: no upload record on the display member");
    const Upload u = *u0;
    for (size_t i = 1; i < g->members.size(); ++i) {
        svo_ctx *m = g->members[i];
        if (offset + n > m->capacity) return fail(SVO_ERR_CAPACITY, "upload exceeds a member's node-pool capacity");
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipDeviceSynchronize());   // renders on the member may still read its pool
        HIP_TRY(hipSetDevice(m0->device));
        HIP_TRY(hipMemcpyPeerAsync(m->d_nodes + offset, m->device, m0->d_nodes + offset, m0->device,
                                   n * sizeof(uint2), m0->stream));
        HIP_TRY(hipMemcpyPeerAsync(m->d_att + offset, m->device, m0->d_att + offset, m0->device,
                                   n * sizeof(uint2), m0->stream));
    }
    HIP_TRY(hipSetDevice(m0->device));
    HIP_TRY(hipStreamSynchronize(m0->stream));
    for (size_t i = 1; i < g->members.size(); ++i) {
        const int rc = commit_upload(g->members[i], u);
        if (rc) return rc;
    }
    return SVO_OK;
}

int destroy_single(svo_ctx *ctx) {
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    hipDeviceSynchronize();   // renders on caller streams may still use the context's buffers
    if (ctx->d_nodes) hipFree(ctx->d_nodes);
    if (ctx->d_att) hipFree(ctx->d_att);
    if (ctx->d_stage) hipFree(ctx->d_stage);
    if (ctx->d_shadow_list) hipFree(ctx->d_shadow_list);
    if (ctx->d_refl_voxel) hipFree(ctx->d_refl_voxel);
    if (ctx->d_object_ids) hipFree(ctx->d_object_ids);
    if (ctx->sky.texels) hipFree(const_cast<svo_sky::Texel *>(ctx->sky.texels));
    if (ctx->d_out_hits) hipFree(ctx->d_out_hits);
    if (ctx->d_out_rgba) hipFree(ctx->d_out_rgba);
    if (ctx->d_accum) hipFree(ctx->d_accum);
    if (ctx->d_accum8) hipFree(ctx->d_accum8);
    if (ctx->copy_stream) hipStreamSynchronize(ctx->copy_stream);
    if (ctx->copy_stream2) hipStreamSynchronize(ctx->copy_stream2);
    free_pinned(ctx);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    if (ctx->copy_stream2) hipStreamDestroy(ctx->copy_stream2);
    ctx->copy_pool.reset();
    if (ctx->h_stage) hipHostFree(ctx->h_stage);
    for (int i = 0; i < svo_ctx::STAGE_CHUNKS; ++i)
        if (ctx->stage_ev[i]) hipEventDestroy(ctx->stage_ev[i]);
    for (Sched &q : ctx->sched) {
        free_sched(q);
        if (q.seg_hint) hipFree(q.seg_hint);
        if (q.tile_start) hipFree(q.tile_start);
        if (q.done) hipEventDestroy(q.done);
        for (int r = 0; r < Sched::STATS_RING; ++r)
            if (q.stats_ev[r]) hipEventDestroy(q.stats_ev[r]);
        if (q.side) {
            hipStreamSynchronize(q.side);
            hipStreamDestroy(q.side);
        }
        if (q.render_done) hipEventDestroy(q.render_done);
        for (int i = 0; i < 2; ++i)
            if (q.build_ev[i]) hipEventDestroy(q.build_ev[i]);
        if (q.stats) hipHostFree(q.stats);
    }
    for (auto &v : ctx->timing_events)
        for (auto &ev : v) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
    for (auto &ev : ctx->timing_free) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
    if (ctx->switch_event) hipEventDestroy(ctx->switch_event);
    if (ctx->q_keys) hipFree(ctx->q_keys);
    if (ctx->q_temp) hipFree(ctx->q_temp);
    if (ctx->q_host) hipFree(ctx->q_host);
    if (ctx->q_event) hipEventDestroy(ctx->q_event);
    if (ctx->d_wave_log) hipFree(ctx->d_wave_log);
    for (DevBoxes &db : ctx->dev_boxes)
        if (db.d) hipFree(db.d);
    if (ctx->count_ts) hipFree(ctx->count_ts);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return SVO_OK;
}

// ------------------------------------------------------------------ svo_config
void config_of(const svo_ctx *c, svo_config *o) {
    svo_config k;
    std::memset(&k, 0, sizeof k);
    k.size = sizeof(svo_config);
    k.version = SVO_CONFIG_VERSION;
    k.tile_order = c->tile_order;
    k.xcd_strips = c->xcd_remap == 2 ? 1 : 0;
    k.issue_priority = c->prio;
    k.order_every = c->order_every;
    k.move_every = c->move_every;
    k.move_spread = c->spread;
    k.relayout = c->relayout;
    k.fetch_all = c->fetch_all;
    k.loop_form = c->lat_mode;
    k.lat_ratio = c->lat_ratio;
    k.segments = c->seg_mode;
    k.seg_table_latency = (uint32_t)c->seg_kpack_lat;
    k.seg_table_issue = (uint32_t)c->seg_kpack_issue;
    k.seg_table_thin = (uint32_t)c->seg_kpack_thin;
    k.seg_ratio = c->seg_ratio;
    k.seg_thin_ratio = c->thin_ratio;
    k.seg_cap = c->seg_cap;
    k.seg_min_chain = c->seg_min_chain;
    k.seg_move = c->seg_move;
    k.seg_jitter = c->seg_jitter;
    k.seg_all = c->seg_all;
    k.seg_scramble = c->seg_scramble;
    k.beam = c->beam;
    k.beam_back = c->beam_back;
    k.beam_back_held = c->beam_back_held;
    k.shadow_form = c->shadow_compact ? 2 : c->fused_shadows ? 0 : 1;
    k.shadow_order = c->shadow_order_enabled;
    k.readback = c->pin_push;
    k.host_copy_threads = c->host_copy_threads;
    k.sparse_payload = c->sparse_payload;
    k.peer_copy = c->peer_copy;
    *o = k;
}

int check_config(const svo_config &k) {
    auto bit = [](int32_t v) { return v == 0 || v == 1; };
    auto table = [](uint32_t t) {
        if (t > 0xFFFFFFu) return false;
        for (int c = 0; c < 6; ++c) {
            const uint32_t kc = (t >> (4 * c)) & 15u;
            if (kc != 0 && kc != 4 && kc != 8) return false;
        }
        return true;
    };
    auto ratio = [](float r) { return std::isfinite(r) && r >= 0.0f; };
    const char *bad = !bit(k.tile_order) ? "tile_order" : !bit(k.xcd_strips) ? "xcd_strips"
                    : !bit(k.issue_priority) ? "issue_priority" : k.order_every < 1 ? "order_every"
                    : k.move_every < 1 ? "move_every" : !bit(k.move_spread) ? "move_spread"
                    : !bit(k.relayout) ? "relayout" : k.fetch_all < -1 || k.fetch_all > 1 ? "fetch_all"
                    : k.loop_form < -1 || k.loop_form > 1 ? "loop_form" : !ratio(k.lat_ratio) ? "lat_ratio"
                    : !bit(k.segments) ? "segments" : !table(k.seg_table_latency) ? "seg_table_latency"
                    : !table(k.seg_table_issue) ? "seg_table_issue" : !table(k.seg_table_thin) ? "seg_table_thin"
                    : !ratio(k.seg_ratio) ? "seg_ratio" : !ratio(k.seg_thin_ratio) ? "seg_thin_ratio"
                    : k.seg_cap < 1 ? "seg_cap" : k.seg_min_chain < 0 ? "seg_min_chain"
                    : k.seg_move < 1 || k.seg_move > 2 ? "seg_move" : k.seg_jitter < 0 || k.seg_jitter > 2 ? "seg_jitter"
                    : k.seg_all != 0 && k.seg_all != 4 && k.seg_all != 8 ? "seg_all" : !bit(k.beam) ? "beam"
                    : k.beam_back < 0 || k.beam_back > 22 ? "beam_back" : k.shadow_form < 0 || k.shadow_form > 2 ? "shadow_form"
                    : !bit(k.shadow_order) ? "shadow_order" : k.readback < 0 || k.readback > 2 ? "readback"
                    : k.host_copy_threads < 0 || k.host_copy_threads > 16 ? "host_copy_threads"
                    : !bit(k.sparse_payload) ? "sparse_payload" : !bit(k.peer_copy) ? "peer_copy"
                    : k.beam_back_held < -1 || k.beam_back_held > 22 ? "beam_back_held" : nullptr;
    if (bad) return fail(SVO_ERR_ARG, std::string("svo_config.") + bad + " out of range");
    return SVO_OK;
}

// One device's context takes a validated config.  Nothing here changes a result; what holds state
// built under the old value is rebuilt: the pinned readback slots (their allocation flags follow
// `readback`), the host copy threads, the pool's splat lists (beam, beam_back, beam_back_held); and every stream's
// loop-form / class-table decision is dropped, so the next order build decides under the new rule.
int apply_config(svo_ctx *c, const svo_config &k) {
    c->tile_order = k.tile_order;
    c->xcd_remap = k.xcd_strips ? 2 : 0;
    c->prio = k.issue_priority;
    c->order_every = k.order_every;
    c->move_every = k.move_every;
    c->spread = k.move_spread;
    c->relayout = k.relayout;
    c->fetch_all = k.fetch_all;
    c->lat_mode = k.loop_form;
    c->lat_ratio = k.lat_ratio;
    c->seg_mode = k.segments;
    c->seg_kpack_lat = (int)k.seg_table_latency;
    c->seg_kpack_issue = (int)k.seg_table_issue;
    c->seg_kpack_thin = (int)k.seg_table_thin;
    c->seg_ratio = k.seg_ratio;
    c->thin_ratio = k.seg_thin_ratio;
    c->seg_cap = k.seg_cap;
    c->seg_min_chain = k.seg_min_chain;
    c->seg_move = k.seg_move;
    c->seg_jitter = k.seg_jitter;
    c->seg_all = k.seg_all;
    c->seg_scramble = k.seg_scramble;
    c->shadow_compact = k.shadow_form == 2;
    c->fused_shadows = k.shadow_form == 0;
    c->shadow_order_enabled = k.shadow_order;
    c->sparse_payload = k.sparse_payload;
    c->peer_copy = k.peer_copy;
    if (c->pin_push != k.readback) {
        if (c->h_pin[0]) {
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));
            if (c->copy_stream2) HIP_TRY(hipStreamSynchronize(c->copy_stream2));
            free_pinned(c);
        }
        c->pin_push = k.readback;
    }
    if (c->host_copy_threads != k.host_copy_threads) {
        c->copy_pool.reset();   // idle between calls (svo_render waits for it)
        c->host_copy_threads = k.host_copy_threads;
    }
    const bool boxes = c->beam != k.beam || c->beam_back != k.beam_back || c->beam_back_held != k.beam_back_held;
    c->beam = k.beam;
    c->beam_back = k.beam_back;
    c->beam_back_held = k.beam_back_held;
    if (boxes && c->n_nodes > 0) {
        const int rc = recompute_pool(c);
        if (rc) return rc;
    }
    for (Sched &q : c->sched) {
        q.lat_key = Geo();
        q.lat_mode = -1;
    }
    return SVO_OK;
}

// ------------------------------------------------------------------ ray queries
// The ray-batch calls (svo_trace_rays .. svo_sample_sky, svo_scene_light_rays among them, and their _host
// twins) share four pieces: HostStage (the staged round trip of a _host call), on_device (the entry shell), the
// check_batch_* argument checks and the launch-struct fillers pool_params / query_args / batch_of.  DESIGN.md 3.2i.

// Make stream s wait for the query-scratch work the previous user enqueued on another stream
// (order_scratch's rule, for the query's own scratch).
int order_query_scratch(svo_ctx *c, hipStream_t s) {
    if (c->q_valid && c->q_stream != s) {
        if (!c->q_event) HIP_TRY(hipEventCreateWithFlags(&c->q_event, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->q_event, c->q_stream));
        HIP_TRY(hipStreamWaitEvent(s, c->q_event, 0));
    }
    c->q_stream = s;
    c->q_valid = true;
    return SVO_OK;
}

// Grow-only query scratch: *buf holds at least `need` bytes afterwards.
template <class T>
int grow_query_scratch(T **buf, size_t *cap, size_t need) {
    if (need <= *cap) return SVO_OK;
    HIP_TRY(hipDeviceSynchronize());   // an earlier asynchronous query may still use the old scratch
    return regrow(buf, cap, need, need);
}

// The staged round trip of a _host call, on the context's stream and its host-staging scratch: reserve the
// parts, begin(), upload, the launch, download, finish().  The rule it exists for: no copy may still read or
// write the caller's arrays once the call has returned, an error included -- so from begin() on, every exit
// but finish() waits for the stream in the destructor, and finish() is the wait whose error is reported.
class HostStage {
public:
    explicit HostStage(svo_ctx *c) : c_(c) {}
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage() {
        if (armed_) hipStreamSynchronize(c_->stream);
    }
    // Reserve `bytes` before begin(): the part's offset.  Every part starts on a 16-byte boundary, the
    // strictest alignment a kernel asks of a list.
    size_t part(size_t bytes) {
        const size_t offset = size_;
        size_ = (offset + bytes + 15) & ~(size_t)15;
        return offset;
    }
    int begin() {
        if (int rc = grow_query_scratch(&c_->q_host, &c_->q_host_cap, size_)) return rc;
        if (int rc = order_query_scratch(c_, c_->stream)) return rc;
        armed_ = true;
        return SVO_OK;
    }
    // A part's device pointer (after begin()).
    template <class T = void>
    T *at(size_t part) const {
        return reinterpret_cast<T *>(static_cast<char *>(c_->q_host) + part);
    }
    // The part's pointer if the caller has this list (an optional input or output), else null.
    template <class T = void>
    T *at_if(const void *wanted, size_t part) const {
        return wanted ? at<T>(part) : nullptr;
    }
    // A null src or dst is a list the caller does not have: no copy.
    int upload(size_t part, const void *src, size_t bytes) {
        if (src) HIP_TRY(hipMemcpyAsync(at(part), src, bytes, hipMemcpyHostToDevice, c_->stream));
        return SVO_OK;
    }
    int download(void *dst, size_t part, size_t bytes) {
        if (dst) HIP_TRY(hipMemcpyAsync(dst, at(part), bytes, hipMemcpyDeviceToHost, c_->stream));
        return SVO_OK;
    }
    int finish() {
        HIP_TRY(hipStreamSynchronize(c_->stream));
        armed_ = false;
        return SVO_OK;
    }

private:
    svo_ctx *c_;
    size_t size_ = 0;
    bool armed_ = false;
};

svo_ctx *batch_context(svo_ctx *ctx) { return is_multi(ctx) ? ctx->members[0] : ctx; }

// The shell of every ray-batch entry point once its arguments are checked: a multi-device context's member 0,
// the pool test where the call walks the pool (before a device is selected), the device, the stream (null:
// the context's own), and body(c, s) with what it throws reported under the entry point's name.
template <class F>
int on_device(svo_ctx *ctx, const char *name, void *stream, bool needs_pool, F &&body) {
    try {
        svo_ctx *c = batch_context(ctx);
        if (needs_pool && c->n_nodes == 0) return fail(SVO_ERR_STATE, "no node pool uploaded (svo_set_buffer)");
        HIP_TRY(hipSetDevice(c->device));
        return body(c, stream ? (hipStream_t)stream : c->stream);
    } catch (const std::exception &e) {
        return fail(SVO_ERR_HIP, std::string(name) + ": " + e.what());
    }
}

// A launch's result, or SVO_ERR_HIP under `label`.
int launched(hipError_t e, const char *label) {
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string(label) + ": " + hipGetErrorString(e));
    return SVO_OK;
}

constexpr size_t MAX_QUERY_RAYS = ((size_t)1 << 31) - 1;

// A LOD pair (svo_set_lod, svo_trace_rays_lod): two non-negative finite numbers (-0 counts as 0).
bool lod_pair_ok(float coef, float bias) { return std::isfinite(coef) && std::isfinite(bias) && coef >= 0.0f && bias >= 0.0f; }
const char *const LOD_PAIR_MSG = "ray_size_coef and ray_size_bias must be finite and not negative";

// ---- the argument checks that need no device and no context state
int check_query_args(size_t n_rays, int stack_mode, uint32_t flags) {
    if (flags & ~(uint32_t)(SVO_QUERY_ORDERED | SVO_QUERY_RAW_DIRECTIONS)) return fail(SVO_ERR_ARG, "unknown query flag bits");
    if (stack_mode != SVO_STACK_HLSL && stack_mode != SVO_STACK_EXACT) return fail(SVO_ERR_ARG, "unknown stack mode");
    if (n_rays > MAX_QUERY_RAYS) return fail(SVO_ERR_ARG, "more than 2^31 - 1 rays in one query");
    return SVO_OK;
}

// The head of the calls on a traced batch (bounce, ambient, light rays): the pointers, then the flags, with
// the call's own word in the complaint.
int check_batch_head(const svo_ctx *ctx, const void *rays, const void *hits, const void *voxel, const void *rays_out,
                     uint32_t flags, const char *word) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!rays) return fail(SVO_ERR_ARG, "null ray list");
    if (!hits) return fail(SVO_ERR_ARG, "null hit records");
    if (!voxel) return fail(SVO_ERR_ARG, "null voxel keys");
    if (!rays_out) return fail(SVO_ERR_ARG, "null output ray list");
    if (flags & ~(uint32_t)SVO_QUERY_RAW_DIRECTIONS) return fail(SVO_ERR_ARG, std::string("unknown ") + word + " flag bits");
    return SVO_OK;
}

// n entries with `fan` output rays each: at most 2^31 - 1 of `what`.
int check_batch_count(size_t n, size_t fan, const char *what) {
    if (n > MAX_QUERY_RAYS / fan) return fail(SVO_ERR_ARG, std::string("more than 2^31 - 1 ") + what + " in one batch");
    return SVO_OK;
}

bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// The tail of the calls that fan out (ambient, light rays): the count, then the output list clear of every
// input.  Not for the calls that may work in place (bounce, object rays: check_batch_count alone).
int check_batch_fan(const void *rays, size_t n, const void *hits, const void *voxel, size_t fan, const void *rays_out,
                    const char *what) {
    if (int rc = check_batch_count(n, fan, what)) return rc;
    const size_t out_bytes = 32 * n * fan;
    if (ranges_overlap(rays_out, out_bytes, rays, 32 * n) || ranges_overlap(rays_out, out_bytes, hits, 24 * n) ||
        ranges_overlap(rays_out, out_bytes, voxel, 8 * n))
        return fail(SVO_ERR_ARG, "the output ray list overlaps an input");
    return SVO_OK;
}

// The device pointers' alignment (null where the call has no such list).
int check_batch_alignment(const void *d_rays, const void *d_rays_out, const void *d_hits, const void *d_voxel) {
    if (((uintptr_t)d_rays | (uintptr_t)d_rays_out) & 15u) return fail(SVO_ERR_ARG, "ray lists must be 16-byte aligned");
    if (((uintptr_t)d_hits | (uintptr_t)d_voxel) & 7u) return fail(SVO_ERR_ARG, "hit records and voxel keys must be 8-byte aligned");
    return SVO_OK;
}

// ---- the launch structs
uint32_t raw_bit(uint32_t flags) { return (flags & SVO_QUERY_RAW_DIRECTIONS) ? svo::QUERY_RAW : 0u; }

svo::LaunchParams pool_params(const svo_ctx *c) {
    svo::LaunchParams p;
    std::memset(&p, 0, sizeof p);
    p.nodes = c->d_nodes;
    p.att = c->d_att;
    p.n_nodes = (uint32_t)std::min<size_t>(c->n_nodes, 0xFFFFFFFFu);
    return p;
}

svo::QueryArgs query_args(const svo_ray *d_rays, size_t n, uint32_t flags, const svo_query_out &out) {
    svo::QueryArgs q;
    std::memset(&q, 0, sizeof q);
    q.rays = reinterpret_cast<const svo::QueryRay *>(d_rays);
    q.n = (uint32_t)n;
    q.flags = raw_bit(flags);
    q.out.hits = reinterpret_cast<svo::Hit *>(out.hits);
    q.out.position = reinterpret_cast<float4 *>(out.position);
    q.out.voxel = reinterpret_cast<unsigned long long *>(out.voxel);
    q.out.hitmask = reinterpret_cast<unsigned long long *>(out.hitmask);
    return q;
}

// A traced batch as the flat kernels take it (bounce, ambient, light, scene-light and object rays; hits,
// voxel and object null where the call has none).
struct Batch {
    const svo::QueryRay *rays;
    uint32_t n, raw;
    const svo::Hit *hits;
    const unsigned long long *voxel;
    svo::QueryRay *out;
    const int32_t *object;   // svo_trace_scene's ids (scene-light rays only)
};

Batch batch_of(const void *d_rays, size_t n, uint32_t flags, const void *d_hits, const void *d_voxel, void *d_rays_out,
               const void *d_object = nullptr) {
    return {static_cast<const svo::QueryRay *>(d_rays), (uint32_t)n, raw_bit(flags), static_cast<const svo::Hit *>(d_hits),
            static_cast<const unsigned long long *>(d_voxel), static_cast<svo::QueryRay *>(d_rays_out),
            static_cast<const int32_t *>(d_object)};
}

int bounce_launch(const Batch &b, hipStream_t s) {
    return launched(svo::launch_bounce_rays(b.rays, b.n, b.raw, b.hits, b.voxel, b.out, s), "bounce launch");
}

int ambient_launch(const Batch &b, int n_rays, float radius, uint32_t variant, hipStream_t s) {
    return launched(svo::launch_ambient_rays(b.rays, b.n, b.raw, b.hits, b.voxel, n_rays, radius, variant, b.out, s),
                    "ambient ray launch");
}

int light_launch(const Batch &b, const svo_light *lights, int n_lights, hipStream_t s) {
    return launched(svo::launch_light_rays(b.rays, b.n, b.raw, b.hits, b.voxel,
                                           reinterpret_cast<const svo_lights::Light *>(lights), n_lights, b.out, s),
                    "light ray launch");
}

int scene_light_launch(const Batch &b, const svo_object *objects, int n_objects, const svo_light *lights, int n_lights,
                       hipStream_t s) {
    svo_objects::Object obs[svo_objects::MAX_OBJECTS] = {};
    for (int j = 0; j < n_objects; ++j) std::memcpy(obs + j, objects + j, sizeof obs[j]);
    return launched(svo::launch_scene_light_rays(b.rays, b.n, b.raw, b.hits, b.voxel, b.object, obs, n_objects,
                                                 reinterpret_cast<const svo_lights::Light *>(lights), n_lights, b.out, s),
                    "scene light ray launch");
}

int object_rays_launch(const Batch &b, const svo_object *object, hipStream_t s) {
    svo_objects::Object ob;
    std::memcpy(&ob, object, sizeof ob);
    return launched(svo::launch_object_rays(b.rays, b.n, ob, b.out, s), "object ray launch");
}

// One query on context c (single-device), its device selected: arguments and pool checked by the caller.
int query_device(svo_ctx *c, const svo_ray *d_rays, size_t n_rays, int stack_mode, uint32_t flags,
                 const svo_query_out &out, hipStream_t s, float lod_coef, float lod_bias) {
    if ((uintptr_t)d_rays & 15u) return fail(SVO_ERR_ARG, "d_rays must be 16-byte aligned");
    svo::LaunchParams p = pool_params(c);
    // loop form: exactly the render launch's choice for this pool (launch): guarded unless the
    // longest path is proven (at most 22 levels, no cycle) and the parent indices are exact
    p.slots = std::max(c->depth - 1, 1);
    p.guard = !c->depth_exact || (stack_mode == 0 && c->n_nodes > ((size_t)1 << 24)) || c->n_nodes >= ((size_t)1 << 29);
    p.fetch_all = c->fetch_all >= 0 ? c->fetch_all : (c->n_nodes < ((size_t)1 << 24) ? 1 : 0);
    // the batch's own level of detail (svo_trace_rays_lod; 0, 0: the plain kernels)
    p.lod = lod_coef != 0.0f || lod_bias != 0.0f;
    p.lod_coef = lod_coef;
    p.lod_bias = lod_bias;
    svo::QueryArgs q = query_args(d_rays, n_rays, flags, out);
    if (flags & SVO_QUERY_ORDERED) {
        const size_t temp = svo::query_sort_bytes(q.n);
        if (temp == 0) return fail(SVO_ERR_HIP, "radix sort: temporary storage query failed");
        int rc = grow_query_scratch(&c->q_keys, &c->q_cap, 4 * n_rays * sizeof(uint32_t));
        if (rc) return rc;
        rc = grow_query_scratch(&c->q_temp, &c->q_temp_cap, temp);
        if (rc) return rc;
        rc = order_query_scratch(c, s);
        if (rc) return rc;
        uint32_t *keys = c->q_keys, *keys_out = keys + n_rays, *index = keys + 2 * n_rays, *index_out = keys + 3 * n_rays;
        hipError_t e = svo::launch_query_keys(q, keys, index, s);
        if (e == hipSuccess) e = svo::launch_query_sort(keys, keys_out, index, index_out, q.n, c->q_temp, temp, s);
        rc = launched(e, "query order");
        if (rc) return rc;
        q.index = index_out;
    }
    return launched(svo::launch_query(p, q, stack_mode, s), "query launch");
}

// The checks svo_trace_rays_lod and its _host twin share.  out_error: the twin's complaint about its outputs,
// or null.
int check_trace_args(svo_ctx *ctx, const void *rays, size_t n_rays, int stack_mode, uint32_t flags, float lod_coef,
                     float lod_bias, const char *out_error) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!lod_pair_ok(lod_coef, lod_bias)) return fail(SVO_ERR_ARG, LOD_PAIR_MSG);
    if (!rays) return fail(SVO_ERR_ARG, "null ray list");
    if (out_error) return fail(SVO_ERR_ARG, out_error);
    return check_query_args(n_rays, stack_mode, flags);
}

int check_bounce_args(svo_ctx *ctx, const void *rays, size_t n, uint32_t flags, const void *hits, const void *voxel,
                      const void *rays_out) {
    if (int rc = check_batch_head(ctx, rays, hits, voxel, rays_out, flags, "bounce")) return rc;
    return check_batch_count(n, 1, "rays");   // no overlap test: rays_out may be rays
}

const char *ambient_setting_error(int n_rays, float radius, uint32_t variant) {
    if (!svo_ambient::valid_count(n_rays)) return "n_rays must be 4, 8 or 16";
    if (!(radius > 0.0f)) return "radius must be +inf or finite and positive";
    if (variant > 7u) return "variant must lie in 0..7";
    return nullptr;
}

int check_ambient_args(svo_ctx *ctx, const void *rays, size_t n, uint32_t flags, const void *hits, const void *voxel,
                       int n_rays, float radius, uint32_t variant, const void *rays_out) {
    if (int rc = check_batch_head(ctx, rays, hits, voxel, rays_out, flags, "ambient")) return rc;
    if (const char *msg = ambient_setting_error(n_rays, radius, variant)) return fail(SVO_ERR_ARG, msg);
    return check_batch_fan(rays, n, hits, voxel, (size_t)n_rays, rays_out, "ambient rays");
}

// A light list as svo_set_lights and svo_light_rays take it (host memory): n_lights in 0 .. 8, and with a
// non-NULL list every light valid (svo_light.h light_error).
int check_light_list(const svo_light *lights, int n_lights) {
    static_assert(sizeof(svo_light) == sizeof(svo_lights::Light), "svo_light layout");
    if (n_lights < 0 || n_lights > svo_lights::MAX_LIGHTS) return fail(SVO_ERR_ARG, "n_lights must lie in 0..8");
    for (int j = 0; lights && j < n_lights; ++j) {
        svo_lights::Light l;
        std::memcpy(&l, lights + j, sizeof l);
        if (const char *msg = svo_lights::light_error(l)) return fail(SVO_ERR_ARG, "light " + std::to_string(j) + ": " + msg);
    }
    return SVO_OK;
}

// The light list of svo_light_rays and svo_scene_light_rays: a non-NULL list of 1 .. 8 valid lights.
int check_ray_light_list(const svo_light *lights, int n_lights) {
    if (!lights) return fail(SVO_ERR_ARG, "null light list");
    if (n_lights < 1) return fail(SVO_ERR_ARG, "n_lights must lie in 1..8");
    return check_light_list(lights, n_lights);
}

int check_light_args(svo_ctx *ctx, const void *rays, size_t n, uint32_t flags, const void *hits, const void *voxel,
                     const svo_light *lights, int n_lights, const void *rays_out) {
    if (int rc = check_batch_head(ctx, rays, hits, voxel, rays_out, flags, "light-ray")) return rc;
    if (int rc = check_ray_light_list(lights, n_lights)) return rc;
    return check_batch_fan(rays, n, hits, voxel, (size_t)n_lights, rays_out, "light rays");
}

// An object list as svo_set_objects and svo_trace_scene take it (host memory): n_objects in 0 .. 8, and with
// a non-NULL list every object valid (svo_object.h object_error).  The roots' bound needs the context:
// check_object_roots.
int check_object_list(const svo_object *objects, int n_objects) {
    static_assert(sizeof(svo_object) == sizeof(svo_objects::Object), "svo_object layout");
    if (n_objects < 0 || n_objects > svo_objects::MAX_OBJECTS) return fail(SVO_ERR_ARG, "n_objects must lie in 0..8");
    for (int j = 0; objects && j < n_objects; ++j) {
        svo_objects::Object ob;
        std::memcpy(&ob, objects + j, sizeof ob);
        if (const char *msg = svo_objects::object_error(ob)) return fail(SVO_ERR_ARG, "object " + std::to_string(j) + ": " + msg);
    }
    return SVO_OK;
}

int check_object_roots(const svo_ctx *c, const svo_object *objects, int n_objects) {
    for (int j = 0; objects && j < n_objects; ++j)
        if ((size_t)objects[j].root >= c->capacity)
            return fail(SVO_ERR_ARG, "object " + std::to_string(j) + ": root outside the node-pool capacity");
    return SVO_OK;
}

// Its own head: no hit records or voxel keys, and the object before the flags.
int check_object_ray_args(svo_ctx *ctx, const void *rays, size_t n, uint32_t flags, const svo_object *object,
                          const void *rays_out) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!rays) return fail(SVO_ERR_ARG, "null ray list");
    if (!rays_out) return fail(SVO_ERR_ARG, "null output ray list");
    if (!object) return fail(SVO_ERR_ARG, "null object");
    if (flags & ~(uint32_t)SVO_QUERY_RAW_DIRECTIONS) return fail(SVO_ERR_ARG, "unknown object-ray flag bits");
    if (int rc = check_object_list(object, 1)) return rc;
    return check_batch_count(n, 1, "rays");   // no overlap test: rays_out may be rays
}

// `any_out` = some output was asked for.
int check_scene_args(svo_ctx *ctx, const void *rays, size_t n, int stack_mode, uint32_t flags, const svo_object *objects,
                     int n_objects, bool any_out) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!rays) return fail(SVO_ERR_ARG, "null ray list");
    if (!any_out) return fail(SVO_ERR_ARG, "every scene-query output is null");
    if (flags & SVO_QUERY_ORDERED) return fail(SVO_ERR_ARG, "SVO_QUERY_ORDERED is not supported by scene queries");
    if (flags & ~(uint32_t)(SVO_QUERY_RAW_DIRECTIONS | SVO_SCENE_NO_TERRAIN)) return fail(SVO_ERR_ARG, "unknown scene-query flag bits");
    if (int rc = check_query_args(n, stack_mode, 0u)) return rc;
    if (n_objects > 0 && !objects) return fail(SVO_ERR_ARG, "null object list");
    if (int rc = check_object_list(objects, n_objects)) return rc;
    return check_object_roots(batch_context(ctx), objects, n_objects);
}

// One scene query on context c (single-device), its device selected: arguments and pool checked by the caller.
int scene_device(svo_ctx *c, const svo_ray *d_rays, size_t n, int stack_mode, uint32_t flags, const svo_object *objects,
                 int n_objects, const svo_query_out &out, int32_t *d_object, hipStream_t s) {
    if ((uintptr_t)d_rays & 15u) return fail(SVO_ERR_ARG, "d_rays must be 16-byte aligned");
    svo::LaunchParams p = pool_params(c);
    p.slots = 21;   // every walk of a scene query is guarded, on the full stack (svo_kernel.hip OBJECT_SLOTS)
    p.guard = 1;
    const svo::QueryArgs q = query_args(d_rays, n, flags, out);
    svo_objects::Object obs[svo_objects::MAX_OBJECTS] = {};
    for (int j = 0; j < n_objects; ++j) std::memcpy(obs + j, objects + j, sizeof obs[j]);
    return launched(svo::launch_scene_query(p, q, obs, n_objects, !(flags & SVO_SCENE_NO_TERRAIN), d_object, stack_mode, s),
                    "scene query launch");
}

// svo_light_rays' checks, then svo_trace_scene's for the object list (not the roots: the call reads no pool),
// with the same complaints for the same faults; the ids are one more input the output must stay clear of.
int check_scene_light_args(svo_ctx *ctx, const void *rays, size_t n, uint32_t flags, const void *hits, const void *voxel,
                           const void *object, const svo_object *objects, int n_objects, const svo_light *lights,
                           int n_lights, const void *rays_out) {
    if (int rc = check_batch_head(ctx, rays, hits, voxel, rays_out, flags, "scene-light-ray")) return rc;
    if (!object) return fail(SVO_ERR_ARG, "null object ids");
    if (n_objects > 0 && !objects) return fail(SVO_ERR_ARG, "null object list");
    if (int rc = check_object_list(objects, n_objects)) return rc;
    if (int rc = check_ray_light_list(lights, n_lights)) return rc;
    if (int rc = check_batch_fan(rays, n, hits, voxel, (size_t)n_lights, rays_out, "light rays")) return rc;
    if (ranges_overlap(rays_out, 32 * n * (size_t)n_lights, object, 4 * n))
        return fail(SVO_ERR_ARG, "the output ray list overlaps an input");
    return SVO_OK;
}

int check_sky_args(svo_ctx *ctx, const float *dirs, size_t n, const float *rgba) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!dirs) return fail(SVO_ERR_ARG, "null direction list");
    if (!rgba) return fail(SVO_ERR_ARG, "null colour output");
    if (n > MAX_QUERY_RAYS) return fail(SVO_ERR_ARG, "more than 2^31 - 1 directions");
    return SVO_OK;
}

int sky_launch(svo_ctx *c, const void *d_dirs, size_t n, void *d_rgba, hipStream_t s) {
    return launched(svo::launch_sample_sky(c->sky, static_cast<const float4 *>(d_dirs), (uint32_t)n,
                                           static_cast<float4 *>(d_rgba), s), "sky sample launch");
}

// The host twin of a call on a traced batch (hits, voxel, object null where the call has none): the inputs
// staged, launch(batch, s), and n * fan rays brought back -- fan 0: n rays, written over the staged input.
template <class F>
int batch_host(svo_ctx *ctx, const char *name, const void *rays, size_t n, uint32_t flags, const void *hits,
               const void *voxel, size_t fan, void *rays_out, F &&launch, const int32_t *object = nullptr) {
    return on_device(ctx, name, nullptr, false, [&](svo_ctx *c, hipStream_t s) {
        HostStage st(c);
        const size_t out_bytes = 32 * n * std::max<size_t>(fan, 1);
        const size_t p_rays = st.part(32 * n), p_hits = st.part(hits ? 24 * n : 0), p_vox = st.part(voxel ? 8 * n : 0),
                     p_id = st.part(object ? 4 * n : 0), p_out = fan ? st.part(out_bytes) : p_rays;
        if (int rc = st.begin()) return rc;
        if (int rc = st.upload(p_rays, rays, 32 * n)) return rc;
        if (int rc = st.upload(p_hits, hits, 24 * n)) return rc;
        if (int rc = st.upload(p_vox, voxel, 8 * n)) return rc;
        if (int rc = st.upload(p_id, object, 4 * n)) return rc;
        if (int rc = launch(batch_of(st.at(p_rays), n, flags, st.at_if(hits, p_hits), st.at_if(voxel, p_vox), st.at(p_out),
                                     st.at_if(object, p_id)), s))
            return rc;
        if (int rc = st.download(rays_out, p_out, out_bytes)) return rc;
        return st.finish();
    });
}

// The host twin of a trace (svo_trace_rays_lod_host, svo_trace_scene_host): the rays staged, trace(c, d_rays,
// out, d_object, s) with a part for every output the caller asked for, and those brought back.
template <class F>
int traced_host(svo_ctx *ctx, const char *name, const svo_ray *rays, size_t n, svo_hit *hits, float *position,
                uint64_t *voxel, int32_t *object, F &&trace) {
    return on_device(ctx, name, nullptr, true, [&](svo_ctx *c, hipStream_t s) {
        HostStage st(c);
        const size_t p_rays = st.part(32 * n), p_pos = st.part(16 * n), p_hits = st.part(24 * n), p_vox = st.part(8 * n),
                     p_id = st.part(object ? 4 * n : 0);
        if (int rc = st.begin()) return rc;
        if (int rc = st.upload(p_rays, rays, 32 * n)) return rc;
        svo_query_out out{};
        out.hits = st.at_if<svo_hit>(hits, p_hits);
        out.position = st.at_if<float>(position, p_pos);
        out.voxel = st.at_if<uint64_t>(voxel, p_vox);
        if (int rc = trace(c, st.at<const svo_ray>(p_rays), out, st.at_if<int32_t>(object, p_id), s)) return rc;
        if (int rc = st.download(hits, p_hits, 24 * n)) return rc;
        if (int rc = st.download(position, p_pos, 16 * n)) return rc;
        if (int rc = st.download(voxel, p_vox, 8 * n)) return rc;
        if (int rc = st.download(object, p_id, 4 * n)) return rc;
        return st.finish();
    });
}

// ---- volume queries (svo_overlap_volumes; svo_overlap.h is the rule)
// The caller's params as this library reads them: the fields inside the caller's size, 0 beyond it; NULL: all
// defaults.  max_visits comes out resolved (0: the default budget).
int read_overlap_params(const svo_overlap_params *params, svo_overlap_params *k) {
    std::memset(k, 0, sizeof *k);
    if (params) {
        if (params->size < 2 * sizeof(uint32_t)) return fail(SVO_ERR_ARG, "svo_overlap_params.size must hold at least size and flags");
        if (params->size > sizeof *k)
            return fail(SVO_ERR_ARG, "svo_overlap_params.size " + std::to_string(params->size) +
                                         " is larger than this library's (" + std::to_string(sizeof *k) + "): a newer ABI");
        std::memcpy(k, params, params->size);
    }
    k->size = sizeof *k;
    if (k->flags & ~(uint32_t)SVO_OVERLAP_ANY) return fail(SVO_ERR_ARG, "unknown overlap flag bits");
    if (k->max_contacts > svo_volumes::MAX_CONTACTS) return fail(SVO_ERR_ARG, "max_contacts must lie in 0..32");
    if (k->max_visits > svo_volumes::MAX_VISITS) return fail(SVO_ERR_ARG, "max_visits must be 0 or lie in 1..2^24");
    if (k->coarse_level > (uint32_t)svo_volumes::MAX_LEVEL) return fail(SVO_ERR_ARG, "coarse_level must be 0 or lie in 1..22");
    if (k->max_visits == 0) k->max_visits = svo_volumes::DEFAULT_VISITS;
    return SVO_OK;
}

// The checks the device and the host form share; out_error: the form's complaint about its outputs, or null.
int check_overlap_args(svo_ctx *ctx, const void *shapes, size_t n, const svo_overlap_params *params, const char *out_error,
                       bool has_contacts, svo_overlap_params *k) {
    static_assert(sizeof(svo_shape) == sizeof(svo_volumes::Shape) && sizeof(svo_contact) == sizeof(svo_volumes::Contact) &&
                      sizeof(svo_overlap) == sizeof(svo_volumes::Summary),
                  "overlap record layouts");
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!shapes) return fail(SVO_ERR_ARG, "null shape list");
    if (out_error) return fail(SVO_ERR_ARG, out_error);
    if (int rc = read_overlap_params(params, k)) return rc;
    if (has_contacts && k->max_contacts == 0) return fail(SVO_ERR_ARG, "contacts asked for with max_contacts 0");
    if (int rc = check_batch_count(n, 1, "shapes")) return rc;
    if (int rc = check_batch_count(n, std::max<size_t>(k->max_contacts, 1), "contacts")) return rc;
    if ((size_t)k->root >= batch_context(ctx)->capacity) return fail(SVO_ERR_ARG, "root outside the node-pool capacity");
    return SVO_OK;
}

// One volume query on context c (single-device), its device selected: arguments and pool checked by the caller.
int overlap_device(svo_ctx *c, const svo_shape *d_shapes, size_t n, const svo_overlap_params &k, const svo_overlap_out &out,
                   hipStream_t s) {
    svo::OverlapArgs a;
    std::memset(&a, 0, sizeof a);
    a.nodes = c->d_nodes;
    a.n_nodes = (uint32_t)std::min<size_t>(c->n_nodes, 0xFFFFFFFFu);
    a.shapes = reinterpret_cast<const svo_volumes::Shape *>(d_shapes);
    a.n = (uint32_t)n;
    a.flags = k.flags;
    a.root = k.root;
    a.max_contacts = k.max_contacts;
    a.max_visits = k.max_visits;
    a.coarse_level = k.coarse_level;
    a.summary = reinterpret_cast<svo_volumes::Summary *>(out.summary);
    a.contacts = reinterpret_cast<svo_volumes::Contact *>(out.contacts);
    a.hitmask = reinterpret_cast<unsigned long long *>(out.hitmask);
    return launched(svo::launch_overlap(a, s), "overlap launch");
}

// ---- closest voxels (svo_closest_voxels; svo_closest.h is the rule)
// The caller's params as this library reads them, like read_overlap_params; max_visits comes out resolved.
int read_closest_params(const svo_closest_params *params, svo_closest_params *k) {
    std::memset(k, 0, sizeof *k);
    if (params) {
        if (params->size < 2 * sizeof(uint32_t)) return fail(SVO_ERR_ARG, "svo_closest_params.size must hold at least size and flags");
        if (params->size > sizeof *k)
            return fail(SVO_ERR_ARG, "svo_closest_params.size " + std::to_string(params->size) +
                                         " is larger than this library's (" + std::to_string(sizeof *k) + "): a newer ABI");
        std::memcpy(k, params, params->size);
    }
    k->size = sizeof *k;
    if (k->flags & ~(uint32_t)SVO_CLOSEST_UNBOUNDED) return fail(SVO_ERR_ARG, "unknown closest flag bits");
    if (k->max_visits > svo_nearest::MAX_VISITS) return fail(SVO_ERR_ARG, "max_visits must be 0 or lie in 1..2^24");
    if (k->coarse_level > (uint32_t)svo_nearest::MAX_LEVEL) return fail(SVO_ERR_ARG, "coarse_level must be 0 or lie in 1..22");
    if (k->max_visits == 0) k->max_visits = svo_nearest::DEFAULT_VISITS;
    return SVO_OK;
}

// The checks the device and the host form share; out_error: the form's complaint about its outputs, or null.
int check_closest_args(svo_ctx *ctx, const void *queries, size_t n, const svo_closest_params *params, const char *out_error,
                       svo_closest_params *k) {
    static_assert(sizeof(svo_closest) == sizeof(svo_nearest::Closest), "closest record layout");
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!queries) return fail(SVO_ERR_ARG, "null query list");
    if (out_error) return fail(SVO_ERR_ARG, out_error);
    if (int rc = read_closest_params(params, k)) return rc;
    if (int rc = check_batch_count(n, 1, "queries")) return rc;
    if ((size_t)k->root >= batch_context(ctx)->capacity) return fail(SVO_ERR_ARG, "root outside the node-pool capacity");
    return SVO_OK;
}

// One closest-voxel query on context c (single-device), its device selected: arguments and pool checked by the caller.
int closest_device(svo_ctx *c, const svo_shape *d_queries, size_t n, const svo_closest_params &k, const svo_closest_out &out,
                   hipStream_t s) {
    svo::ClosestArgs a;
    std::memset(&a, 0, sizeof a);
    a.nodes = c->d_nodes;
    a.n_nodes = (uint32_t)std::min<size_t>(c->n_nodes, 0xFFFFFFFFu);
    a.queries = reinterpret_cast<const svo_volumes::Shape *>(d_queries);
    a.n = (uint32_t)n;
    a.flags = k.flags;
    a.root = k.root;
    a.max_visits = k.max_visits;
    a.coarse_level = k.coarse_level;
    a.nearest = reinterpret_cast<svo_nearest::Closest *>(out.nearest);
    a.contacts = reinterpret_cast<svo_volumes::Contact *>(out.contacts);
    a.hitmask = reinterpret_cast<unsigned long long *>(out.hitmask);
    return launched(svo::launch_closest(a, s), "closest launch");
}

}  // namespace

extern "C" {

int svo_trace_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n_rays, int stack_mode, uint32_t flags,
                   const svo_query_out *out, void *stream) {
    return svo_trace_rays_lod(ctx, d_rays, n_rays, stack_mode, flags, 0.0f, 0.0f, out, stream);
}

int svo_trace_rays_lod(svo_ctx *ctx, const svo_ray *d_rays, size_t n_rays, int stack_mode, uint32_t flags,
                       float ray_size_coef, float ray_size_bias, const svo_query_out *out, void *stream) {
    const char *out_error = !out ? "null svo_query_out"
                            : !out->hits && !out->position && !out->voxel && !out->hitmask ? "every query output is null"
                                                                                           : nullptr;
    if (int rc = check_trace_args(ctx, d_rays, n_rays, stack_mode, flags, ray_size_coef, ray_size_bias, out_error)) return rc;
    if (n_rays == 0) return SVO_OK;
    return on_device(ctx, "svo_trace_rays", stream, true, [&](svo_ctx *c, hipStream_t s) {
        return query_device(c, d_rays, n_rays, stack_mode, flags, *out, s, ray_size_coef, ray_size_bias);
    });
}

int svo_trace_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n_rays, int stack_mode, uint32_t flags,
                        svo_hit *hits, float *position, uint64_t *voxel) {
    return svo_trace_rays_lod_host(ctx, rays, n_rays, stack_mode, flags, 0.0f, 0.0f, hits, position, voxel);
}

int svo_trace_rays_lod_host(svo_ctx *ctx, const svo_ray *rays, size_t n, int stack_mode, uint32_t flags,
                            float ray_size_coef, float ray_size_bias, svo_hit *hits, float *position, uint64_t *voxel) {
    const char *out_error = !hits && !position && !voxel ? "every query output is null" : nullptr;
    if (int rc = check_trace_args(ctx, rays, n, stack_mode, flags, ray_size_coef, ray_size_bias, out_error)) return rc;
    if (n == 0) return SVO_OK;
    return traced_host(ctx, "svo_trace_rays_host", rays, n, hits, position, voxel, nullptr,
                       [&](svo_ctx *c, const svo_ray *d_rays, const svo_query_out &out, int32_t *, hipStream_t s) {
                           return query_device(c, d_rays, n, stack_mode, flags, out, s, ray_size_coef, ray_size_bias);
                       });
}

int svo_bounce_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                    const uint64_t *d_voxel, svo_ray *d_rays_out, void *stream) {
    if (int rc = check_bounce_args(ctx, d_rays, n, flags, d_hits, d_voxel, d_rays_out)) return rc;
    if (int rc = check_batch_alignment(d_rays, d_rays_out, d_hits, d_voxel)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_bounce_rays", stream, false, [&](svo_ctx *, hipStream_t s) {
        return bounce_launch(batch_of(d_rays, n, flags, d_hits, d_voxel, d_rays_out), s);
    });
}

int svo_bounce_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                         const uint64_t *voxel, svo_ray *rays_out) {
    if (int rc = check_bounce_args(ctx, rays, n, flags, hits, voxel, rays_out)) return rc;
    if (n == 0) return SVO_OK;
    return batch_host(ctx, "svo_bounce_rays_host", rays, n, flags, hits, voxel, 0, rays_out, bounce_launch);   // in place
}

int svo_ambient_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                     const uint64_t *d_voxel, int n_rays, float radius, uint32_t variant, svo_ray *d_rays_out,
                     void *stream) {
    if (int rc = check_ambient_args(ctx, d_rays, n, flags, d_hits, d_voxel, n_rays, radius, variant, d_rays_out)) return rc;
    if (int rc = check_batch_alignment(d_rays, d_rays_out, d_hits, d_voxel)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_ambient_rays", stream, false, [&](svo_ctx *, hipStream_t s) {
        return ambient_launch(batch_of(d_rays, n, flags, d_hits, d_voxel, d_rays_out), n_rays, radius, variant, s);
    });
}

int svo_ambient_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                          const uint64_t *voxel, int n_rays, float radius, uint32_t variant, svo_ray *rays_out) {
    if (int rc = check_ambient_args(ctx, rays, n, flags, hits, voxel, n_rays, radius, variant, rays_out)) return rc;
    if (n == 0) return SVO_OK;
    return batch_host(ctx, "svo_ambient_rays_host", rays, n, flags, hits, voxel, (size_t)n_rays, rays_out,
                      [&](const Batch &b, hipStream_t s) { return ambient_launch(b, n_rays, radius, variant, s); });
}

int svo_light_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                   const uint64_t *d_voxel, const svo_light *lights, int n_lights, svo_ray *d_rays_out, void *stream) {
    if (int rc = check_light_args(ctx, d_rays, n, flags, d_hits, d_voxel, lights, n_lights, d_rays_out)) return rc;
    if (int rc = check_batch_alignment(d_rays, d_rays_out, d_hits, d_voxel)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_light_rays", stream, false, [&](svo_ctx *, hipStream_t s) {
        return light_launch(batch_of(d_rays, n, flags, d_hits, d_voxel, d_rays_out), lights, n_lights, s);
    });
}

int svo_light_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                        const uint64_t *voxel, const svo_light *lights, int n_lights, svo_ray *rays_out) {
    if (int rc = check_light_args(ctx, rays, n, flags, hits, voxel, lights, n_lights, rays_out)) return rc;
    if (n == 0) return SVO_OK;
    return batch_host(ctx, "svo_light_rays_host", rays, n, flags, hits, voxel, (size_t)n_lights, rays_out,
                      [&](const Batch &b, hipStream_t s) { return light_launch(b, lights, n_lights, s); });
}

int svo_scene_light_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                         const uint64_t *d_voxel, const int32_t *d_object, const svo_object *objects, int n_objects,
                         const svo_light *lights, int n_lights, svo_ray *d_rays_out, void *stream) {
    if (int rc = check_scene_light_args(ctx, d_rays, n, flags, d_hits, d_voxel, d_object, objects, n_objects, lights, n_lights,
                                        d_rays_out))
        return rc;
    if (int rc = check_batch_alignment(d_rays, d_rays_out, d_hits, d_voxel)) return rc;
    if ((uintptr_t)d_object & 3u) return fail(SVO_ERR_ARG, "object ids must be 4-byte aligned");
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_scene_light_rays", stream, false, [&](svo_ctx *, hipStream_t s) {
        return scene_light_launch(batch_of(d_rays, n, flags, d_hits, d_voxel, d_rays_out, d_object), objects, n_objects, lights,
                                  n_lights, s);
    });
}

int svo_scene_light_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                              const uint64_t *voxel, const int32_t *object, const svo_object *objects, int n_objects,
                              const svo_light *lights, int n_lights, svo_ray *rays_out) {
    if (int rc = check_scene_light_args(ctx, rays, n, flags, hits, voxel, object, objects, n_objects, lights, n_lights, rays_out))
        return rc;
    if (n == 0) return SVO_OK;
    return batch_host(ctx, "svo_scene_light_rays_host", rays, n, flags, hits, voxel, (size_t)n_lights, rays_out,
                      [&](const Batch &b, hipStream_t s) { return scene_light_launch(b, objects, n_objects, lights, n_lights, s); },
                      object);
}

int svo_object_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_object *object,
                    svo_ray *d_rays_out, void *stream) {
    if (int rc = check_object_ray_args(ctx, d_rays, n, flags, object, d_rays_out)) return rc;
    if (int rc = check_batch_alignment(d_rays, d_rays_out, nullptr, nullptr)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_object_rays", stream, false, [&](svo_ctx *, hipStream_t s) {
        return object_rays_launch(batch_of(d_rays, n, flags, nullptr, nullptr, d_rays_out), object, s);
    });
}

int svo_object_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_object *object,
                         svo_ray *rays_out) {
    if (int rc = check_object_ray_args(ctx, rays, n, flags, object, rays_out)) return rc;
    if (n == 0) return SVO_OK;
    return batch_host(ctx, "svo_object_rays_host", rays, n, flags, nullptr, nullptr, 0, rays_out,   // in place
                      [&](const Batch &b, hipStream_t s) { return object_rays_launch(b, object, s); });
}

int svo_trace_scene(svo_ctx *ctx, const svo_ray *d_rays, size_t n, int stack_mode, uint32_t flags,
                    const svo_object *objects, int n_objects, const svo_query_out *out, int32_t *d_object, void *stream) {
    const bool any_out = d_object || (out && (out->hits || out->position || out->voxel || out->hitmask));
    if (int rc = check_scene_args(ctx, d_rays, n, stack_mode, flags, objects, n_objects, any_out)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_trace_scene", stream, true, [&](svo_ctx *c, hipStream_t s) {
        const svo_query_out none{};
        return scene_device(c, d_rays, n, stack_mode, flags, objects, n_objects, out ? *out : none, d_object, s);
    });
}

int svo_trace_scene_host(svo_ctx *ctx, const svo_ray *rays, size_t n, int stack_mode, uint32_t flags,
                         const svo_object *objects, int n_objects, svo_hit *hits, float *position, uint64_t *voxel,
                         int32_t *object) {
    if (int rc = check_scene_args(ctx, rays, n, stack_mode, flags, objects, n_objects, hits || position || voxel || object))
        return rc;
    if (n == 0) return SVO_OK;
    return traced_host(ctx, "svo_trace_scene_host", rays, n, hits, position, voxel, object,
                       [&](svo_ctx *c, const svo_ray *d_rays, const svo_query_out &out, int32_t *d_object, hipStream_t s) {
                           return scene_device(c, d_rays, n, stack_mode, flags, objects, n_objects, out, d_object, s);
                       });
}

int svo_sample_sky(svo_ctx *ctx, const float *d_dirs, size_t n, float *d_rgba, void *stream) {
    if (int rc = check_sky_args(ctx, d_dirs, n, d_rgba)) return rc;
    if (((uintptr_t)d_dirs | (uintptr_t)d_rgba) & 15u) return fail(SVO_ERR_ARG, "directions and colours must be 16-byte aligned");
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_sample_sky", stream, false,
                     [&](svo_ctx *c, hipStream_t s) { return sky_launch(c, d_dirs, n, d_rgba, s); });
}

int svo_sample_sky_host(svo_ctx *ctx, const float *dirs, size_t n, float *rgba) {
    if (int rc = check_sky_args(ctx, dirs, n, rgba)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_sample_sky_host", nullptr, false, [&](svo_ctx *c, hipStream_t s) {
        HostStage st(c);
        const size_t p_dirs = st.part(16 * n);   // the directions, 16 bytes each, sampled in place
        if (int rc = st.begin()) return rc;
        if (int rc = st.upload(p_dirs, dirs, 16 * n)) return rc;
        if (int rc = sky_launch(c, st.at(p_dirs), n, st.at(p_dirs), s)) return rc;
        if (int rc = st.download(rgba, p_dirs, 16 * n)) return rc;
        return st.finish();
    });
}

int svo_overlap_volumes(svo_ctx *ctx, const svo_shape *d_shapes, size_t n, const svo_overlap_params *params,
                        const svo_overlap_out *out, void *stream) {
    const char *out_error = !out ? "null svo_overlap_out"
                            : !out->summary && !out->contacts && !out->hitmask ? "every overlap output is null"
                                                                               : nullptr;
    svo_overlap_params k;
    if (int rc = check_overlap_args(ctx, d_shapes, n, params, out_error, out && out->contacts, &k)) return rc;
    if (((uintptr_t)d_shapes | (uintptr_t)out->summary | (uintptr_t)out->contacts) & 15u)
        return fail(SVO_ERR_ARG, "shapes, summaries and contacts must be 16-byte aligned");
    if ((uintptr_t)out->hitmask & 7u) return fail(SVO_ERR_ARG, "the hit mask must be 8-byte aligned");
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_overlap_volumes", stream, true,
                     [&](svo_ctx *c, hipStream_t s) { return overlap_device(c, d_shapes, n, k, *out, s); });
}

int svo_overlap_volumes_host(svo_ctx *ctx, const svo_shape *shapes, size_t n, const svo_overlap_params *params,
                             svo_overlap *summary, svo_contact *contacts) {
    const char *out_error = !summary && !contacts ? "every overlap output is null" : nullptr;
    svo_overlap_params k;
    if (int rc = check_overlap_args(ctx, shapes, n, params, out_error, contacts != nullptr, &k)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_overlap_volumes_host", nullptr, true, [&](svo_ctx *c, hipStream_t s) {
        HostStage st(c);
        const size_t n_contacts = contacts ? n * k.max_contacts : 0;
        const size_t p_shapes = st.part(32 * n), p_sum = st.part(summary ? 16 * n : 0), p_con = st.part(16 * n_contacts);
        if (int rc = st.begin()) return rc;
        if (int rc = st.upload(p_shapes, shapes, 32 * n)) return rc;
        svo_overlap_out out{};
        out.summary = st.at_if<svo_overlap>(summary, p_sum);
        out.contacts = st.at_if<svo_contact>(contacts, p_con);
        if (int rc = overlap_device(c, st.at<const svo_shape>(p_shapes), n, k, out, s)) return rc;
        if (int rc = st.download(summary, p_sum, 16 * n)) return rc;
        if (int rc = st.download(contacts, p_con, 16 * n_contacts)) return rc;
        return st.finish();
    });
}

int svo_closest_voxels(svo_ctx *ctx, const svo_shape *d_queries, size_t n, const svo_closest_params *params,
                       const svo_closest_out *out, void *stream) {
    const char *out_error = !out ? "null svo_closest_out"
                            : !out->nearest && !out->contacts && !out->hitmask ? "every closest output is null"
                                                                               : nullptr;
    svo_closest_params k;
    if (int rc = check_closest_args(ctx, d_queries, n, params, out_error, &k)) return rc;
    if (((uintptr_t)d_queries | (uintptr_t)out->nearest | (uintptr_t)out->contacts) & 15u)
        return fail(SVO_ERR_ARG, "queries, nearest records and contacts must be 16-byte aligned");
    if ((uintptr_t)out->hitmask & 7u) return fail(SVO_ERR_ARG, "the hit mask must be 8-byte aligned");
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_closest_voxels", stream, true,
                     [&](svo_ctx *c, hipStream_t s) { return closest_device(c, d_queries, n, k, *out, s); });
}

int svo_closest_voxels_host(svo_ctx *ctx, const svo_shape *queries, size_t n, const svo_closest_params *params,
                            svo_closest *nearest, svo_contact *contacts) {
    const char *out_error = !nearest && !contacts ? "every closest output is null" : nullptr;
    svo_closest_params k;
    if (int rc = check_closest_args(ctx, queries, n, params, out_error, &k)) return rc;
    if (n == 0) return SVO_OK;
    return on_device(ctx, "svo_closest_voxels_host", nullptr, true, [&](svo_ctx *c, hipStream_t s) {
        HostStage st(c);
        const size_t p_queries = st.part(32 * n), p_near = st.part(nearest ? 32 * n : 0), p_con = st.part(contacts ? 16 * n : 0);
        if (int rc = st.begin()) return rc;
        if (int rc = st.upload(p_queries, queries, 32 * n)) return rc;
        svo_closest_out out{};
        out.nearest = st.at_if<svo_closest>(nearest, p_near);
        out.contacts = st.at_if<svo_contact>(contacts, p_con);
        if (int rc = closest_device(c, st.at<const svo_shape>(p_queries), n, k, out, s)) return rc;
        if (int rc = st.download(nearest, p_near, 32 * n)) return rc;
        if (int rc = st.download(contacts, p_con, contacts ? 16 * n : 0)) return rc;
        return st.finish();
    });
}

int svo_get_config(svo_ctx *ctx, svo_config *cfg) {
    if (!cfg) return fail(SVO_ERR_ARG, "cfg is null");
    if (cfg->size < 2 * sizeof(uint32_t)) return fail(SVO_ERR_ARG, "svo_config.size must hold at least size and version");
    static const svo_ctx defaults;
    svo_config k;
    config_of(ctx ? ctx : &defaults, &k);
    const size_t n = std::min<size_t>(cfg->size, sizeof k);
    k.size = (uint32_t)n;
    std::memcpy(cfg, &k, n);
    return SVO_OK;
}

int svo_set_config(svo_ctx *ctx, const svo_config *cfg) {
    if (!ctx || !cfg) return fail(SVO_ERR_ARG, "null argument");
    if (cfg->size < 2 * sizeof(uint32_t)) return fail(SVO_ERR_ARG, "svo_config.size must hold at least size and version");
    if (cfg->size > sizeof(svo_config))
        return fail(SVO_ERR_ARG, "svo_config.size " + std::to_string(cfg->size) + " is larger than this library's (" +
                                     std::to_string(sizeof(svo_config)) + "): a newer ABI");
    svo_config k;
    config_of(ctx, &k);   // fields past the caller's size keep the context's values
    std::memcpy(&k, cfg, cfg->size);
    k.size = sizeof k;
    k.version = SVO_CONFIG_VERSION;
    int rc = check_config(k);
    if (rc) return rc;
    if (is_multi(ctx)) {
        for (svo_ctx *m : ctx->members) {
            rc = apply_config(m, k);
            if (rc) return rc;
        }
        if (k.peer_copy != ctx->peer_copy) {   // the members' payload routes: frames in flight first
            for (svo_ctx *m : ctx->members) {
                HIP_TRY(hipSetDevice(m->device));
                HIP_TRY(hipDeviceSynchronize());
            }
            HIP_TRY(hipSetDevice(ctx->members[0]->device));
            for (size_t i = 1; i < ctx->peers.size(); ++i)
                ctx->peers[i].link = k.peer_copy ? SVO_LINK_COPY : ctx->peers[i].native_link;
        }
    }
    return apply_config(ctx, k);
}

int svo_beam_starts(svo_ctx *ctx, int width, int height, const svo_band *band, float *d_starts, void *stream) {
    if (!d_starts) return fail(SVO_ERR_ARG, "d_starts is null");
    if (ctx && is_multi(ctx)) return fail(SVO_ERR_ARG, "beam starts of a member context (svo_get_member)");
    svo::Outputs o{};
    o.starts = d_starts;
    return launch(ctx, width, height, SVO_STACK_HLSL, band, o, reinterpret_cast<hipStream_t>(stream));
}

int svo_abi_version(void) { return 10; }

const char *svo_last_error(void) { return g_last_error.c_str(); }

int svo_create(int device, size_t capacity_nodes, svo_ctx **out) {
    if (!out) return fail(SVO_ERR_ARG, "out is null");
    *out = nullptr;
    if (capacity_nodes == 0 || capacity_nodes > (size_t)0xFFFFFFFFu)
        return fail(SVO_ERR_ARG, "capacity_nodes must be in [1, 2^32)");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SVO_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    svo_ctx *ctx = new (std::nothrow) svo_ctx();
    if (!ctx) return fail(SVO_ERR_ARG, "out of host memory");
    ctx->device = device;
    ctx->capacity = capacity_nodes;
    hipError_t e = hipMalloc(&ctx->d_nodes, capacity_nodes * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&ctx->d_att, capacity_nodes * sizeof(uint2));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    // zero-filled pool: descriptors never uploaded read as empty (0), like the
    // fresh ComputeBuffers of RaytracingMaster.InitializeSVOBuffer
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_nodes, 0, capacity_nodes * sizeof(uint2), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_att, 0, capacity_nodes * sizeof(uint2), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device);
    int lds_block = 0;
    if (e == hipSuccess) e = hipDeviceGetAttribute(&lds_block, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (e == hipSuccess && lds_block > 0) ctx->lds_per_block = (size_t)lds_block;
    // diagnostics only (svo_rt.h): traces and timing aids, never a policy
    if (const char *k = std::getenv("SVO_DEBUG")) ctx->debug = std::atoi(k);
    if (const char *k = std::getenv("SVO_WAVE_LOG")) ctx->wave_log_path = k;
    if (const char *k = std::getenv("SVO_BEAM_DIAG")) ctx->beam_diag = (uint32_t)std::atoi(k);
    if (e != hipSuccess) {
        destroy_single(ctx);
        return fail(SVO_ERR_HIP, std::string("svo_create: ") + hipGetErrorString(e));
    }
    *out = ctx;
    return SVO_OK;
}

int svo_create_multi(const int *devices, int num_devices, size_t capacity_nodes, int band_rows, svo_ctx **out) {
    if (!out || !devices) return fail(SVO_ERR_ARG, "null argument");
    *out = nullptr;
    if (num_devices < 1 || num_devices > svo::MAX_PARTS) return fail(SVO_ERR_ARG, "num_devices must be in [1, 64]");
    if (band_rows <= 0) return fail(SVO_ERR_ARG, "band_rows must be positive");
    svo_ctx *g = new (std::nothrow) svo_ctx();
    if (!g) return fail(SVO_ERR_ARG, "out of host memory");
    g->device = devices[0];
    g->capacity = capacity_nodes;
    g->band_rows = band_rows;
    g->peers.resize(num_devices);
    auto bail = [&](int rc) {
        svo_destroy(g);
        return rc;
    };
    for (int i = 0; i < num_devices; ++i) {
        svo_ctx *m = nullptr;
        int rc = svo_create(devices[i], capacity_nodes, &m);
        if (rc) return bail(rc);
        g->members.push_back(m);
    }
    // the display device reads every other device's payload over xGMI (peer access);
    // a member it cannot map gets the copy fallback (SVO_LINK_COPY, multi_render).
    // svo_config.peer_copy forces the copy for every member but the display device itself
    // (the one-GPU test of that path: a repeated device index)
    for (int i = 1; i < num_devices; ++i) {
        Peer &pr = g->peers[i];
        if (devices[i] == devices[0]) {
            pr.native_link = pr.link = SVO_LINK_SELF;
            continue;
        }
        int ok = 0;
        hipError_t e = hipDeviceCanAccessPeer(&ok, devices[0], devices[i]);
        if (e != hipSuccess || !ok) {
            (void)hipGetLastError();
            pr.native_link = pr.link = SVO_LINK_COPY;
            continue;
        }
        hipSetDevice(devices[0]);
        e = hipDeviceEnablePeerAccess(devices[i], 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) {
            (void)hipGetLastError();
            pr.native_link = pr.link = SVO_LINK_PEER;
        } else {   // reported as possible, refused when enabled: copy instead
            (void)hipGetLastError();
            pr.native_link = pr.link = SVO_LINK_COPY;
        }
    }
    for (int i = 1; i < num_devices; ++i) {
        hipSetDevice(devices[i]);
        for (int j = 0; j < 2; ++j)
            if (hipEventCreateWithFlags(&g->peers[i].rendered[j], hipEventDisableTiming) != hipSuccess)
                return bail(fail(SVO_ERR_HIP, "hipEventCreate"));
    }
    hipSetDevice(devices[0]);
    for (int j = 0; j < 2; ++j)
        if (hipEventCreateWithFlags(&g->gathered[j], hipEventDisableTiming) != hipSuccess)
            return bail(fail(SVO_ERR_HIP, "hipEventCreate"));
    *out = g;
    return SVO_OK;
}

int svo_set_band_deal(svo_ctx *ctx, int cycle, const uint8_t *owner) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!is_multi(ctx)) return fail(SVO_ERR_ARG, "svo_set_band_deal needs a multi-device context");
    if (cycle < 0 || cycle > svo::MAX_CYCLE) return fail(SVO_ERR_ARG, "cycle must be in [0, 256]");
    if (cycle > 0 && !owner) return fail(SVO_ERR_ARG, "owner is null");
    const int n = (int)ctx->members.size();
    for (int i = 0; i < cycle; ++i)
        if (owner[i] >= n) return fail(SVO_ERR_ARG, "owner entry names no member");
    // payload sizes change: let frames in flight finish with the old deal first
    for (svo_ctx *m : ctx->members) {
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipDeviceSynchronize());
    }
    ctx->deal_cycle = cycle;
    for (int i = 0; i < cycle; ++i) ctx->deal_owner[i] = owner[i];
    return SVO_OK;
}

int svo_num_devices(svo_ctx *ctx, int *n) {
    if (!ctx || !n) return fail(SVO_ERR_ARG, "null argument");
    *n = is_multi(ctx) ? (int)ctx->members.size() : 1;
    return SVO_OK;
}

int svo_get_member_link(svo_ctx *ctx, int index, int *device, int *link) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    const int n = is_multi(ctx) ? (int)ctx->members.size() : 1;
    if (index < 0 || index >= n) return fail(SVO_ERR_ARG, "member index out of range");
    if (device) *device = is_multi(ctx) ? ctx->members[index]->device : ctx->device;
    if (link) *link = is_multi(ctx) && index > 0 ? ctx->peers[index].link : SVO_LINK_SELF;
    return SVO_OK;
}

int svo_get_member(svo_ctx *ctx, int index, svo_ctx **member) {
    if (!ctx || !member) return fail(SVO_ERR_ARG, "null argument");
    const int n = is_multi(ctx) ? (int)ctx->members.size() : 1;
    if (index < 0 || index >= n) return fail(SVO_ERR_ARG, "member index out of range");
    *member = is_multi(ctx) ? ctx->members[index] : ctx;
    return SVO_OK;
}

int svo_set_buffer(svo_ctx *ctx, const int32_t *desc, size_t n_desc, const uint32_t *att,
                   size_t n_att, size_t dst_offset) {
    if (!ctx || (!desc && n_desc) || (!att && n_att)) return fail(SVO_ERR_ARG, "null argument");
    if (is_multi(ctx)) {   // validated and uploaded once, then replicated device to device
        int rc = svo_set_buffer(ctx->members[0], desc, n_desc, att, n_att, dst_offset);
        if (rc) return rc;
        return replicate_upload(ctx, dst_offset, n_desc);
    }
    if (dst_offset + n_desc > ctx->capacity || 2 * dst_offset + n_att > 2 * ctx->capacity)
        return fail(SVO_ERR_CAPACITY, "upload exceeds node-pool capacity");
    if (n_att != 2 * n_desc) return fail(SVO_ERR_ARG, "attachments must hold 2 words per descriptor");
    if (n_desc == 0) return SVO_OK;
    // host-side validation walk on the absolute view
    std::vector<uint32_t> lo(n_desc), first(n_desc);
    for (size_t i = 0; i < n_desc; ++i) {
        uint32_t cd = (uint32_t)desc[i];
        lo[i] = cd & 0xFFFFu;
        first[i] = cd ? (uint32_t)(dst_offset + i) + (cd >> 16) : 0u;
    }
    Upload u;
    int rc = validate_upload(ctx, lo.data(), first.data(), n_desc, dst_offset, &u);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // renders, assembles and accumulations on any stream may still read the pool
    HIP_TRY(hipDeviceSynchronize());
    if (n_desc > ctx->stage_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        rc = regrow(&ctx->d_stage, &ctx->stage_cap, n_desc, n_desc * sizeof(int32_t));
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_stage, desc, n_desc * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    unsigned blocks = (unsigned)((n_desc + 255) / 256);
    hipLaunchKernelGGL(convert_v1_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->d_stage,
                       ctx->d_nodes, n_desc, (uint32_t)dst_offset);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->d_att + dst_offset, att, n_att * sizeof(uint32_t), hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return commit_upload(ctx, u);
}

int svo_set_buffer_v2(svo_ctx *ctx, const uint64_t *nodes, size_t n_nodes, const uint32_t *att,
                      size_t n_att, size_t dst_offset) {
    if (!ctx || (!nodes && n_nodes) || (!att && n_att)) return fail(SVO_ERR_ARG, "null argument");
    if (is_multi(ctx)) {
        int rc = svo_set_buffer_v2(ctx->members[0], nodes, n_nodes, att, n_att, dst_offset);
        if (rc) return rc;
        return replicate_upload(ctx, dst_offset, n_nodes);
    }
    if (dst_offset + n_nodes > ctx->capacity) return fail(SVO_ERR_CAPACITY, "upload exceeds node-pool capacity");
    if (n_att != 2 * n_nodes) return fail(SVO_ERR_ARG, "attachments must hold 2 words per node");
    if (n_nodes == 0) return SVO_OK;
    std::vector<uint32_t> lo(n_nodes), first(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) {
        lo[i] = (uint32_t)nodes[i];
        first[i] = (uint32_t)(nodes[i] >> 32);
        if (lo[i] > 0xFFFFu) return fail(SVO_ERR_FORMAT, "v2 node low word must only hold the two masks");
    }
    Upload u;
    int rc = validate_upload(ctx, lo.data(), first.data(), n_nodes, dst_offset, &u);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());   // as in svo_set_buffer
    static_assert(sizeof(uint2) == sizeof(uint64_t), "node layout");
    HIP_TRY(hipMemcpyAsync(ctx->d_nodes + dst_offset, nodes, n_nodes * sizeof(uint64_t), hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_att + dst_offset, att, n_att * sizeof(uint32_t), hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return commit_upload(ctx, u);
}

int svo_set_camera(svo_ctx *ctx, const float c2w[16], const float inv_proj[16], float px_off_x,
                   float px_off_y, const float light[4]) {
    if (!ctx || !c2w || !inv_proj || !light) return fail(SVO_ERR_ARG, "null argument");
    for (svo_ctx *m : ctx->members) svo_set_camera(m, c2w, inv_proj, px_off_x, px_off_y, light);
    // a moved camera changes the tiles' costs: the next launch refreshes the dispatch order
    // (a new pixel offset or light alone does not)
    if (!ctx->cam_set || std::memcmp(ctx->cam.c2w, c2w, sizeof(ctx->cam.c2w)) != 0 ||
        std::memcmp(ctx->cam.inv_proj, inv_proj, sizeof(ctx->cam.inv_proj)) != 0)
        ++ctx->view_gen;
    if (!ctx->cam_set || ctx->cam.px_off[0] != px_off_x || ctx->cam.px_off[1] != px_off_y ||
        std::memcmp(ctx->cam.light, light, sizeof(ctx->cam.light)) != 0)
        ++ctx->cost_gen;
    std::memcpy(ctx->cam.c2w, c2w, sizeof(ctx->cam.c2w));
    std::memcpy(ctx->cam.inv_proj, inv_proj, sizeof(ctx->cam.inv_proj));
    ctx->cam.px_off[0] = px_off_x;
    ctx->cam.px_off[1] = px_off_y;
    std::memcpy(ctx->cam.light, light, sizeof(ctx->cam.light));
    ctx->cam_set = true;
    return SVO_OK;
}

int svo_set_lod(svo_ctx *ctx, float ray_size_coef, float ray_size_bias) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!lod_pair_ok(ray_size_coef, ray_size_bias)) return fail(SVO_ERR_ARG, LOD_PAIR_MSG);
    for (svo_ctx *m : ctx->members) svo_set_lod(m, ray_size_coef, ray_size_bias);
    ray_size_coef += 0.0f;   // -0 -> +0
    ray_size_bias += 0.0f;
    // another pair: other hits and other tile costs -- the streams' orders rebuild as after a camera move
    if (ctx->lod_coef != ray_size_coef || ctx->lod_bias != ray_size_bias) ++ctx->view_gen;
    ctx->lod_coef = ray_size_coef;
    ctx->lod_bias = ray_size_bias;
    return SVO_OK;
}

int svo_set_reflection(svo_ctx *ctx, const float specular[3], int max_bounces) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3 && specular; ++k) {
        if (!(specular[k] >= 0.0f && specular[k] <= 1.0f)) return fail(SVO_ERR_ARG, "specular components must lie in [0, 1]");
        s[k] = specular[k];
    }
    if (max_bounces < 0 || max_bounces > 7) return fail(SVO_ERR_ARG, "max_bounces must lie in 0..7");
    const bool on = max_bounces > 0 && (s[0] != 0.0f || s[1] != 0.0f || s[2] != 0.0f);
    if (on && is_multi(ctx))
        return fail(SVO_ERR_STATE, "reflection on a multi-device context is not supported");
    for (int k = 0; k < 3; ++k) ctx->specular[k] = s[k];
    ctx->max_bounces = max_bounces;
    return SVO_OK;
}

int svo_get_reflection(svo_ctx *ctx, float specular[3], int *max_bounces) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    for (int k = 0; k < 3 && specular; ++k) specular[k] = ctx->specular[k];
    if (max_bounces) *max_bounces = ctx->max_bounces;
    return SVO_OK;
}

int svo_set_ambient(svo_ctx *ctx, const float ambient[3], int n_rays, float radius, uint32_t variant) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    float a[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3 && ambient; ++k) {
        if (!(ambient[k] >= 0.0f && ambient[k] <= 4.0f)) return fail(SVO_ERR_ARG, "ambient components must lie in [0, 4]");
        a[k] = ambient[k];
    }
    if (n_rays != 0 && !svo_ambient::valid_count(n_rays)) return fail(SVO_ERR_ARG, "n_rays must be 0, 4, 8 or 16");
    if (const char *msg = ambient_setting_error(n_rays ? n_rays : 4, radius, variant)) return fail(SVO_ERR_ARG, msg);
    const bool on = n_rays > 0 && (a[0] != 0.0f || a[1] != 0.0f || a[2] != 0.0f);
    if (on && is_multi(ctx))
        return fail(SVO_ERR_STATE, "an ambient term on a multi-device context is not supported");
    for (int k = 0; k < 3; ++k) ctx->ambient[k] = a[k];
    ctx->ambient_rays = n_rays;
    ctx->ambient_radius = radius;
    ctx->ambient_variant = variant;
    return SVO_OK;
}

int svo_get_ambient(svo_ctx *ctx, float ambient[3], int *n_rays, float *radius, uint32_t *variant) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    for (int k = 0; k < 3 && ambient; ++k) ambient[k] = ctx->ambient[k];
    if (n_rays) *n_rays = ctx->ambient_rays;
    if (radius) *radius = ctx->ambient_radius;
    if (variant) *variant = ctx->ambient_variant;
    return SVO_OK;
}

int svo_set_lights(svo_ctx *ctx, const svo_light *lights, int n_lights) {
    if (int rc = check_light_list(lights, n_lights)) return rc;   // before the context is read
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    const int n = lights ? n_lights : 0;
    if (n > 0 && is_multi(ctx)) return fail(SVO_ERR_STATE, "lights on a multi-device context are not supported");
    for (int j = 0; j < svo_lights::MAX_LIGHTS; ++j) {
        svo_lights::Light l{};
        if (j < n) std::memcpy(&l, lights + j, sizeof l);
        ctx->lights[j] = l;
    }
    ctx->n_lights = n;
    return SVO_OK;
}

int svo_get_lights(svo_ctx *ctx, svo_light *lights, int cap, int *n_lights) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    for (int j = 0; lights && j < cap && j < ctx->n_lights; ++j) std::memcpy(lights + j, ctx->lights + j, sizeof(svo_light));
    if (n_lights) *n_lights = ctx->n_lights;
    return SVO_OK;
}

int svo_set_objects(svo_ctx *ctx, const svo_object *objects, int n_objects) {
    if (int rc = check_object_list(objects, n_objects)) return rc;   // before the context is read
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    const int n = objects ? n_objects : 0;
    if (n > 0 && is_multi(ctx)) return fail(SVO_ERR_STATE, "objects on a multi-device context are not supported");
    if (int rc = check_object_roots(ctx, objects, n)) return rc;
    for (int j = 0; j < svo_objects::MAX_OBJECTS; ++j) {
        svo_objects::Object ob{};
        if (j < n) std::memcpy(&ob, objects + j, sizeof ob);
        ctx->objects[j] = ob;
    }
    ctx->n_objects = n;
    return SVO_OK;
}

int svo_get_objects(svo_ctx *ctx, svo_object *objects, int cap, int *n_objects) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    for (int j = 0; objects && j < cap && j < ctx->n_objects; ++j) std::memcpy(objects + j, ctx->objects + j, sizeof(svo_object));
    if (n_objects) *n_objects = ctx->n_objects;
    return SVO_OK;
}

int svo_set_skybox(svo_ctx *ctx, const float *rgba, int width, int height, uint32_t flags) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (flags & ~(uint32_t)(SVO_SKY_BILINEAR | SVO_SKY_CLAMP_V)) return fail(SVO_ERR_ARG, "unknown skybox flag bits");
    if (rgba) {
        if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "skybox width/height must be positive");
        if (width > svo_sky::MAX_DIM || height > svo_sky::MAX_DIM)
            return fail(SVO_ERR_ARG, "skybox width/height must not exceed " + std::to_string(svo_sky::MAX_DIM));
        const size_t n = (size_t)width * (size_t)height;
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {   // alpha is ignored
                const float c = rgba[4 * i + k];
                if (!(c >= 0.0f && c <= std::numeric_limits<float>::max()))
                    return fail(SVO_ERR_ARG, "skybox colour components must be finite and non-negative");
            }
        if (is_multi(ctx)) return fail(SVO_ERR_STATE, "a skybox texture on a multi-device context is not supported");
    }
    if (!rgba && !ctx->sky.texels) return SVO_OK;   // nothing set, nothing to release (a multi-device context too)
    HIP_TRY(hipSetDevice(ctx->device));
    // renders, queries and svo_sample_sky on any stream may still read the previous texture
    HIP_TRY(hipDeviceSynchronize());
    if (ctx->sky.texels) hipFree(const_cast<svo_sky::Texel *>(ctx->sky.texels));
    ctx->sky = svo_sky::Texture{nullptr, 0, 0, 0u};
    if (!rgba) return SVO_OK;
    const size_t bytes = (size_t)width * (size_t)height * sizeof(svo_sky::Texel);
    svo_sky::Texel *d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    const hipError_t e = hipMemcpy(d, rgba, bytes, hipMemcpyHostToDevice);   // blocking: SetData semantics
    if (e != hipSuccess) {
        hipFree(d);
        return fail(SVO_ERR_HIP, std::string("skybox upload: ") + hipGetErrorString(e));
    }
    ctx->sky = svo_sky::Texture{d, width, height, flags};
    return SVO_OK;
}

int svo_get_skybox(svo_ctx *ctx, int *width, int *height, uint32_t *flags) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (width) *width = ctx->sky.width;
    if (height) *height = ctx->sky.height;
    if (flags) *flags = ctx->sky.flags;
    return SVO_OK;
}

int svo_get_lod(svo_ctx *ctx, float *ray_size_coef, float *ray_size_bias) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (ray_size_coef) *ray_size_coef = ctx->lod_coef;
    if (ray_size_bias) *ray_size_bias = ctx->lod_bias;
    return SVO_OK;
}

int svo_render_frame(svo_ctx *ctx, int width, int height, int stack_mode, const svo_band *band,
                     const svo_frame *frame, void *stream) {
    if (!ctx || !frame) return fail(SVO_ERR_ARG, "null argument");
    if (is_multi(ctx)) {
        if (band && band->band_count != 1) return fail(SVO_ERR_ARG, "a multi-device context splits the frame itself");
        if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
        return multi_render(ctx, width, height, stack_mode, frame, reinterpret_cast<hipStream_t>(stream));
    }
    return launch(ctx, width, height, stack_mode, band, outputs_of(frame), reinterpret_cast<hipStream_t>(stream));
}

int svo_render_samples(svo_ctx *ctx, int width, int height, int stack_mode, const svo_band *band, int n_samples,
                       const float *px_offsets, uint32_t first_sample, float *d_accum, uint32_t *d_rgba8,
                       uint8_t *d_rgb8, int layout, void *stream) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (n_samples < 1 || n_samples > svo::MAX_SAMPLES) return fail(SVO_ERR_ARG, "n_samples must be in [1, 8]");
    if (!px_offsets || !d_accum) return fail(SVO_ERR_ARG, "null px_offsets or d_accum");
    if ((uintptr_t)d_accum & 15u) return fail(SVO_ERR_ARG, "d_accum must be 16-byte aligned");
    if (layout != SVO_LAYOUT_BAND && layout != SVO_LAYOUT_FRAME) return fail(SVO_ERR_ARG, "unknown layout");
    SampleArgs sa{n_samples, px_offsets, first_sample, reinterpret_cast<float4 *>(d_accum), d_rgba8, d_rgb8, layout};
    if (is_multi(ctx)) {   // the frame split over the members, each blending its own rows on its own device
        if (band && band->band_count != 1) return fail(SVO_ERR_ARG, "a multi-device context splits the frame itself");
        if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
        if (!d_rgba8 || d_rgb8) return fail(SVO_ERR_ARG, "a multi-device context assembles d_rgba8 (d_rgb8 must be NULL)");
        svo_frame f{};
        f.rgba8 = d_rgba8;
        f.layout = SVO_LAYOUT_FRAME;
        sa.layout = SVO_LAYOUT_FRAME;
        return multi_render(ctx, width, height, stack_mode, &f, reinterpret_cast<hipStream_t>(stream), &sa);
    }
    return launch(ctx, width, height, stack_mode, band, svo::Outputs{}, reinterpret_cast<hipStream_t>(stream), &sa);
}

int svo_assemble_frame(svo_ctx *ctx, int width, int height, const svo_band *deal, int n_parts,
                       const void *const *parts, int part_format, int skip_part, const svo_frame *frame,
                       void *stream) {
    if (!ctx || !parts || !frame || !deal) return fail(SVO_ERR_ARG, "null argument");
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    svo::Outputs o = outputs_of(frame);
    int rc = check_assemble_args(c, width, height, n_parts, part_format, skip_part, o);
    if (rc) return rc;
    if (deal->band_count != n_parts) return fail(SVO_ERR_ARG, "deal band_count must equal n_parts");
    svo_band db = *deal;
    db.band_rank = 0;
    Deal d;
    rc = check_band(&db, height, &d);
    if (rc) return rc;
    for (int i = 0; i < n_parts; ++i)
        if (!parts[i] && i != skip_part) return fail(SVO_ERR_ARG, "null part pointer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    // no ordering against the context's render streams: the assemble reads only the
    // caller's parts and the (upload-synchronised) attachments and writes only the
    // caller's frame, so a gather stream beside the render stream runs concurrently
    // (ordering the two made the display rank's step 1.3x slower, tools/rank0_cost.py)
    return assemble(c, width, height, d, n_parts, parts, part_format, skip_part, o, s);
}

int svo_render(svo_ctx *ctx, int width, int height, int stack_mode, float *rgba_out, svo_hit *hits_out) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
    size_t px = (size_t)width * (size_t)height;
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_out(c, px);
    if (rc) return rc;
    rc = order_scratch(c, c->stream);
    if (rc) return rc;
    svo_frame f{};
    f.hits = hits_out ? reinterpret_cast<svo_hit *>(c->d_out_hits) : nullptr;
    f.rgba = rgba_out ? reinterpret_cast<float *>(c->d_out_rgba) : nullptr;
    f.layout = SVO_LAYOUT_FRAME;
    if (is_multi(ctx)) {
        if (!hits_out && !rgba_out) return SVO_OK;
        rc = multi_render(ctx, width, height, stack_mode, &f, c->stream);
    } else {
        rc = launch(c, width, height, stack_mode, nullptr, outputs_of(&f), c->stream);
    }
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // The outputs reach the caller's pageable arrays through plugin-owned pinned staging: the DMA of
    // chunk i (at the link's rate) runs while host threads copy chunk i - 1 out of the staging
    // (a pageable hipMemcpy stages through the runtime's own small buffer: ~13 GB/s, 6.2 ms for the
    // 83 MB of a 1080p frame, BENCH_r04.json host_path).
    const size_t hb = hits_out ? px * sizeof(svo_hit) : 0, rb = rgba_out ? px * 4 * sizeof(float) : 0;
    if (c->h_stage_cap < hb + rb) {
        if (c->h_stage) hipHostFree(c->h_stage);
        c->h_stage = nullptr;
        c->h_stage_cap = 0;
        HIP_TRY(hipHostMalloc(&c->h_stage, hb + rb, hipHostMallocDefault));
        c->h_stage_cap = hb + rb;
    }
    if (!c->stage_ev[0])
        for (int i = 0; i < svo_ctx::STAGE_CHUNKS; ++i)
            HIP_TRY(hipEventCreateWithFlags(&c->stage_ev[i], hipEventDisableTiming));
    if (!c->copy_pool) {
        const int n = c->host_copy_threads > 0 ? c->host_copy_threads : (int)std::thread::hardware_concurrency() / 2;
        c->copy_pool.reset(new CopyPool(std::max(1, std::min(n, 16))));
    }
    struct Part { char *dst; const char *dev; char *stage; size_t bytes; };
    Part parts[2];
    int np = 0;
    if (hb) parts[np++] = {reinterpret_cast<char *>(hits_out), static_cast<const char *>(c->d_out_hits),
                           static_cast<char *>(c->h_stage), hb};
    if (rb) parts[np++] = {reinterpret_cast<char *>(rgba_out), static_cast<const char *>(c->d_out_rgba),
                           static_cast<char *>(c->h_stage) + hb, rb};
    const size_t total = hb + rb;
    const size_t chunk = ((total + svo_ctx::STAGE_CHUNKS - 1) / svo_ctx::STAGE_CHUNKS + 4095) & ~(size_t)4095;
    // chunk i covers bytes [i chunk, (i + 1) chunk) of the concatenated outputs
    auto for_range = [&](size_t lo, size_t hi, auto fn) {
        size_t base = 0;
        for (int k = 0; k < np; ++k) {
            const size_t a = std::max(lo, base), b = std::min(hi, base + parts[k].bytes);
            if (a < b) fn(parts[k], a - base, b - a);
            base += parts[k].bytes;
        }
    };
    int n_chunks = 0;
    for (size_t lo = 0; lo < total; lo += chunk, ++n_chunks) {
        const size_t hi = std::min(total, lo + chunk);
        hipError_t e = hipSuccess;
        for_range(lo, hi, [&](const Part &q, size_t off, size_t n) {
            if (e == hipSuccess) e = hipMemcpyAsync(q.stage + off, q.dev + off, n, hipMemcpyDeviceToHost, c->stream);
        });
        HIP_TRY(e);
        HIP_TRY(hipEventRecord(c->stage_ev[n_chunks], c->stream));
    }
    CopyPool &pool = *c->copy_pool;
    // every exit waits for the copy threads: none may still write the caller's arrays, or read the
    // staging, once this call has returned (an error included)
    struct WaitPool {
        CopyPool &p;
        ~WaitPool() { p.wait(); }
    } wait_pool{pool};
    for (int i = 0; i < n_chunks; ++i) {
        HIP_TRY(hipEventSynchronize(c->stage_ev[i]));
        const size_t lo = (size_t)i * chunk, hi = std::min(total, lo + chunk);
        for_range(lo, hi, [&](const Part &q, size_t off, size_t n) {
            const size_t per = ((n + pool.size() - 1) / pool.size() + 63) & ~(size_t)63;
            for (size_t o = 0; o < n; o += per) pool.submit(q.dst + off + o, q.stage + off + o, std::min(per, n - o));
        });
    }
    return SVO_OK;
}

int svo_render_progressive(svo_ctx *ctx, int width, int height, int stack_mode, uint32_t sample,
                           uint32_t *rgba8_out, float *rgba_out) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!rgba8_out && !rgba_out) return fail(SVO_ERR_ARG, "no output requested");
    if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
    const size_t px = (size_t)width * (size_t)height;
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_out(c, px);
    if (rc) return rc;
    bool fresh = false;
    rc = ensure_accum(c, width, height, &fresh);
    if (rc) return rc;
    if (fresh) sample = 0;   // a resized target: this sample replaces the (zeroed) frame
    rc = order_scratch(c, c->stream);
    if (rc) return rc;
    struct AmbientStep {   // this sample's ambient variant: (variant + sample) & 7, for this launch only
        svo_ctx *c;
        ~AmbientStep() { c->ambient_step = 0; }
    } ambient_step{c};
    c->ambient_step = sample & 7u;
    svo_frame f{};
    f.rgba = reinterpret_cast<float *>(c->d_out_rgba);   // this sample's Result
    f.layout = SVO_LAYOUT_FRAME;
    rc = is_multi(ctx) ? multi_render(ctx, width, height, stack_mode, &f, c->stream)
                       : launch(c, width, height, stack_mode, nullptr, outputs_of(&f), c->stream);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = svo::launch_accumulate(c->d_accum, reinterpret_cast<const float4 *>(c->d_out_rgba), px, sample,
                                          c->num_cus, c->stream);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("accumulate launch: ") + hipGetErrorString(e));
    if (rgba8_out) {
        e = svo::launch_pack_rgba8(c->d_accum, c->d_accum8, px, c->num_cus, c->stream);
        if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("pack launch: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(rgba8_out, c->d_accum8, px * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (rgba_out)
        HIP_TRY(hipMemcpyAsync(rgba_out, c->d_accum, px * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SVO_OK;
}

int svo_render_progressive_async(svo_ctx *ctx, int width, int height, int stack_mode, uint32_t sample,
                                 int pixel_format, const void **frame_out) {
    if (!ctx || !frame_out) return fail(SVO_ERR_ARG, "null argument");
    *frame_out = nullptr;
    if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
    if (pixel_format != SVO_PIXELS_RGBA8 && pixel_format != SVO_PIXELS_RGB8)
        return fail(SVO_ERR_ARG, "unknown pixel format");
    const size_t px = (size_t)width * (size_t)height;
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_out(c, px);
    if (rc) return rc;
    bool fresh = false;
    rc = ensure_accum(c, width, height, &fresh);
    if (rc) return rc;
    if (fresh) sample = 0;   // as svo_render_progressive: a resized target restarts the accumulation
    if (c->pin_format != pixel_format) {   // the slots' previous frames are in another format
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));
        if (c->copy_stream2) HIP_TRY(hipStreamSynchronize(c->copy_stream2));
        free_pinned(c);
        c->pin_format = pixel_format;
    }
    rc = ensure_pinned(c, width, height);
    if (rc) return rc;
    rc = order_scratch(c, c->stream);
    if (rc) return rc;
    struct AmbientStep {   // this sample's ambient variant: (variant + sample) & 7, for this launch only
        svo_ctx *c;
        ~AmbientStep() { c->ambient_step = 0; }
    } ambient_step{c};
    c->ambient_step = sample & 7u;
    svo_frame f{};
    f.rgba = reinterpret_cast<float *>(c->d_out_rgba);   // this sample's Result
    f.layout = SVO_LAYOUT_FRAME;
    rc = is_multi(ctx) ? multi_render(ctx, width, height, stack_mode, &f, c->stream)
                       : launch(c, width, height, stack_mode, nullptr, outputs_of(&f), c->stream);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = svo::launch_accumulate(c->d_accum, reinterpret_cast<const float4 *>(c->d_out_rgba), px, sample,
                                          c->num_cus, c->stream);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("accumulate launch: ") + hipGetErrorString(e));
    const int k = c->pin_next;
    // slot k's previous copy (PIN_SLOTS frames ago) must have read d_pin[k] before the pack overwrites it
    if (c->pin_used[k]) HIP_TRY(hipStreamWaitEvent(c->stream, c->pin_copied[k], 0));
    e = pixel_format == SVO_PIXELS_RGB8
            ? svo::launch_pack_rgb8(c->d_accum, reinterpret_cast<uint8_t *>(c->d_pin[k]), px, c->num_cus, c->stream)
            : svo::launch_pack_rgba8(c->d_accum, c->d_pin[k], px, c->num_cus, c->stream);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("pack launch: ") + hipGetErrorString(e));
    HIP_TRY(hipEventRecord(c->pin_packed[k], c->stream));
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->pin_packed[k], 0));
    const size_t fbytes = px * (pixel_format == SVO_PIXELS_RGB8 ? 3 : 4);
    if (c->pin_push == 1) {   // a kernel writes the mapped pinned buffer over PCIe
        void *dst = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dst, c->h_pin[k], 0));
        e = svo::launch_push_host(c->d_pin[k], dst, (fbytes + 15) & ~(size_t)15, c->num_cus, c->copy_stream);
        if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("push launch: ") + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(c->pin_copied[k], c->copy_stream));
    } else if (c->pin_push == 2) {   // two DMA copies of half the frame each, on two copy streams
        const size_t half = (fbytes / 2) & ~(size_t)4095;
        HIP_TRY(hipStreamWaitEvent(c->copy_stream2, c->pin_packed[k], 0));
        HIP_TRY(hipMemcpyAsync(c->h_pin[k], c->d_pin[k], half, hipMemcpyDeviceToHost, c->copy_stream));
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint8_t *>(c->h_pin[k]) + half,
                               reinterpret_cast<uint8_t *>(c->d_pin[k]) + half, fbytes - half, hipMemcpyDeviceToHost,
                               c->copy_stream2));
        HIP_TRY(hipEventRecord(c->pin_copied2[k], c->copy_stream2));
        HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->pin_copied2[k], 0));
        HIP_TRY(hipEventRecord(c->pin_copied[k], c->copy_stream));
    } else {
        HIP_TRY(hipMemcpyAsync(c->h_pin[k], c->d_pin[k], fbytes, hipMemcpyDeviceToHost, c->copy_stream));
        HIP_TRY(hipEventRecord(c->pin_copied[k], c->copy_stream));
    }
    c->pin_used[k] = true;
    c->pin_next = (k + 1) % svo_ctx::PIN_SLOTS;
    ++c->pin_frames;
    if (c->pin_frames >= 2) {   // the previous call's frame: wait for its copy only
        const int prev = (k + svo_ctx::PIN_SLOTS - 1) % svo_ctx::PIN_SLOTS;
        HIP_TRY(hipEventSynchronize(c->pin_copied[prev]));
        *frame_out = c->h_pin[prev];
    }
    return SVO_OK;
}

int svo_progressive_last(svo_ctx *ctx, const void **frame_out) {
    if (!ctx || !frame_out) return fail(SVO_ERR_ARG, "null argument");
    *frame_out = nullptr;
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    if (c->pin_frames == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int last = (c->pin_next + svo_ctx::PIN_SLOTS - 1) % svo_ctx::PIN_SLOTS;
    HIP_TRY(hipEventSynchronize(c->pin_copied[last]));
    *frame_out = c->h_pin[last];
    return SVO_OK;
}

int svo_render_device(svo_ctx *ctx, int width, int height, int stack_mode, const svo_band *band, void *d_rgba,
                      void *d_hits, void *stream) {
    svo_frame f{};
    f.hits = reinterpret_cast<svo_hit *>(d_hits);
    f.rgba = reinterpret_cast<float *>(d_rgba);
    f.layout = SVO_LAYOUT_BAND;
    if (ctx && is_multi(ctx)) {
        f.layout = SVO_LAYOUT_FRAME;
        if (!d_rgba && !d_hits) return SVO_OK;
    }
    return svo_render_frame(ctx, width, height, stack_mode, band, &f, stream);
}

int svo_pack_hits(svo_ctx *ctx, int width, int height, const svo_band *band, const void *d_rgb8, void *d_part,
                  void *stream) {
    if (!ctx || !d_rgb8 || !d_part) return fail(SVO_ERR_ARG, "null argument");
    if (width <= 0 || height <= 0) return fail(SVO_ERR_ARG, "width/height must be positive");
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    Deal d;
    int rc = check_band(band, height, &d);
    if (rc) return rc;
    const int rows = band_rows_local(height, d);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    hipError_t e = svo::launch_pack_hits(reinterpret_cast<const uint8_t *>(d_rgb8), width, rows, d_part, s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("pack hits launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

int svo_count_fetches(svo_ctx *ctx, int width, int height, int stack_mode, const svo_band *band,
                      void *d_fetches, void *stream) {
    if (!d_fetches) return fail(SVO_ERR_ARG, "d_fetches is null");
    if (ctx && is_multi(ctx)) return fail(SVO_ERR_ARG, "count fetches on a member context (svo_get_member)");
    svo::Outputs o{};
    o.fetches = reinterpret_cast<uint32_t *>(d_fetches);
    return launch(ctx, width, height, stack_mode, band, o, reinterpret_cast<hipStream_t>(stream));
}

int svo_set_options(svo_ctx *ctx, uint32_t options) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (options & ~(uint32_t)(SVO_OPT_SHADOW_RAYS | SVO_OPT_KERNEL_TIMING | SVO_OPT_COUNT_BEAM | SVO_OPT_SCENE_SHADOWS))
        return fail(SVO_ERR_ARG, "unknown option bits");
    for (svo_ctx *m : ctx->members) m->options = options;
    ctx->options = options;
    return SVO_OK;
}

int svo_stage_time(svo_ctx *ctx, int stage, double *mean_ms, uint64_t *launches) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (stage < 0 || stage >= N_STAGES) return fail(SVO_ERR_ARG, "unknown stage");
    if (is_multi(ctx)) {
        // every member records its own launches (svo_set_options sets the option on all):
        // drain them all, so none accumulates events, and report the slowest member
        double worst = 0.0;
        uint64_t worst_n = 0;
        for (svo_ctx *m : ctx->members) {
            double ms = 0.0;
            uint64_t n = 0;
            int rc = svo_stage_time(m, stage, &ms, &n);
            if (rc) return rc;
            if (n && (worst_n == 0 || ms > worst)) { worst = ms; worst_n = n; }
        }
        if (mean_ms) *mean_ms = worst;
        if (launches) *launches = worst_n;
        return SVO_OK;
    }
    svo_ctx *c = ctx;
    HIP_TRY(hipSetDevice(c->device));
    double sum = 0.0;
    uint64_t n = 0;
    hipError_t err = hipSuccess;
    for (auto &ev : c->timing_events[stage]) {
        float ms = 0.0f;
        if (err == hipSuccess) err = hipEventSynchronize(ev.second);
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev.first, ev.second);
        if (err == hipSuccess) { sum += ms; ++n; }
        c->timing_free.push_back(ev);
    }
    c->timing_events[stage].clear();
    if (err != hipSuccess) return fail(SVO_ERR_HIP, std::string("svo_stage_time: ") + hipGetErrorString(err));
    if (mean_ms) *mean_ms = n ? sum / (double)n : 0.0;
    if (launches) *launches = n;
    return SVO_OK;
}

int svo_kernel_time(svo_ctx *ctx, double *mean_ms, uint64_t *launches) {
    return svo_stage_time(ctx, STAGE_KERNEL, mean_ms, launches);
}

int svo_stage_times(svo_ctx *ctx, int stage, float *ms_out, size_t cap, size_t *launches) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (stage < 0 || stage >= N_STAGES) return fail(SVO_ERR_ARG, "unknown stage");
    if (cap && !ms_out) return fail(SVO_ERR_ARG, "ms_out is null");
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    if (is_multi(ctx))   // the other members' records are dropped, so none accumulates
        for (size_t i = 1; i < ctx->members.size(); ++i) {
            int rc = svo_stage_time(ctx->members[i], stage, nullptr, nullptr);
            if (rc) return rc;
        }
    HIP_TRY(hipSetDevice(c->device));
    size_t n = 0;
    hipError_t err = hipSuccess;
    for (auto &ev : c->timing_events[stage]) {
        float ms = 0.0f;
        if (err == hipSuccess) err = hipEventSynchronize(ev.second);
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev.first, ev.second);
        if (err == hipSuccess) {
            if (n < cap) ms_out[n] = ms;
            ++n;
        }
        c->timing_free.push_back(ev);
    }
    c->timing_events[stage].clear();
    if (err != hipSuccess) return fail(SVO_ERR_HIP, std::string("svo_stage_times: ") + hipGetErrorString(err));
    if (launches) *launches = n;
    return SVO_OK;
}

int svo_get_info(svo_ctx *ctx, size_t *n_nodes, int *max_depth, int *device) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    if (n_nodes) *n_nodes = c->n_nodes;
    if (max_depth) *max_depth = c->depth;
    if (device) *device = c->device;
    return SVO_OK;
}

int svo_accumulate(svo_ctx *ctx, void *d_accum, const void *d_sample, size_t n_px, uint32_t sample,
                   void *stream) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (n_px == 0) return SVO_OK;
    if (!d_accum || !d_sample) return fail(SVO_ERR_ARG, "null accumulation or sample buffer");
    if (((uintptr_t)d_accum | (uintptr_t)d_sample) & 15u) return fail(SVO_ERR_ARG, "buffers must be 16-byte aligned");
    svo_ctx *c = is_multi(ctx) ? ctx->members[0] : ctx;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // caller buffers only: the caller orders them against its renders (no context state)
    hipError_t e = svo::launch_accumulate(reinterpret_cast<float4 *>(d_accum), reinterpret_cast<const float4 *>(d_sample),
                                          n_px, sample, c->num_cus, s);
    if (e != hipSuccess) return fail(SVO_ERR_HIP, std::string("accumulate launch: ") + hipGetErrorString(e));
    return SVO_OK;
}

int svo_forget_stream(svo_ctx *ctx, void *stream) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (!stream) return SVO_OK;   // the context's own stream lives as long as the context
    for (svo_ctx *m : ctx->members) {
        int rc = svo_forget_stream(m, stream);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool known = (ctx->scratch_valid && ctx->scratch_stream == s) || (ctx->q_valid && ctx->q_stream == s);
    for (Sched &q : ctx->sched) known = known || (q.used && q.stream == s);
    if (!known) return SVO_OK;
    HIP_TRY(hipStreamSynchronize(s));
    if (ctx->q_valid && ctx->q_stream == s) {   // the query scratch: nothing of s is pending on it now
        ctx->q_valid = false;
        ctx->q_stream = nullptr;
    }
    for (Sched &q : ctx->sched) {
        if (!q.used || q.stream != s) continue;
        // the set's buffers stay allocated for the next stream; only the stream is forgotten
        if (q.side) HIP_TRY(hipStreamSynchronize(q.side));
        q.used = false;
        q.stream = nullptr;
        reset_builds(q);
        q.launches = q.shadow_launches = 0;
        q.view_prev = ~0ull;
        q.built_cost = ~0ull;
        q.last_build = 0;
        for (int r = 0; r < Sched::STATS_RING; ++r) q.stats_pending[r] = false;
        q.lat_key = Geo();
        q.lat_mode = -1;
    }
    if (ctx->scratch_valid && ctx->scratch_stream == s) {
        ctx->scratch_valid = false;
        ctx->scratch_stream = nullptr;
    }
    return SVO_OK;
}

int svo_synchronize(svo_ctx *ctx) {
    if (!ctx) return fail(SVO_ERR_ARG, "null context");
    if (is_multi(ctx)) {
        for (svo_ctx *m : ctx->members) {
            int rc = svo_synchronize(m);
            if (rc) return rc;
        }
        return SVO_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());   // the context's stream and every caller stream it rendered on
    // nothing is pending on any stream now, and a caller may destroy its streams (svo_rt.h): the
    // context records no event on a stream it saw before this point (an eviction of its
    // dispatch-order set skips the hand-over event; the host-path scratch needs no ordering)
    for (Sched &q : ctx->sched) q.idle = true;
    ctx->scratch_valid = false;
    ctx->scratch_stream = nullptr;
    ctx->q_valid = false;
    ctx->q_stream = nullptr;
    return SVO_OK;
}

int svo_destroy(svo_ctx *ctx) {
    if (!ctx) return SVO_OK;
    if (!is_multi(ctx) && ctx->peers.empty()) return destroy_single(ctx);
    for (svo_ctx *m : ctx->members) {   // drain every device first: payloads and events are shared
        hipSetDevice(m->device);
        hipDeviceSynchronize();
    }
    for (size_t i = 1; i < ctx->peers.size(); ++i) {
        Peer &pr = ctx->peers[i];
        if (i < ctx->members.size()) hipSetDevice(ctx->members[i]->device);
        for (int j = 0; j < 2; ++j) {
            if (pr.buf[j]) hipFree(pr.buf[j]);
            if (pr.rendered[j]) hipEventDestroy(pr.rendered[j]);
        }
        if (pr.dense) hipFree(pr.dense);
        if (pr.accum) hipFree(pr.accum);
    }
    if (!ctx->members.empty()) hipSetDevice(ctx->members[0]->device);
    for (size_t i = 1; i < ctx->peers.size(); ++i)
        for (int j = 0; j < 2; ++j)
            if (ctx->peers[i].local[j]) hipFree(ctx->peers[i].local[j]);
    for (int j = 0; j < 2; ++j)
        if (ctx->gathered[j]) hipEventDestroy(ctx->gathered[j]);
    for (svo_ctx *m : ctx->members) destroy_single(m);
    delete ctx;
    return SVO_OK;
}

}  // extern "C"
