/*
 * svo_rt.h -- C-ABI of the MI355X sparse-voxel-octree ray caster (libsvo_rt.so).
 *
 * Drop-in native plugin for the reference's GPU host driver
 * `RaytracingMaster` (Assets/Scripts/SVO/GPU/RaytracingMaster.cs) and the
 * compute kernel it dispatches (Assets/Shaders/RaytraceCompute.compute +
 * NVIDIASVO.compute + AttachmentLookup.compute).  Plain C types only: no
 * torch / HIP types cross this boundary (streams are passed as void*).
 *
 * Conventions:
 *  - every function returns SVO_OK (0) or a negative svo_status; the
 *    thread-local svo_last_error() gives the text.  No C++ exception crosses.
 *  - host arrays are owned by the caller and copied before the call returns
 *    (ComputeBuffer.SetData semantics); device memory is owned by the context.
 *  - one context is driven from one host thread at a time; its asynchronous
 *    entry points take any hipStream_t, and renders on different streams run
 *    concurrently (per-stream dispatch-order state).
 *  - a caller stream handed to a context may be destroyed after
 *    svo_forget_stream(ctx, stream), svo_synchronize(ctx) or svo_destroy(ctx):
 *    until one of them, the context may record an event on it (when a fifth
 *    stream takes its dispatch-order state over, or another stream takes the
 *    host-path scratch or the ordered ray query's scratch).  After svo_synchronize no work is pending anywhere, so
 *    the context records nothing on a stream it saw before that call.
 *  - policy (dispatch order, loop form, segmented rays, beam starts, shadow and
 *    readback forms) is one svo_config per context, svo_set_config; no
 *    environment variable changes what the library computes or how (four
 *    diagnostic switches only add traces and timing aids: INTEGRATION.md).
 */
#ifndef SVO_RT_H
#define SVO_RT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svo_ctx svo_ctx;

typedef enum svo_status {
    SVO_OK = 0,
    SVO_ERR_ARG = -1,        /* null / out-of-range argument */
    SVO_ERR_CAPACITY = -2,   /* upload exceeds the node-pool capacity */
    SVO_ERR_FORMAT = -3,     /* malformed node pool (pointer out of range, too deep) */
    SVO_ERR_HIP = -4,        /* HIP runtime failure */
    SVO_ERR_STATE = -5       /* call out of order (e.g. render before upload) */
} svo_status;

/* Stack modes: HLSL reproduces the float2 round trip
 * of NVIDIASVO.compute:98; EXACT keeps exact (parent, t_max) entries.  The round
 * trip keeps 24 bits of each entry: a parent index above 2^24 is rounded, and a
 * popped t_max (asint ~ 2^30) is off by up to 2^-17 relative, which hides a voxel
 * whose crossing is shorter than 2^-17 t (t in SVO units from the ray's origin):
 * voxels of a pool 16 or more levels deep are lost when seen from outside the
 * cube (1 of 1,000 aimed rays at depth 16, 8 % at depth 19, 20 % at depth 21;
 * none from origins next to the geometry).  Hosts take EXACT when the node count
 * exceeds 2^24 or the pool's depth is 16 or more (INTEGRATION.md "Stack mode",
 * tests/test_geometry_model.py). */
typedef enum svo_stack_mode { SVO_STACK_HLSL = 0, SVO_STACK_EXACT = 1 } svo_stack_mode;

/* Per-pixel hit record, 24 bytes. */
typedef struct svo_hit {
    uint32_t parent;     /* descriptor holding the hit leaf (NVIDIASVO.compute:177); 0xFFFFFFFF = miss */
    uint8_t  hit_idx;    /* child slot of the hit leaf = idx ^ octant_mask ^ 7 (:176) */
    uint8_t  hit_scale;  /* leaf scale, 23 - depth */
    uint16_t flags;      /* bit0 hit, bit1 iteration cap, bit2 stack overflow, bit3 in shadow,
                            bit4 invalid ray (svo_trace_rays only) */
    float    t;          /* bestHit.distance = 2048 * t_min (:163,171); +inf on miss */
    float    nx, ny, nz; /* normalize(decodeNormal(att[2*parent+1] >> 16)) (:177-182) */
} svo_hit;

/* Compact per-pixel record, 12 bytes = the first 12 bytes of svo_hit: what moves
 * between devices when a frame is split.  The display device rebuilds the normal
 * and the Result colour from it with its own SVO replica and camera (the normal
 * is a function of `parent` alone, NVIDIASVO.compute:177-182). */
typedef struct svo_hit_compact {
    uint32_t parent;
    uint32_t meta;       /* hit_idx | hit_scale << 8 | flags << 16 (svo_hit bytes 4..7) */
    float    t;
} svo_hit_compact;

/* Row split of one frame across ranks/GPUs: rows are grouped in bands of
 * `band_rows`; round-robin (cycle 0) band b belongs to rank b % band_count;
 * a weighted deal (0 < cycle <= 256) gives band b to rank owner[b % cycle]
 * (owner: `cycle` entries, each < band_count), e.g. fewer bands to the display
 * rank, which also assembles the frame.  A rank's output holds only its own rows,
 * in increasing y.  {1, 0, 1} (or NULL) = whole frame.  band_rows is any positive
 * number, not only a multiple of the 8-row tile (the kernels' tiles are cut from the
 * rank's own rows in order, so one tile may hold rows of several bands), and a rank may
 * own no rows at all (a band taller than the frame): its render is a no-op that returns
 * SVO_OK and its part may be empty (0 bytes; a sparse part: the 4-byte count, 0). */
typedef struct svo_band {
    int band_rows;
    int band_rank;
    int band_count;
    int cycle;                /* 0: round-robin */
    const uint8_t *owner;     /* cycle > 0: owner[b % cycle] = rank of band b */
} svo_band;

/* Every per-pixel output of one render (device pointers on the context's
 * device, each nullable).  layout SVO_LAYOUT_BAND: buffers hold only the rows of
 * the render's band, in increasing y (the whole frame without a band);
 * SVO_LAYOUT_FRAME: full-frame buffers, this band's rows written in place. */
enum { SVO_LAYOUT_BAND = 0, SVO_LAYOUT_FRAME = 1 };
typedef struct svo_frame {
    svo_hit *hits;             /* 24-byte hit records */
    float *rgba;               /* RGBA32F Result (RaytraceCompute.compute:167) */
    uint32_t *rgba8;           /* display RGBA8: R | G << 8 | B << 16 | 255 << 24, each
                                  channel (uint)(saturate(c) * 255 + 0.5) */
    svo_hit_compact *compact;  /* 12-byte records */
    float *position;           /* float4 per pixel: bestHit.position (NVIDIASVO.compute:165-174),
                                  w = 0; misses 0 (CreateRayHit, RaytraceCompute.compute:33-41) */
    uint64_t *voxel;           /* voxel key x | y << 21 | z << 42 of the hit leaf (integer voxel
                                  coordinates at the leaf scale, un-mirrored; unique for depth <= 21);
                                  misses all ones */
    uint8_t *rgb8;             /* display RGB, 3 bytes per pixel (R, G, B): the RGBA8 word without
                                  its constant alpha -- the dense band payload of a split frame */
    uint64_t *hitmask;         /* one word per 8x8 tile of the render's rows (band-local tiles, row-major,
                                  ceil(W/8) per tile row): bit (y%8)*8 + x%8 set = that pixel hit a
                                  voxel (the wave's ballot) -- the head of a sparse band payload */
    int layout;
} svo_frame;

/* Render policy of a context (ABI 10) -- the plugin's counterpart of RaytracingMaster's
 * Inspector fields (RaytracingMaster.cs:16-18): every switch that chooses HOW a frame is
 * traced.  None changes a result: every combination renders bit-identical frames (the GPU
 * suite runs the oracle comparison under each); they move only time.  Versioned by size: a
 * caller sets `size` = sizeof(svo_config) as it was compiled, svo_set_config reads the fields
 * that fit in it and keeps the context's values of any later ones, svo_get_config writes at
 * most `size` bytes.  svo_get_config(NULL, cfg) gives the defaults below.  Hex tables: one
 * nibble per cost class (lowest = heaviest: >= 7/8, 3/4, 1/2, 1/4, 1/8 of the heaviest tile,
 * rest), each 0 (whole tiles), 4 or 8 (t-segments per ray). */
#define SVO_CONFIG_VERSION 2
typedef struct svo_config {
    uint32_t size;               /* sizeof(svo_config) as compiled by the caller */
    uint32_t version;            /* SVO_CONFIG_VERSION (written by svo_get_config) */
    /* dispatch order */
    int32_t  tile_order;         /* 1: heaviest cost class first, from earlier launches' tile costs; 0: strip order */
    int32_t  xcd_strips;         /* 1: tile columns dealt to the 8 XCDs in interleaved strips; 0: raster */
    int32_t  issue_priority;     /* 1: s_setprio 3/2/1 by cost class */
    int32_t  order_every;        /* >= 1: rebuild the order every k-th launch while costs drift (32) */
    int32_t  move_every;         /* >= 1: while the camera moves, rebuild every k-th launch (4) */
    int32_t  move_spread;        /* 1: a moving camera's order classes a tile by its 3x3 neighbourhood (1) */
    int32_t  relayout;           /* 1: rebuild once in a new class table's own layout (1) */
    int32_t  fetch_all;          /* -1: by pool size (< 2^24 nodes: 1); 0: fetch on a changed node; 1: every trip */
    /* loop form */
    int32_t  loop_form;          /* -1: by the last order build's statistics; 0: lean; 1: latency form */
    float    lat_ratio;          /* latency-bound when summed trips < ratio x resident waves x heaviest (0.3) */
    /* segmented rays */
    int32_t  segments;           /* 1: heavy tiles traced as t-segments by the class tables; 0: never */
    uint32_t seg_table_latency;  /* class table of a latency-bound launch (0x444) */
    uint32_t seg_table_issue;    /* ... of an issue-bound launch (0x4) */
    uint32_t seg_table_thin;     /* ... of a latency-bound launch below seg_thin_ratio (0x888) */
    float    seg_ratio;          /* the latency-bound boundary with beam starts (0.28) */
    float    seg_thin_ratio;     /* the thin boundary (0.083) */
    int32_t  seg_cap;            /* >= 1: segmented tiles per XCD at most (96) */
    int32_t  seg_min_chain;      /* a latency-bound launch whose heaviest tile has fewer trips: no segments (160) */
    int32_t  seg_move;           /* starts after a camera move: 1 the stored ones, 2 even split (2) */
    int32_t  seg_jitter;         /* ... in a jittered launch: 0 no segments, 1 stored, 2 even split (2) */
    int32_t  seg_all;            /* tests: 0 off, 4 or 8 = every tile segmented with that K */
    uint32_t seg_scramble;       /* tests: != 0 replaces every start by a hash (unordered, NaN, +-inf) */
    /* beam starts */
    int32_t  beam;               /* 1: primary rays start at their tile's splatted lower bound of the hit t */
    int32_t  beam_back;          /* >= 0: splat the boxes this many levels above the leaves (2) */
    /* shadow rays (SVO_OPT_SHADOW_RAYS) */
    int32_t  shadow_form;        /* 0: fused into the primary launch; 1: second pass over tiles; 2: over the
                                    compacted hit list */
    int32_t  shadow_order;       /* 1: the two-pass form's tiles in their own cost order */
    /* host paths */
    int32_t  readback;           /* svo_render_progressive_async copy: 0 one DMA, 1 kernel push, 2 two DMAs */
    int32_t  host_copy_threads;  /* svo_render's host copy threads (0: half the hardware threads, <= 16) */
    /* multi-device contexts (svo_create_multi) */
    int32_t  sparse_payload;     /* 1: display-only frames travel as sparse hit payloads */
    int32_t  peer_copy;          /* 1: every member's payload copied instead of pulled over xGMI (tests) */
    /* version 2 */
    int32_t  beam_back_held;     /* a held view (the second launch at a view on a stream and later) re-splats
                                    once with boxes this many levels above the leaves (0); -1: beam_back */
} svo_config;
int svo_get_config(svo_ctx *ctx, svo_config *cfg);
int svo_set_config(svo_ctx *ctx, const svo_config *cfg);

/* ~ RaytracingMaster.InitializeSVOBuffer (RaytracingMaster.cs:111-116):
 * allocate a node pool of `capacity_nodes` descriptors (+2 attachment words
 * each) on HIP device `device`. */
int svo_create(int device, size_t capacity_nodes, svo_ctx **out);

/* Multi-device context (north star: the image sharded into screen bands over
 * the GPUs of one node, the SVO replicated per GPU, the bands gathered to the
 * display GPU over xGMI).  devices[0] is the display device; the same index may
 * repeat (one GPU then renders several members' bands: the test form).  Every
 * other entry point accepts the result: uploads and camera go to every device;
 * svo_render / svo_render_device / svo_render_frame render the whole frame in
 * `band_rows`-row bands dealt round-robin over the devices and leave it on
 * devices[0] (outputs are devices[0] pointers, frame layout).  The reference
 * dispatches one grid over the whole frame (RaytracingMaster.cs:66-68).
 * Payload transport per member (svo_get_member_link): the display device pulls a
 * member's payload over xGMI when hipDeviceCanAccessPeer allows it; when it does
 * not (or svo_config.peer_copy forces it), the member's stream copies the payload
 * into a buffer on the display device (hipMemcpyPeerAsync) and the assemble
 * reads that copy -- creation no longer fails for lack of peer access.
 * band_rows need not be a multiple of the 8-row tile, and a member may own no rows
 * of a frame (its render is a no-op and its payload is empty). */
int svo_create_multi(const int *devices, int num_devices, size_t capacity_nodes, int band_rows, svo_ctx **out);
int svo_num_devices(svo_ctx *ctx, int *num_devices);
/* How member `index`'s band payload reaches the display device: SVO_LINK_SELF
 * (the display device itself, or the same device index), SVO_LINK_PEER (pulled
 * over xGMI with peer access), SVO_LINK_COPY (copied by hipMemcpyPeerAsync).
 * *device = the member's HIP device.  Single-device contexts: index 0, SELF. */
enum { SVO_LINK_SELF = 0, SVO_LINK_PEER = 1, SVO_LINK_COPY = 2 };
int svo_get_member_link(svo_ctx *ctx, int index, int *device, int *link);
/* Weighted band deal for a multi-device context (svo_band.cycle / owner): band b
 * goes to member owner[b % cycle]; e.g. fewer bands for devices[0], which also
 * assembles the frame.  cycle 0 = round-robin (the default). */
int svo_set_band_deal(svo_ctx *ctx, int cycle, const uint8_t *owner);
/* The per-device context `index` of a multi-device context (the context itself
 * for index 0 of a single-device one): owned by the group, not destroyed alone. */
int svo_get_member(svo_ctx *ctx, int index, svo_ctx **member);

/* ~ RaytracingMaster.SetSVOBuffer(RT.SVOData data, int offset)
 * (RaytracingMaster.cs:118-135, CompactSVO.cs:22-35): upload `n_desc` reference
 * descriptors (int32: ptr16 << 16 | valid8 << 8 | nonleaf8, ptr RELATIVE to the
 * descriptor) and `n_att` attachment words at descriptor offset `dst_offset`.
 * Deviation (documented): attachments land at word 2*dst_offset; the
 * reference writes them at word `offset` (RaytracingMaster.cs:134). */
int svo_set_buffer(svo_ctx *ctx, const int32_t *desc, size_t n_desc,
                   const uint32_t *att, size_t n_att, size_t dst_offset);

/* Wide node format for pools whose child pointers exceed 16 bits:
 * node = (uint64)first_nonleaf_child_abs << 32 | valid8 << 8 | nonleaf8. */
int svo_set_buffer_v2(svo_ctx *ctx, const uint64_t *nodes, size_t n_nodes,
                      const uint32_t *att, size_t n_att, size_t dst_offset);

/* ~ RaytracingMaster.UpdateShaderParameters (RaytracingMaster.cs:32-41):
 * Unity Matrix4x4 (column-major) camera-to-world and inverse projection,
 * _PixelOffset and _DirectionalLight (forward.xyz, intensity). */
int svo_set_camera(svo_ctx *ctx, const float c2w[16], const float inv_proj[16],
                   float px_off_x, float px_off_y, const float light[4]);

/* ~ RaytracingMaster.Render / Dispatch (RaytracingMaster.cs:60-74): trace one
 * primary ray per pixel of a width x height frame.  rgba_out (W*H*4 floats,
 * = the Result RWTexture2D<float4>) and hits_out (W*H records) are HOST
 * buffers, either may be NULL.  Blocks until the results are on the host. */
int svo_render(svo_ctx *ctx, int width, int height, int stack_mode,
               float *rgba_out, svo_hit *hits_out);

/* Device-resident variant for hosts that keep the frame in HBM: d_rgba /
 * d_hits are device pointers on this context's device (either may be NULL),
 * `band` selects this rank's rows (NULL = all), `stream` is a hipStream_t
 * (NULL = the context's own stream).  Asynchronous: returns after enqueue --
 * with one exception: the automatic loop-form choice (svo_config.loop_form -1,
 * the default) waits, once per new static view (the second render after a camera move),
 * for the dispatch-order build of the first one, i.e. for up to one frame of
 * already-enqueued work on that stream.  A caller whose stream waits on something
 * the host signals only after this call returns must set loop_form 0 or 1.  The same
 * holds for svo_render_frame and the renders of svo_render. */
int svo_render_device(svo_ctx *ctx, int width, int height, int stack_mode,
                      const svo_band *band, void *d_rgba, void *d_hits, void *stream);

/* General render: every output of svo_frame, for the rows of `band` (NULL = the
 * whole frame; a multi-device context requires NULL).  Asynchronous. */
int svo_render_frame(svo_ctx *ctx, int width, int height, int stack_mode, const svo_band *band,
                     const svo_frame *frame, void *stream);

/* Samples in flight -- the reference's progressive frame loop (_PixelOffset = (Random.value,
 * Random.value) per frame, RaytracingMaster.cs:35; the AddShader blend with _Sample =
 * _currentSample, then _currentSample++, :70-73, AddShader.shader:44-47), several frames'
 * samples in ONE launch: trace n_samples (1..8) jittered samples of the frame (or of `band`'s
 * rows) -- sample k with _PixelOffset (px_offsets[2k], px_offsets[2k + 1]), the context's
 * camera otherwise -- and blend them in order into d_accum (RGBA32F, band or frame layout as
 * `layout`), sample k with _Sample = first_sample + k.  The blend is svo_accumulate's
 * arithmetic: d_accum ends bit-identical to n_samples single-sample renders each followed by
 * svo_accumulate.  d_rgba8 / d_rgb8 (nullable): the blended pixels' display RGBA8 words /
 * 3-byte RGB (a split frame's band payload).  Primary rays only.  Asynchronous.  One launch
 * holds n_samples waves per 8x8 tile, so a small band's heaviest wave no longer drains alone
 * (DESIGN.md 6.1).  A multi-device context (band NULL, frame layout) splits the frame over
 * its devices: each member blends its own rows into a band accumulation it keeps on its own
 * device (zeroed when the frame size changes), the display device into d_accum's rows of its
 * bands; the members' blended rows travel as 3-byte RGB and d_rgba8 (required; d_rgb8 must be
 * NULL) receives the whole frame's display words. */
int svo_render_samples(svo_ctx *ctx, int width, int height, int stack_mode, const svo_band *band, int n_samples,
                       const float *px_offsets, uint32_t first_sample, float *d_accum, uint32_t *d_rgba8,
                       uint8_t *d_rgb8, int layout, void *stream);

/* Rebuild a split frame on this context's device from its band parts: part m
 * holds the rows of rank m of the deal `deal` (band_count == n_parts; band_rank
 * ignored; round-robin: bands b with b % n_parts == m), band layout, as
 * svo_hit_compact records (SVO_PART_COMPACT: frame
 * outputs hits / rgba / rgba8 / compact, the normal and colour rebuilt from this
 * context's SVO replica and camera), RGBA8 words (SVO_PART_RGBA8) or 3-byte RGB
 * (SVO_PART_RGB8; rows of 3 * width bytes) or sparse hit RGB (SVO_PART_SPARSE_RGB8:
 * svo_pack_hits' layout, read as is -- no scan here; miss pixels get the sky computed
 * here) -- the last three
 * rebuild the frame output rgba8 only.  Part pointers must be readable from this device (its own memory,
 * or a peer's with peer access).  skip_part (or -1): a part already rendered in
 * place.  `frame` must use the frame layout.  This is the display-side half of
 * the one-process-per-GPU split (parts received over RCCL); multi-device
 * contexts use it internally.  Asynchronous. */
enum { SVO_PART_COMPACT = 0, SVO_PART_RGBA8 = 1, SVO_PART_RGB8 = 2, SVO_PART_SPARSE_RGB8 = 3 };
int svo_assemble_frame(svo_ctx *ctx, int width, int height, const svo_band *deal, int n_parts,
                       const void *const *parts, int part_format, int skip_part, const svo_frame *frame,
                       void *stream);

/* Sparse band payload (wave ballot + prefix sum).  Part layout, n_tiles = ceil(W/8) *
 * ceil(rows/8) of the band:
 *   bytes [0, 8 n)             uint64 hit mask per tile (svo_frame.hitmask, written by the render)
 *   bytes [8 n, 12 n + 4)      uint32 hits before each tile, then the band's hit count
 *   bytes [12 n + 4, + 3 count) the 3-byte RGB of every hit pixel, tile by tile in lane order
 * `d_part` holds the masks on entry; this writes the offsets (an exclusive scan of the
 * masks' popcounts) and packs the hits' RGB from `d_rgb8` (the band's dense
 * svo_frame.rgb8).  Allocate SVO_SPARSE_PART_BYTES(n_tiles, band pixels) (its tail
 * beyond the RGB is the scan's scratch, never sent); the part to send is
 * SVO_SPARSE_HEAD_BYTES(n_tiles) + 3 * count bytes, count = the uint32 at byte 12 n.
 * Misses cost nothing -- the display device computes their sky.  Asynchronous. */
#define SVO_SPARSE_HEAD_BYTES(n_tiles) (12u * (size_t)(n_tiles) + 4u)
#define SVO_SPARSE_PART_BYTES(n_tiles, n_px)                                                          \
    (((SVO_SPARSE_HEAD_BYTES(n_tiles) + 3u * (size_t)(n_px) + 3u) & ~(size_t)3) + 4u * (size_t)(n_tiles) + \
     4u * (((size_t)(n_tiles) + 1023u) / 1024u))
int svo_pack_hits(svo_ctx *ctx, int width, int height, const svo_band *band, const void *d_rgb8, void *d_part,
                  void *stream);

/* Instrumented trace: per-ray descriptor-fetch counts (device uint32 array,
 * NVIDIASVO.compute:60-62 executions), used for the algorithmic-bytes figure
 * of the roofline.  Same arguments as svo_render_device plus d_fetches.
 * By default the reference's own walk from the cube entry; with the option
 * SVO_OPT_COUNT_BEAM the walk the render actually runs, from the beam start
 * (DESIGN.md 3.1d). */
int svo_count_fetches(svo_ctx *ctx, int width, int height, int stack_mode,
                      const svo_band *band, void *d_fetches, void *stream);

/* Diagnostics (ABI 10): the start of every primary ray's walk under the current camera -- the
 * beam start of DESIGN.md 3.1d, in SVO-space t (the loop's t_min; the hit record's t is 2048 x
 * that), one float per pixel of `band`'s rows (band layout), -inf where the ray starts at its cube
 * entry.  A record is exact iff no hit lies before its start, so start <= the oracle's hit t on
 * every hit ray is the bound's conservativeness (tests/test_gpu_beam.py).  Asynchronous. */
int svo_beam_starts(svo_ctx *ctx, int width, int height, const svo_band *band, float *d_starts, void *stream);

/* Render options (bit set).  SVO_OPT_SHADOW_RAYS: after the primary pass,
 * trace one shadow ray per hit toward -_DirectionalLight (SURVEY.md 8(d) C3;
 * the reference's shadow test is commented out at RaytraceCompute.compute:105-112):
 * origin = world hit point + 0.001 * normal; an occluded pixel gets hit flag
 * bit 3 and a black Result. */
enum { SVO_OPT_SHADOW_RAYS = 1, SVO_OPT_KERNEL_TIMING = 2, SVO_OPT_COUNT_BEAM = 4 };
enum { SVO_OPT_SCENE_SHADOWS = 8 };   /* svo_set_options: shadow and light passes know the objects (below) */
int svo_set_options(svo_ctx *ctx, uint32_t options);

/* SVO_OPT_KERNEL_TIMING: every render launch brackets its primary-ray kernel
 * (only that kernel: not the shadow pass, not the dispatch-order kernel) with
 * HIP events on the launch stream.  svo_kernel_time waits for the recorded
 * launches and returns their mean kernel duration in ms and their number, then
 * forgets them.  Measurement only (bench.py's roofline); no reference
 * counterpart. */
int svo_kernel_time(svo_ctx *ctx, double *mean_ms, uint64_t *launches);
/* The same for a stage: SVO_STAGE_KERNEL (= svo_kernel_time) or SVO_STAGE_ASSEMBLE
 * (the assemble kernel of svo_assemble_frame / a multi-device frame).  On a
 * multi-device context every member's recorded launches of the stage are drained
 * and the slowest member's mean is returned (launches: that member's count);
 * svo_get_member gives one device's own figure. */
enum { SVO_STAGE_KERNEL = 0, SVO_STAGE_ASSEMBLE = 1 };
int svo_stage_time(svo_ctx *ctx, int stage, double *mean_ms, uint64_t *launches);
/* Every recorded launch's duration of a stage, in launch order (the first `cap`
 * into ms_out; *launches = how many were recorded), then forgets them like
 * svo_stage_time.  A multi-device context returns devices[0]'s launches and drops
 * the other members' records.  For hosts that watch frame-to-frame variation
 * (a moving camera renders every frame at a new view). */
int svo_stage_times(svo_ctx *ctx, int stage, float *ms_out, size_t cap, size_t *launches);

/* ~ Graphics.Blit(Result, destination, AddMaterial) with _Sample = `sample`
 * (RaytracingMaster.cs:70-73, AddShader.shader:10,44-47): progressive
 * accumulation dst = src * a + dst * (1 - a), a = 1 / (sample + 1), on all four
 * channels (source alpha = a).  d_accum and d_sample are device buffers of
 * n_px RGBA32F pixels (16-byte aligned) on the context's device; `stream` as in
 * svo_render_device.  The caller keeps `sample` (_currentSample): 0 after a
 * camera change (RaytracingMaster.cs:44-47), +1 per frame. */
int svo_accumulate(svo_ctx *ctx, void *d_accum, const void *d_sample, size_t n_px, uint32_t sample,
                   void *stream);

/* ~ RaytracingMaster.OnRenderImage end to end (RaytracingMaster.cs:55-74 with
 * AddShader.shader:44-47): render one sample of the frame at the current camera,
 * blend it into the context's device-resident accumulation frame with
 * _Sample = `sample` (svo_accumulate's blend; the frame is reallocated whenever
 * its size changes, and the first sample after that is blended as sample 0 --
 * it replaces the frame -- whatever `sample` says), and copy the accumulated frame to the host as display RGBA8
 * words (4 B/px, R in the low byte = Unity TextureFormat.RGBA32; each colour
 * channel (uint)(saturate(c) * 255 + 0.5), alpha 255) and/or RGBA32F (16 B/px); either output may be
 * NULL, not both.  Only the accumulated frame crosses PCIe: 8.3 MB per 1080p
 * frame as RGBA8 against 83 MB for svo_render's RGBA32F + hit records.  A
 * multi-device context renders the sample split over its devices and
 * accumulates on devices[0].  Blocking. */
int svo_render_progressive(svo_ctx *ctx, int width, int height, int stack_mode, uint32_t sample,
                           uint32_t *rgba8_out, float *rgba_out);

/* svo_render_progressive for a host that displays every frame (Unity:
 * Texture2D.LoadRawTextureData(IntPtr, int) on the returned pointer, then Apply):
 * enqueue one sample -- render, blend with _Sample = `sample`, pack the accumulated
 * frame to display pixels -- and their copy into plugin-owned pinned host memory on a
 * copy stream, then return in *frame_out the PREVIOUS call's frame (NULL on the first
 * call after creation, a size change or a pixel-format change), waiting only for that
 * frame's copy.  So the D2H of frame k overlaps the render of frame k + 1, and the host
 * never waits for the frame it just asked for.  pixel_format: SVO_PIXELS_RGBA8 (4 B/px,
 * the words of svo_render_progressive's rgba8_out = TextureFormat.RGBA32) or
 * SVO_PIXELS_RGB8 (3 B/px, the same words without their constant alpha =
 * TextureFormat.RGB24: a quarter fewer bytes over PCIe).  A returned pointer (W * H
 * pixels) stays valid until the call after next; the plugin owns it.
 * svo_progressive_last returns the most recent frame, waiting for its copy (the end of a
 * sequence).  The blocking svo_render_progressive stays available. */
enum { SVO_PIXELS_RGBA8 = 0, SVO_PIXELS_RGB8 = 1 };
int svo_render_progressive_async(svo_ctx *ctx, int width, int height, int stack_mode, uint32_t sample,
                                 int pixel_format, const void **frame_out);
int svo_progressive_last(svo_ctx *ctx, const void **frame_out);

/* Ray queries: trace a caller-supplied batch of world-space rays through the uploaded pool --
 * picking, line of sight, secondary rays.  The reference has this on its CPU side only
 * (the SVO interface's Trace(UnityEngine.Ray), Assets/Scripts/SVO/RTUtility/Interfaces.cs:6-15,
 * driven by SVODriver.UpdateRaycast, SVODriver.cs:74-87).  No camera is involved and a query
 * reads the node pool only: it leaves every piece of render state alone (dispatch orders, tile
 * costs, beam starts, view-change detection, kernel-timing records, the progressive frame), so
 * a render before and after a query gives the same bytes and takes the same path.
 *
 * Each ray is processed in this order:
 *  1. classify: a ray is INVALID if any origin or direction component is non-finite, if t_max
 *     is NaN, or if all three direction components are zero.  An invalid ray is not traced: it
 *     gets the miss record (parent 0xFFFFFFFF, t +inf, normal 0) with flag bit 4
 *     (SVO_HIT_INVALID_RAY), position 0, voxel key all ones, hit-mask bit 0.
 *  2. clamp: unless SVO_QUERY_RAW_DIRECTIONS is set, every direction component with
 *     |d| < 2^-23 becomes copysign(2^-23, d) (-0 gives -2^-23).  Deviation (documented): this
 *     is Laine-Karras's small-direction clamp, which the reference commented out
 *     (NVIDIASVO.compute:21-24, epsilon exp2(-s_max) at :3); without it an exactly axis-aligned
 *     ray misses everything.  The position output uses the clamped direction.
 *  3. trace: the walk of IntersectSVO (NVIDIASVO.compute:12-198) on that origin and direction,
 *     in the context's pool and the given stack mode -- the primary rays' own loop; hit record,
 *     position and voxel key are bit-identical to the CPU oracle's for the same ray.
 * Units: `t` of the record keeps its meaning everywhere else in this header, 2048 x the
 * SVO-space t_min; the world-space hit point is origin + (t / 64) * dir, and with a unit
 * direction t / 64 is the world distance.  The direction is used as given, NOT normalised.
 * t_max is a filter on the finished record, not an early exit: the ray stays a hit iff
 * t * (1 / 64) <= t_max in f32; otherwise every output gets the plain miss record (flags 0).
 * +inf: no limit.
 * Outputs: every non-NULL output is fully written for all n_rays (the caller zeroes nothing),
 * nothing is written past n_rays entries or past ceil(n_rays / 64) mask words, and the unused
 * bits of the last mask word are 0.
 * SVO_QUERY_ORDERED: the rays are traced in the order of a 30-bit key (3 bits octant mask, 27
 * bits Morton code of the ray's entry point into the cube; invalid rays and rays that miss the
 * cube last), sorted on the device, and every output is scattered to the ray's own index --
 * placement only, the results are byte-identical to the unordered query.  Keys, indices and
 * the sort's temporary storage are context-owned and grow-only.
 * n_rays == 0: SVO_OK, nothing launched.  n_rays above 2^31 - 1, a NULL context, d_rays or out,
 * an out with every pointer NULL, unknown flag bits or a bad stack mode: SVO_ERR_ARG (checked
 * before any device is touched); no pool uploaded: SVO_ERR_STATE.  A multi-device context
 * runs the query on devices[0].  d_rays and the outputs are device pointers on that device,
 * d_rays 16-byte aligned.  Asynchronous on `stream` (NULL: the context's own). */
typedef struct svo_ray {      /* 32 bytes, 16-byte aligned in device memory */
    float origin[3];          /* world space, as CreateCameraRay's ray.origin */
    float t_max;              /* world-space parameter limit; +inf: none */
    float dir[3];             /* world space, used as given: NOT normalised */
    uint32_t reserved;        /* 0 */
} svo_ray;

typedef struct svo_query_out { /* device pointers, each nullable, not all NULL */
    svo_hit  *hits;           /* n records */
    float    *position;       /* n float4, svo_frame.position's definition */
    uint64_t *voxel;          /* n keys, svo_frame.voxel's definition */
    uint64_t *hitmask;        /* ceil(n/64) words: bit i%64 of word i/64 = ray i hit */
} svo_query_out;

enum { SVO_QUERY_ORDERED = 1, SVO_QUERY_RAW_DIRECTIONS = 2 };
enum { SVO_HIT_INVALID_RAY = 0x10 };   /* svo_hit.flags bit 4: the query's ray was invalid */

int svo_trace_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n_rays, int stack_mode,
                   uint32_t flags, const svo_query_out *out, void *stream);

/* The same for HOST arrays (rays and each output nullable except rays, not all outputs NULL):
 * staged through context-owned device buffers on the context's stream; returns when the
 * results are on the host.  Blocking. */
int svo_trace_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n_rays, int stack_mode,
                        uint32_t flags, svo_hit *hits, float *position, uint64_t *voxel);

/* Level of detail (opt-in; off by default, and with it off every byte is what it was).
 * Laine-Karras's "terminate if the voxel is small enough", which the reference keeps commented
 * out (NVIDIASVO.compute:77-79).  A ray carries two non-negative finite f32 numbers:
 *   ray_size_coef  the growth of its footprint per unit of SVO-space t,
 *   ray_size_bias  its footprint at t = 0 in SVO units (the cube's side is 1: a world length / 32).
 * In the walk of IntersectSVO a valid child is entered when t_min <= min(t_max, tc_max) (:75,
 * :90).  At that point, before the leaf test (:93), the child is tested for size:
 *   small  <=>  fl(fl(tc_max * ray_size_coef) + ray_size_bias) >= scale_exp2
 * (two IEEE roundings, no fma; tc_max the child's exit time, :69; scale_exp2 its side; an ordered
 * compare, NaN is false).  A small child ends the walk exactly as a leaf does: the record's
 * parent is the descriptor holding the voxel, hit_idx its slot, hit_scale above the leaf scale,
 * t = 2048 t_min, the normal the parent's, the colour the parent's DXT texel of that slot, flag
 * bit 0 set.  No flag marks an inner voxel (it is readable from the pool: the parent's non-leaf
 * bit of hit_idx), and position, voxel key and the compact record keep their definitions at
 * hit_scale.  Deviation from Laine-Karras (documented): they test one line earlier, before the
 * t-span test; here only children the walk would otherwise enter are tested, so a voxel the ray
 * does not cross is never reported.
 * (0, 0) is off.  (0, 2^-k) is a depth clamp: every voxel of side <= 2^-k is a leaf.  For a
 * camera, ray_size_coef = pixels * 2 * |inv_proj[1][1]| / height is the footprint of `pixels`
 * pixels at the frame's centre per unit t of a unit-length ray.
 *
 * svo_set_lod sets the pair of the PRIMARY rays of svo_render, svo_render_device,
 * svo_render_frame, svo_render_samples, svo_render_progressive(_async) and svo_count_fetches (a
 * multi-device context: of every member).  svo_beam_starts and svo_assemble_frame are not
 * affected.  It is not a svo_config field: svo_config never changes results.  Changing the pair
 * counts as a camera move for the dispatch-order state and restarts nothing else.  With LOD on:
 *   - cost-ordered dispatch, XCD strips, issue priority and fetch_all work as without it;
 *   - segmented tiles and the latency loop form are off, whatever svo_config says;
 *   - beam starts stay on, each start bounded by a floor below which no LOD hit in a voxel
 *     larger than the splat list's smallest box can lie; where that floor is
 *     not positive the launch takes no beam starts;
 *   - with SVO_OPT_SHADOW_RAYS set every render entry point returns SVO_ERR_STATE before it
 *     enqueues anything: shadow rays with LOD are not supported.
 * A negative, NaN or infinite number or a NULL context: SVO_ERR_ARG.  svo_get_lod: either
 * pointer may be NULL. */
int svo_set_lod(svo_ctx *ctx, float ray_size_coef, float ray_size_bias);   /* 0, 0 = off (default) */
int svo_get_lod(svo_ctx *ctx, float *ray_size_coef, float *ray_size_bias);

/* svo_trace_rays / svo_trace_rays_host with a LOD pair of the batch's own, applied to every ray
 * of it: classify, clamp, the t_max filter, SVO_QUERY_ORDERED and every output rule are those of
 * svo_trace_rays, and with (0, 0) the results are byte-identical to it.  The context's own pair
 * (svo_set_lod) is neither read nor changed, like all other render state.  Argument errors:
 * svo_trace_rays' and a negative, NaN or infinite number, all checked before any device is
 * touched. */
int svo_trace_rays_lod(svo_ctx *ctx, const svo_ray *d_rays, size_t n_rays, int stack_mode,
                       uint32_t flags, float ray_size_coef, float ray_size_bias,
                       const svo_query_out *out, void *stream);
int svo_trace_rays_lod_host(svo_ctx *ctx, const svo_ray *rays, size_t n_rays, int stack_mode,
                            uint32_t flags, float ray_size_coef, float ray_size_bias,
                            svo_hit *hits, float *position, uint64_t *voxel);

/* Specular reflection (opt-in; off by default, and with it off every byte is what it was).
 * The reference's CSMain runs up to 8 Trace / Shade rounds (RaytraceCompute.compute:159-166): Shade
 * moves the ray to the hit point, reflects it and multiplies its energy by `specular` (:97-104),
 * which the reference hard-codes to 0, so its loop runs once.
 *
 * The bounce rule.  Inputs: a ray as traced -- world-space origin o and direction d (a camera ray
 * as is; any other ray's direction after the query's clamp) -- and its hit: t (the record's t),
 * the record normal n, hit_scale s and the voxel key's integer coordinates c.  Every operation is
 * one IEEE f32 rounding, no fma:
 *  1. box: side = 2^(s - 18), lo_k = c_k side - 16, hi_k = lo_k + side (exact: the voxel in world space).
 *  2. entry face: face_k = d_k > 0 ? lo_k : hi_k; te_k = (face_k - o_k) (1 / d_k); g = 0, then for
 *     k = 1, 2: g = k if te_k > te_g (ordered: a NaN never wins); out = d_g > 0 ? -1 : +1.
 *  3. origin: P_k = o_k + (t (1 / 64)) d_k for k != g; origin_g = face_g + out (side 2^-6).
 *  4. direction: dn = (n_0 d_0 + n_1 d_1) + n_2 d_2; r_k = d_k - (2 dn) n_k; if r_g points into the
 *     face (out > 0 and r_g < 0, or out < 0 and r_g > 0), r_g = -r_g.  Not renormalised.
 *  5. the bounce ray is {origin, t_max +inf, r, 0}, traced as svo_trace_rays traces it with flags 0.
 * Deviation (documented): the reference's origin P + 0.001 n uses the smooth normal, which on voxels
 * very often lies on or inside the voxel just hit (INTEGRATION.md "Reflections" has the counts);
 * here the ray leaves through the cube face it entered by and, on pools of up to 12 levels, cannot
 * re-enter that voxel; from 16 levels on some rays do (INTEGRATION.md "Reflections", the table by depth).
 *
 * svo_bounce_rays: from a batch and its results to the next batch: out[i] = the bounce ray of
 * rays[i] if hits[i] has flag bit 0, else the dead ray (all 32 bytes zero except t_max = +inf: a
 * zero direction, so svo_trace_rays classifies it invalid).  flags: SVO_QUERY_RAW_DIRECTIONS only
 * (how rays[i] was traced).  Reads no pool.  Writes nothing past n entries; d_rays_out may be
 * d_rays.  NULL pointers, unknown flag bits or n > 2^31 - 1: SVO_ERR_ARG, checked before any device
 * is touched; n == 0: SVO_OK, nothing launched.  Ray lists 16-byte aligned, records and keys
 * 8-byte.  A multi-device context runs it on devices[0].  Asynchronous on `stream`; the host form
 * blocks. */
int svo_bounce_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                    const uint64_t *d_voxel, svo_ray *d_rays_out, void *stream);
int svo_bounce_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                         const uint64_t *voxel, svo_ray *rays_out);

/* Reflections in renders.  specular: three numbers in [0, 1]; max_bounces in 0..7 (the reference's
 * loop is 8 rounds: the primary ray plus 7); anything else, NaN included: SVO_ERR_ARG.  NULL, all
 * zero or max_bounces 0: off.  Not a svo_config field: svo_config never changes results.
 * Per pixel with a primary hit (misses keep their sky): res = the pixel's colour as rendered with
 * reflection off and e = (1, 1, 1); then for b = 1 .. max_bounces: e *= specular; stop if e is all
 * zero; make the bounce ray of the current ray and hit; stop if it is invalid by the query's
 * classify; trace it; col = the shaded colour of its hit (normal and DXT albedo of the new record),
 * or the sky of the traced direction on a miss (a record without flag bit 0 is a miss);
 * res += e col; stop on a miss, else the bounce ray and its hit become current.
 * Only rgba, rgba8 and rgb8 change (and through them a progressive accumulation); hits, compact,
 * position, voxel and hitmask stay the primary ray's.  The bounces are a second pass behind the
 * primary launch, which takes exactly the path it takes with reflection off.
 * Served: svo_render, svo_render_device, svo_render_frame (any band, layout and stream) and
 * svo_render_progressive(_async).  svo_count_fetches, svo_beam_starts and svo_assemble_frame are
 * unaffected.  Stated limits, each SVO_ERR_STATE before anything is enqueued: a render with
 * SVO_OPT_SHADOW_RAYS set, a render with LOD on, svo_render_samples; and svo_set_reflection with a
 * non-zero setting on a multi-device context (its compact parts rebuild colours on the display
 * device).  svo_get_reflection: either pointer may be NULL. */
int svo_set_reflection(svo_ctx *ctx, const float specular[3], int max_bounces);   /* NULL / 0 = off (default) */
int svo_get_reflection(svo_ctx *ctx, float specular[3], int *max_bounces);

/* Skybox (opt-in; none by default, and with none every byte is what it was).
 * ~ RayTracingShader.SetTexture(0, "_SkyboxTexture", SkyboxTexture) (RaytracingMaster.cs:6,28): Shade's miss
 * branch samples an equirectangular panorama at (phi, theta) = (atan2(d.x, -d.z) / -PI * 0.5, acos(d.y) / -PI)
 * (RaytraceCompute.compute:119-125).  Without a texture a miss gets the procedural gradient.
 *
 * The sky rule: direction d = (x, y, z), used as given (NOT assumed unit), to RGB.  Every operation is one
 * IEEE f32 rounding, no fma; only + - * /, sqrt, floor, compares and selects (csrc/svo_sky.h; numpy: sky.py):
 *  1. invalid: a non-finite component, or x = y = z = 0: the colour is (0, 0, 0).  Otherwise d is divided by
 *     max(|x|, |y|, |z|).
 *  2. angles: polar = atan2f32(sqrt(x x + z z), y) in [0, PI]; azim = atan2f32(x, -z).  atan2f32 is the rule's
 *     own (INTEGRATION.md "Skybox" spells it out); atan2f32(+-0, positive) = +-0, atan2f32(0, 0) = +0.  For a unit
 *     direction polar is the reference's acos(d.y): a restatement, mathematically identical, in other f32
 *     operations (no normalisation needed, well conditioned at the poles).
 *  3. theta = polar / -PI, phi = azim / -PI * 0.5f, PI = 3.14159265f; the sample point is (phi, theta).
 *  4. wrap: u = phi - floor(phi), a result of 1 becomes 0.  v: the same on theta (repeat, Unity's default
 *     wrapMode), or min(max(theta + 1, 0), 1) with SVO_SKY_CLAMP_V (row indices then clamp to [0, H - 1]).
 *  5. nearest: i = min((int)floor(u W), W - 1), j = min((int)floor(v H), H - 1).
 *  6. SVO_SKY_BILINEAR: x = u W - 0.5, i0 = floor(x), fx = x - i0, columns i0 and i0 + 1 wrapped mod W; rows
 *     likewise, wrapped mod H or clamped; c = (t00 (1 - fx) + t10 fx) (1 - fy) + (t01 (1 - fx) + t11 fx) fy
 *     per channel, in that order.
 *  7. rows: texel (i, j) is rgba[4 (j W + i)], row 0 is v = 0 -- Unity's raw texel order (GetPixels /
 *     GetPixelData: bottom row first).  The horizon is v = 0.5, "up" is towards the last row; straight up
 *     itself is theta = 0: row 0 with repeat (as in the reference), the last row with clamp.
 * (u, v) is within 1.0e-7 of the exact value (measured), 1/1200 texel at the largest size.
 *
 * svo_set_skybox: rgba is a HOST array of width x height x 4 floats (a Unity Color[]; alpha is ignored),
 * copied before the call returns; the texels live on the context's device.  NULL: back to the gradient
 * (width, height ignored).  Waits for every stream that may still read the previous texture.  Not a
 * svo_config field: svo_config never changes results.  Leaves the dispatch-order state, tile costs, beam
 * starts and view-change detection alone.  SVO_ERR_ARG, checked before any device is touched: a NULL
 * context, unknown flag bits, and with a non-NULL rgba a non-positive size, a size above 8192, or a colour
 * component (alpha excepted) that is negative or not finite.  SVO_ERR_STATE: a non-NULL rgba on a
 * multi-device context.  svo_get_skybox: 0 x 0 = none; every pointer may be NULL.
 *
 * Renders: with a texture set, every pixel whose hit-mask bit is clear (a miss, also one whose record
 * carries the iteration-cap or stack-overflow flag) gets the rule's colour of its camera ray's direction
 * (alpha 1), in rgba, rgba8 and rgb8 (and through them a progressive accumulation).  Hit pixels and every
 * other output are untouched.  It is a pass behind the primary launch, which takes exactly the path it takes
 * without a texture (it additionally writes its tile hit masks to context-owned scratch when the caller
 * passed no hitmask).  With svo_set_reflection, bounce rays that miss take the rule on their traced
 * direction.  Served: svo_render, svo_render_device, svo_render_frame (any band, layout and stream) and
 * svo_render_progressive(_async); it combines with SVO_OPT_SHADOW_RAYS, LOD and reflection without new
 * rules.  svo_count_fetches and svo_beam_starts are unaffected, and so is svo_assemble_frame: compact and
 * sparse parts get the display side's gradient on misses, so a one-process-per-GPU split with a skybox
 * sends dense RGB8 / RGBA8 parts (band renders fill them correctly).  Stated limit: svo_render_samples
 * with a texture set returns SVO_ERR_STATE before anything is enqueued.
 *
 * svo_sample_sky: the rule for caller-supplied directions -- the texture if one is set, else the gradient
 * 0.25 + 0.5 k, 0.35 + 0.55 k, 0.6 + 0.4 k with k = 0.5 y + 0.5 of the direction's y as given (an invalid
 * direction is black here too) -- the shading a ray-query user lacks for rays that miss.  d_dirs: n float4
 * (w ignored), d_rgba: n float4 (alpha 1), device pointers on the context's device (a multi-device
 * context: devices[0]), 16-byte aligned; d_rgba may be d_dirs.  Writes nothing past n entries; n == 0:
 * SVO_OK, nothing launched; NULL pointers, n > 2^31 - 1: SVO_ERR_ARG.  Asynchronous on `stream` (NULL: the
 * context's own); the host form blocks. */
enum { SVO_SKY_BILINEAR = 1, SVO_SKY_CLAMP_V = 2 };
int svo_set_skybox(svo_ctx *ctx, const float *rgba, int width, int height, uint32_t flags);   /* NULL = procedural (default) */
int svo_get_skybox(svo_ctx *ctx, int *width, int *height, uint32_t *flags);                   /* 0 x 0: none */
int svo_sample_sky(svo_ctx *ctx, const float *d_dirs, size_t n, float *d_rgba, void *stream);
int svo_sample_sky_host(svo_ctx *ctx, const float *dirs, size_t n, float *rgba);

/* Ambient: sky light with ambient occlusion (opt-in; off by default, and with it off every byte is what
 * it was).  The reference has no ambient term (a documented deviation): it lights a hit with one
 * directional light, so a pixel that faces away from it, or that the shadow pass occludes, is black.
 *
 * The ambient rule (csrc/svo_ambient.h; numpy: ambient.py).  Every operation is one IEEE f32 rounding,
 * no fma.  Direction tables for N in {4, 8, 16}: entry k is (a, b, c) with r = sqrt((k + 0.5) / N),
 * phi = (k + 0.5) pi (3 - sqrt 5), a = r cos phi, b = r sin phi, c = sqrt(1 - r r), computed in float64 and
 * rounded once; the 28 triples committed in csrc/svo_ambient.h are the truth.  Every |component| >= 2^-10
 * and c > 0.  Variant v in 0..7: if v & 4 swap a and b, then v & 3 times (a, b) -> (-b, a); all exact.
 * Per traced ray (o, d) and its hit (t, hit_scale, voxel key):
 *  1. steps 1-3 of the bounce rule above give the entry axis g, out = d_g > 0 ? -1 : +1 and the origin
 *     (P off the axis g, face_g + out side 2^-6 on it).
 *  2. direction k: dir_g = out c, dir_{(g+1)%3} = a, dir_{(g+2)%3} = b of the variant's entry k.
 *  3. the ambient ray is {origin, t_max = radius, dir, 0}, traced as svo_trace_rays traces it with flags 0
 *     (classify, the clamp -- the identity here --, the walk, then the t (1 / 64) <= t_max filter on the
 *     finished record; no early exit on radius).  radius: +inf, or positive and finite, in world units.
 *  4. the ray is open iff its record has neither flag bit 0 nor bit 4.  A record with only the
 *     iteration-cap or stack-overflow flag is open; a hit at t = 0 (an origin inside a neighbouring
 *     voxel) counts as occluded.
 * Fold per hit pixel: alb = the primary record's DXT albedo; direct = the pixel's colour as rendered with
 * ambient off (black if the record carries flag bit 3); S = (0, 0, 0); for k = 0 .. N - 1 in that order,
 * if ray k is open, S += sky of its direction (the gradient of dir_y, or the skybox rule on dir with a
 * texture set); A = S (1 / N); res_c = direct_c + (ambient_c alb_c) A_c; alpha 1.
 * Only rgba, rgba8 and rgb8 change (and through them a progressive accumulation); hits, compact, position,
 * voxel and hitmask stay the primary ray's, a shadow pass's bit 3 included; miss pixels are untouched.
 *
 * svo_set_ambient: ambient three finite numbers in [0, 4], n_rays in {0, 4, 8, 16}, radius +inf or finite
 * and > 0, variant < 8; anything else, NaN included: SVO_ERR_ARG, checked before the context is read or a
 * device touched.  NULL ambient, all-zero ambient or n_rays 0: off.  Not a svo_config field: svo_config
 * never changes results.  Leaves the dispatch-order state, tile costs, beam starts, view-change detection
 * and kernel-timing records alone (SVO_STAGE_KERNEL still brackets the primary kernel only).  The variant
 * is the same for every pixel of a launch; svo_render_progressive(_async) use (variant + sample) & 7, so
 * an accumulated frame sees up to 8 N directions.  The pass runs behind the primary launch and its shadow
 * pass (all three shadow_form's), before the sky pass.  Served: svo_render, svo_render_device,
 * svo_render_frame (any band, layout and stream) and svo_render_progressive(_async); it combines with
 * SVO_OPT_SHADOW_RAYS and a skybox texture.  svo_count_fetches, svo_beam_starts and svo_assemble_frame are
 * unaffected; a launch that writes no colour output has no ambient pass.  Stated limits, each SVO_ERR_STATE
 * before anything is enqueued: a render with reflection on, a render with LOD on, svo_render_samples; and
 * a non-off setting on a multi-device context.  svo_get_ambient: every pointer may be NULL.
 *
 * svo_ambient_rays: out[i n_rays + k] = ray k of rays[i] if hits[i] has flag bit 0, else the dead ray
 * (svo_bounce_rays') for every k.  flags: SVO_QUERY_RAW_DIRECTIONS only (how rays[i] was traced).  n_rays
 * in {4, 8, 16}; n n_rays <= 2^31 - 1.  Writes nothing past n n_rays entries; the output must not overlap
 * an input (SVO_ERR_ARG).  NULL pointers, unknown flag bits, a bad n_rays, radius or variant: SVO_ERR_ARG
 * before any device is touched; n == 0: SVO_OK, nothing launched.  Reads no pool.  Ray lists 16-byte
 * aligned, records and keys 8-byte.  A multi-device context runs it on devices[0].  Asynchronous on
 * `stream`; the host form blocks. */
enum { SVO_AMBIENT_MAX_RAYS = 16 };
int svo_set_ambient(svo_ctx *ctx, const float ambient[3], int n_rays, float radius, uint32_t variant);   /* NULL / 0 = off (default) */
int svo_get_ambient(svo_ctx *ctx, float ambient[3], int *n_rays, float *radius, uint32_t *variant);
int svo_ambient_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                     const uint64_t *d_voxel, int n_rays, float radius, uint32_t variant, svo_ray *d_rays_out,
                     void *stream);
int svo_ambient_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                          const uint64_t *voxel, int n_rays, float radius, uint32_t variant, svo_ray *rays_out);

/* Lights: up to 8 point lights with shadow rays (opt-in; none by default, and with none every byte and
 * every launch is what it was).  The reference has _DirectionalLight only (a documented deviation).
 *
 * The light rule (csrc/svo_light.h; numpy: lights.py).  Every operation is one IEEE f32 rounding, no fma;
 * only + - * /, sqrt, compares and selects.  Per traced ray (o, d after the query's clamp), its hit
 * (t, hit_scale, voxel key, record normal n) and a light (p, R, c, flags):
 *  1. steps 1-3 of the bounce rule above give the entry axis g, out = d_g > 0 ? -1 : +1 and the origin Q
 *     (P off the axis g, face_g + out side 2^-6 on it).
 *  2. L_k = p_k - Q_k.  The light is facing iff L_g out > 0 (ordered; the product is exact): a light behind
 *     the plane of the face the camera sees lights nothing there.
 *  3. d2 = (L0 L0 + L1 L1) + L2 L2, u = d2 / (R R).  The light is in range iff u < 1 (ordered; NaN: false).
 *  4. not facing, or out of range: no ray and no contribution.
 *  5. the shadow ray is {Q, t_max = 1, dir = L, 0}, traced as svo_trace_rays traces it with flags 0:
 *     classify, the small-direction clamp (it can move a component of L below 2^-23: the traced direction is
 *     the clamped one, shading keeps L), the walk, then the t (1 / 64) <= t_max filter on the finished
 *     record, no early exit.  The direction is the unnormalised L, so parameter 1 is the light itself and a
 *     hit beyond the light is filtered to a miss.  The pixel is lit by this light iff the record has neither
 *     flag bit 0 nor bit 4.  A record with only the iteration-cap or stack-overflow flag is lit; a hit at
 *     t = 0 is occluded.  With SVO_LIGHT_NO_SHADOW the step is skipped: facing and in range means lit.
 *  6. dist = sqrt(d2); ndl = ((n0 L0 + n1 L1) + n2 L2) / dist; s = ndl > 0 ? ndl : 0, then s < 1 ? s : 1
 *     (the directional light's saturate; NaN gives 0); w = 1 - u u, then w = w w; a = w / (1 + d2);
 *     k = s a; contrib_c = (k c_c) alb_c with alb the primary record's DXT albedo.
 *  7. fold per hit pixel: res = the pixel's colour as rendered with lights off (black if the record carries
 *     flag bit 3); for j = 0 .. n_lights - 1 in that order, if lit by light j, res_c = res_c + contrib_c;
 *     alpha 1.
 * Only rgba, rgba8 and rgb8 change (and through them a progressive accumulation); hits, compact, position,
 * voxel and hitmask stay the primary ray's, a shadow pass's bit 3 included; miss pixels are untouched.
 *
 * svo_set_lights copies the host array.  n_lights outside 0..8; or, in a non-NULL list, a position
 * component that is not finite or has |p_k| > 2^20, a range not in (0, 2^20], a colour component that is
 * negative, NaN or > 65536, unknown flag bits: SVO_ERR_ARG, checked before the context is read or a device
 * touched.  NULL or n_lights 0: off.  Not a svo_config field: svo_config never changes results.  Leaves the
 * dispatch-order state, tile costs, beam starts, view-change detection and kernel-timing records alone
 * (SVO_STAGE_KERNEL still brackets the primary kernel only), and the primary launch takes exactly the path
 * it takes with lights off.  The pass runs behind the primary launch and its shadow pass (all three
 * shadow_form's), before the sky pass.  Served: svo_render, svo_render_device, svo_render_frame (any band,
 * layout and stream) and svo_render_progressive(_async); it combines with SVO_OPT_SHADOW_RAYS and a skybox
 * texture (which only fills miss pixels: lights do not sample it).  svo_count_fetches, svo_beam_starts and
 * svo_assemble_frame are unaffected; a launch that writes no colour output has no light pass.  Stated
 * limits, each SVO_ERR_STATE before anything is enqueued: a render with lights and reflection on, with
 * lights and LOD on, with lights and a non-off ambient setting (the ambient pass rebuilds the direct colour
 * from the record and would drop the lights' share), svo_render_samples with lights; and a non-empty list
 * on a multi-device context.  svo_get_lights: copies min(cap, n) lights, *n_lights = n; pointers nullable.
 *
 * svo_light_rays: out[i n_lights + j] = the shadow ray of rays[i] toward lights[j] (a HOST array, 1..8
 * valid lights) if hits[i] has flag bit 0 and the light is facing and in range, else the dead ray
 * (svo_bounce_rays').  The lights' flags are not read: the call is geometry only.  flags:
 * SVO_QUERY_RAW_DIRECTIONS only (how rays[i] was traced).  n n_lights <= 2^31 - 1.  Writes nothing past
 * n n_lights entries; the output must not overlap an input (SVO_ERR_ARG).  NULL pointers, unknown flag
 * bits, a bad light: SVO_ERR_ARG before any device is touched; n == 0: SVO_OK, nothing launched.  Reads no
 * pool.  Ray lists 16-byte aligned, records and keys 8-byte.  A multi-device context runs it on
 * devices[0].  Asynchronous on `stream`; the host form blocks. */
typedef struct svo_light {      /* 32 bytes */
    float position[3];          /* world space */
    float range;                /* world units, finite, 0 < range <= 2^20 */
    float colour[3];            /* colour x intensity, each finite in [0, 65536] */
    uint32_t flags;             /* SVO_LIGHT_NO_SHADOW */
} svo_light;
enum { SVO_MAX_LIGHTS = 8 };
enum { SVO_LIGHT_NO_SHADOW = 1 };   /* no shadow ray: facing and in range means lit */
int svo_set_lights(svo_ctx *ctx, const svo_light *lights, int n_lights);          /* NULL / 0 = off (default) */
int svo_get_lights(svo_ctx *ctx, svo_light *lights, int cap, int *n_lights);
int svo_light_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                   const uint64_t *d_voxel, const svo_light *lights, int n_lights, svo_ray *d_rays_out, void *stream);
int svo_light_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                        const uint64_t *voxel, const svo_light *lights, int n_lights, svo_ray *rays_out);

/* Scene objects: sub-SVOs of the context's pool placed in the world (opt-in; none by default, and with
 * none every byte and every launch is what it was).  An object is a tree uploaded behind the terrain with
 * svo_set_buffer(.., dst_offset) -- v1 descriptors are relative, so it is uploaded as it is -- and a
 * placement: a position, a rotation and a power-of-two scale.  Moving it is one svo_set_objects call; no
 * pool is rebuilt.  The reference only sketched this (Clipmap.compute's chunk loop, never compiled in).
 *
 * The object rule (csrc/svo_object.h; numpy: objects.py).  Every operation is one IEEE f32 rounding, no
 * fma; only + - * /, compares and selects.  A world ray (o, d, t_max) and an object (root, k, p, R), with
 * s = 2^-k (exact):
 *  1. classify the world ray as svo_trace_rays does: a non-finite component, a NaN t_max or an all-zero d
 *     makes it invalid, and an invalid ray has no candidate anywhere.
 *  2. q_i = o_i - p_i; o'_j = ((R_0j q_0 + R_1j q_1) + R_2j q_2) s; d'_j = ((R_0j d_0 + R_1j d_1) + R_2j d_2) s.
 *     Origin and direction take the same exact scale, so the ray parameter is shared: a record's t / 64 is
 *     the world ray's own parameter for the terrain and for every object.
 *  3. the object ray is {o', t_max, d', 0}.  It is classified again (d' can underflow to zero, o' can
 *     overflow): invalid means no candidate in this object.  Unless SVO_QUERY_RAW_DIRECTIONS is set, the
 *     small-direction clamp applies to d'.  Note: (x 1 + y 0) + z 0 turns a -0 component into +0, so an
 *     identity placement is byte-identical to svo_trace_rays only for rays without negative-zero components.
 *  4. cube test (part of the rule: the walk's t_min is not provably monotone in f32).  t_in, t_out = the
 *     walk's own entry (after its max(.., 0)) and exit of the cube [1, 2]^3 for the clamped object ray;
 *     t_entry = fl(fl(32 t_in) 64).  The object is walked iff t_in <= t_out (ordered) and (the best record so
 *     far is a miss or t_entry < best.t).  Otherwise no walk and no candidate.
 *  5. the walk is IntersectSVO exactly as the query runs it, in the given stack mode, with parent = root
 *     after the ray setup; then the query's t (1 / 64) <= t_max filter on the finished record.  The record's
 *     parent is the absolute pool index; hit_idx, hit_scale, t and the flags are the walk's own; the normal
 *     is rotated to world, n_i = (R_i0 m_0 + R_i1 m_1) + R_i2 m_2 with m the walk's record normal, not
 *     renormalised.  Position and voxel key stay OBJECT-LOCAL (the hit position's definition on the object
 *     ray); the world hit point is o + (t / 64) d.
 *  6. fold.  Candidates in a fixed order: the terrain (root 0, the world ray traced as svo_trace_rays traces
 *     it) unless SVO_SCENE_NO_TERRAIN, then objects 0 .. n - 1.  The best is the first candidate with flag
 *     bit 0; a later one replaces it iff its t < the best t (ordered, strict: ties keep the earlier).  If
 *     nothing hit, the result is the terrain's record when the terrain was a candidate (its iteration-cap
 *     and overflow flags survive, and an invalid ray keeps its flag 0x10), else the plain miss record.
 *     Object id: -1 a miss, 0 the terrain, j + 1 object j.
 * Every walk of a scene query and of the object pass runs the guarded loop form on the 21-slot stack (proven
 * safe on cyclic and over-deep pools; the same bytes as the unguarded form on proper trees), so nothing
 * about an object's subtree needs validating.  A ray that leaves an object's root pops parent 0.
 *
 * svo_object_rays: out[i] = the object ray of steps 2-3 BEFORE the clamp, {o', t_max, d', 0}; the dead ray
 * of svo_bounce_rays when the world ray is invalid.  Geometry only: reads no pool, the object's root is
 * not read.  d_rays_out may be d_rays.  flags: SVO_QUERY_RAW_DIRECTIONS is accepted and changes nothing (the
 * result is the unclamped ray either way); any other bit, a NULL pointer, an invalid object, n > 2^31 - 1:
 * SVO_ERR_ARG before any device is touched; n == 0: SVO_OK, nothing launched.  Ray lists 16-byte aligned.
 * Asynchronous on `stream`; the host form blocks.  A multi-device context runs it on devices[0].
 *
 * svo_trace_scene: svo_trace_rays over the terrain and `objects`, a HOST array of 0 .. 8 objects (copied
 * before the call returns).  The context's own list is neither read nor changed.  flags:
 * SVO_QUERY_RAW_DIRECTIONS and SVO_SCENE_NO_TERRAIN; SVO_QUERY_ORDERED is SVO_ERR_ARG in this version.
 * Outputs as svo_trace_rays' (every non-NULL output fully written, mask tail bits 0) plus d_object (nullable,
 * n entries); out and d_object not all NULL.  n_objects == 0 without SVO_SCENE_NO_TERRAIN gives
 * svo_trace_rays' bytes.  An invalid object, n_objects outside 0 .. 8, a root >= the context's capacity:
 * SVO_ERR_ARG before any device is touched.  A root past the uploaded nodes reads the zero descriptor and
 * hits nothing.  No pool uploaded: SVO_ERR_STATE.  The host form has no mask output.
 *
 * svo_set_objects: the list used by renders; the host array is copied, NULL or 0 turns objects off.  Not
 * a svo_config field.  It leaves the dispatch-order state, tile costs, beam starts, view-change detection
 * and kernel-timing records alone, and the primary launch takes exactly the path it takes without objects.
 * The object pass runs behind the primary launch and before the sky pass: per pixel the camera ray (traced
 * as given, like the primary ray: no clamp, t_max +inf), the primary record as the best so far, steps 2-6
 * for objects 0 .. n - 1.  A pixel whose best changed gets every output the launch writes: hits (rotated
 * normal) and compact; position and voxel, object-local; colour through the Shade rule with the rotated
 * normal and the new record's DXT albedo in rgba, rgba8 and rgb8 (and through them a progressive
 * accumulation); its bit in the tile's hit-mask word, so a skybox leaves it alone.  Untouched pixels keep
 * every byte.  Which object a pixel shows is readable from `parent` (objects live in their own pool ranges).
 * Served: svo_render, svo_render_device, svo_render_frame (any band, layout and stream) and
 * svo_render_progressive(_async); it combines with a skybox texture.  svo_count_fetches, svo_beam_starts and
 * svo_assemble_frame are unaffected; a compact part rebuilds an object pixel's normal from `parent`
 * UNROTATED, so a one-process-per-GPU split with objects sends dense RGB parts.  Stated limits, each
 * SVO_ERR_STATE before anything is enqueued: a render with a non-empty list and reflection, an ambient term
 * or LOD, svo_render_samples with objects; a render with a non-empty list and SVO_OPT_SHADOW_RAYS or lights
 * unless SVO_OPT_SCENE_SHADOWS is set ("Objects in light" below); and a non-empty list on a multi-device
 * context (refused by svo_set_objects).  svo_get_objects: copies min(cap, n) objects,
 * *n_objects = n; pointers nullable. */
typedef struct svo_object {     /* 64 bytes */
    uint32_t root;              /* descriptor index of the object's root in the context's pool */
    int32_t  scale_log2;        /* k in [-8, 8]: the object's cube has side 32 * 2^k world units */
    uint32_t flags;             /* 0 (no bits defined yet; unknown bits: SVO_ERR_ARG) */
    float    position[3];       /* world position of the cube's centre, finite, |p| <= 2^20 */
    float    rotation[9];       /* row-major R, world = R * object; every entry of R R^T - I within
                                   2^-10 (checked in float64), det > 0 */
    uint32_t reserved;          /* 0 */
} svo_object;
enum { SVO_MAX_OBJECTS = 8 };
enum { SVO_SCENE_NO_TERRAIN = 4 };   /* svo_trace_scene flags: the terrain (root 0) is no candidate */
int svo_set_objects(svo_ctx *ctx, const svo_object *objects, int n_objects);        /* NULL / 0 = off (default) */
int svo_get_objects(svo_ctx *ctx, svo_object *objects, int cap, int *n_objects);
int svo_object_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_object *object,
                    svo_ray *d_rays_out, void *stream);
int svo_object_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_object *object,
                         svo_ray *rays_out);
int svo_trace_scene(svo_ctx *ctx, const svo_ray *d_rays, size_t n, int stack_mode, uint32_t flags,
                    const svo_object *objects, int n_objects, const svo_query_out *out, int32_t *d_object, void *stream);
int svo_trace_scene_host(svo_ctx *ctx, const svo_ray *rays, size_t n, int stack_mode, uint32_t flags,
                         const svo_object *objects, int n_objects, svo_hit *hits, float *position, uint64_t *voxel,
                         int32_t *object);

/* Objects in light: the light rule for the records of a scene query, whose hit may lie on a placed object,
 * a rotated and scaled voxel (csrc/svo_scene_light.h; numpy: scene_light.py).  Every operation is one IEEE
 * f32 rounding, no fma; only + - * /, sqrt, compares and selects.
 *  (a) Origin and face of a scene hit, from the traced world ray (o, d) AS GIVEN to svo_trace_scene, the
 *      record (t, hit_scale, the world normal n), the voxel key (object-local) and the object id:
 *       - id -1, an id outside -1 .. n_objects, or a record without flag bit 0: nothing; every light gets
 *         the dead ray.  No table entry is read for such an id.
 *       - id 0 (terrain): the light rule unchanged; its steps 1-2 give Q, g and out.
 *       - id c + 1, ob = objects[c] = (k, p, R):
 *          1. (o', d') = step 2 of the object rule from the world ray as given, then the small-direction
 *             clamp on d' unless SVO_QUERY_RAW_DIRECTIONS: the ray the scene query walked in the object.
 *          2. (g, out, Q') = steps 1-3 of the bounce rule on (o', d', t, hit_scale, key).  The parameter t is
 *             shared between the frames and the object frame's cube is the world convention's [-16, 16]^3.
 *          3. Q_i = (((R_i0 Q'_0 + R_i1 Q'_1) + R_i2 Q'_2) 2^k) + p_i (2^k is exact); N_i = out R_ig
 *             (exact): the entered face's outward normal in world space.
 *  (b) Toward a light (p_l, range, colour): L = p_l - Q.  An object hit is facing iff
 *      (N_0 L_0 + N_1 L_1) + N_2 L_2 > 0 (ordered); the terrain keeps L_g out > 0.  d2, u and "in range" are
 *      the light rule's step 3.  Not facing, or out of range: the dead ray.  Otherwise the ray is
 *      {Q, t_max 1, L, 0}, and the light's factor is the light rule's step 6 with the record's world normal.
 *
 * svo_scene_light_rays is svo_light_rays for the results of svo_trace_scene: out[i n_lights + j] = the
 * world-space shadow ray of hit i toward lights[j], or svo_bounce_rays' dead ray.  d_object: the ids
 * svo_trace_scene wrote (n int32, 4-byte aligned).  objects (0 .. 8, the list the batch was traced with; the
 * roots are not read or checked) and lights (1 .. 8; flags not read) are HOST arrays, copied before the call
 * returns.  flags: SVO_QUERY_RAW_DIRECTIONS only (how rays[i] was traced).  n n_lights <= 2^31 - 1.  Writes
 * nothing past n n_lights entries; the output must not overlap an input (SVO_ERR_ARG).  The argument checks
 * are svo_light_rays' and svo_trace_scene's, with their messages, before any device is touched; n == 0:
 * SVO_OK, nothing launched.  Reads no pool.  Ray lists 16-byte aligned, records and keys 8-byte.  A
 * multi-device context runs it on devices[0].  Asynchronous on `stream`; the host form blocks.  Tracing the
 * output with svo_trace_scene (flags 0, the same objects) gives the occlusion of each light over the whole
 * scene: lit iff the record has neither flag bit 0 nor bit 4.
 *
 *  (c) Occlusion over the scene.  A secondary ray is occluded iff the record svo_trace_scene gives for it --
 *      over the terrain and the context's objects, with the same flags and stack mode -- has flag bit 0.
 *      (That bit needs no nearest hit: it is "the terrain candidate hits, or some object whose cube span
 *      test t_in <= t_out holds for a valid object ray hits after the t_max filter", so the passes stop a
 *      ray at its first hit.)
 *  (d) In renders.  SVO_OPT_SCENE_SHADOWS (svo_set_options bit 8; off by default, and with it off every byte
 *      and every refusal is what it was) lets the shadow and the light pass know the objects.  With the bit
 *      set, a non-empty object list and SVO_OPT_SHADOW_RAYS and / or lights: the primary launch takes exactly
 *      the path it takes with neither (no fused shadows, whatever svo_config.shadow_form says: all three
 *      forms give the same bytes); the object pass follows; then, over the hit pixels of the finished
 *      records (the hit masks after the object pass),
 *       - the directional shadow: the shadow ray above, P + 0.001 n from the record (world normal) and the
 *         camera ray, direction -light, traced as given (raw, t_max +inf).  A ray the query's classify calls
 *         invalid is not traced and leaves the pixel lit; an occluded pixel gets flag bit 3 in hits and
 *         compact and the black Result in every colour output.  The reference's P + 0.001 n self-hit is kept
 *         as the terrain has it: an object pixel is very often shadowed by its own object.
 *       - the lights: step 7's fold of the light rule with (a)-(c): the ray {Q, 1, L} is traced with flags 0
 *         (clamped; shading keeps L); lit iff its record has neither flag bit 0 nor bit 4;
 *         SVO_LIGHT_NO_SHADOW skips the walk; res starts from the pixel's direct colour, black with bit 3;
 *         the albedo is the record's (att[parent] at hit_idx; parent is the absolute pool index).
 *      The sky pass comes last.  Only the outputs the shadow and light passes change without objects are
 *      changed.  With the bit set and an empty list every launch takes the path and writes the bytes it does
 *      with the bit clear.  Every occlusion walk is the guarded loop on the 21-slot stack.  The opt-in is
 *      also honest about cost: every shadow ray may walk up to eight more cubes.  The bit is harmless on a
 *      multi-device context (svo_set_objects refuses a non-empty list there).
 *
 * Out of scope, each SVO_ERR_STATE or SVO_ERR_ARG as before where it can be asked for: objects in bounce and
 * ambient rays (objects with reflection or an ambient term stay refused, with the bit set too); objects under
 * LOD and svo_render_samples; objects on multi-device contexts; an early exit at the light or at a radius;
 * SVO_QUERY_ORDERED for scene queries; more than eight objects, or an index over them; a directional shadow
 * ray that avoids the P + 0.001 n self-hit. */
int svo_scene_light_rays(svo_ctx *ctx, const svo_ray *d_rays, size_t n, uint32_t flags, const svo_hit *d_hits,
                         const uint64_t *d_voxel, const int32_t *d_object, const svo_object *objects, int n_objects,
                         const svo_light *lights, int n_lights, svo_ray *d_rays_out, void *stream);
int svo_scene_light_rays_host(svo_ctx *ctx, const svo_ray *rays, size_t n, uint32_t flags, const svo_hit *hits,
                              const uint64_t *voxel, const int32_t *object, const svo_object *objects, int n_objects,
                              const svo_light *lights, int n_lights, svo_ray *rays_out);

/* Volume queries: which voxels does a world-space volume touch?  Collision broad-phase, spawn placement,
 * trigger volumes, editor selection.  The reference has no volume query of any kind (a documented addition).
 * A batch of caller-supplied shapes, each an axis-aligned box or a sphere; per shape the number of leaf
 * voxels it touches, the first K of them as contact records, and one bit of a hit mask.  The query reads the
 * node pool only: it leaves every piece of render state alone (dispatch orders, tile costs, beam starts,
 * view-change detection, kernel-timing records, the progressive frame), like svo_trace_rays.
 *
 * The overlap rule (csrc/svo_overlap.h; Python: overlap.py; INTEGRATION.md "Volume queries").  Exact: voxel
 * boxes are dyadic numbers, the box test is compares only and the sphere test is monotone under rounding, so
 * the result equals a brute force over all leaves under the same test -- no margins.
 *  - Shape (svo_shape, 32 bytes, 16-byte aligned like svo_ray).  SVO_SHAPE_BOX: the closed box [p, q].
 *    SVO_SHAPE_SPHERE: centre p, radius q[0]; q[1], q[2] and reserved are 0.  INVALID: a non-finite number
 *    among p and q, p_k > q_k in a box, a negative radius, an unknown kind.  An invalid shape is not walked:
 *    count 0, visits 0, flags 0x10 (SVO_HIT_INVALID_RAY's value), no contacts, mask bit 0.
 *  - Frame: the tree's own world convention, the cube [-16, 16]^3.  The root descriptor is level 0; a child at
 *    level L with integer coordinates i has side = 2^(5 - L), lo_k = i_k side - 16, hi_k = lo_k + side, all
 *    exact in f32.  Slot c of a descriptor is the child at offset (c & 1, c >> 1 & 1, c >> 2 & 1); its valid
 *    bit is valid8 >> c & 1 and its descriptor first + popcount(nonleaf8 & ((1 << c) - 1)).
 *  - Touch.  Box: lo_k <= q_k and hi_k >= p_k for every k (closed intervals, exact compares).  Sphere:
 *    e_k = max(max(lo_k - p_k, p_k - hi_k), 0), d2 = (e0 e0 + e1 e1) + e2 e2, each operation one IEEE f32
 *    rounding, no fma; touch iff d2 <= r r (ordered).
 *  - Walk: depth-first from `root`, slots 0 .. 7 ascending.  `visits` counts descriptor fetches; an index at
 *    or past the uploaded nodes reads the zero descriptor.  A fetch that would make visits exceed max_visits
 *    sets flag bit 1 (budget) and ends the walk: count and contacts are those found so far.  For each valid
 *    child that touches: if its non-leaf bit is clear, or its level equals coarse_level (when non-zero), it
 *    is a result voxel: count += 1, stored as a contact while count <= K, and with SVO_OVERLAP_ANY the walk
 *    ends here.  Otherwise, at level 22 -- the depth limit of the guarded ray walk -- it sets flag bit 2
 *    (overflow) and is not entered.  Otherwise it is entered.  The walk therefore ends on cyclic and
 *    over-deep pools, and nothing about a pool needs validating.  Flag bit 0 is count > 0.
 *  - Contact (svo_contact, 16 bytes): parent, meta = hit_idx | hit_scale << 8 and the voxel key have svo_hit's
 *    and svo_frame.voxel's definitions for that voxel (hit_idx the slot, hit_scale 23 - level), so a contact
 *    indexes the attachments exactly as a ray hit does.  Contacts come out in walk order, which is Morton
 *    order.  Unused entries are {0xFFFFFFFF, 0, all ones}.
 * One lane of a wave takes one shape, so one huge volume holds its wave for up to max_visits dependent
 * fetches: that is what the budget is for.  Keep it small for broad-phase queries, and ask for a coarse_level
 * when the leaves are not needed.
 *
 * svo_overlap_params is versioned by its size like svo_config: the caller sets `size` = sizeof as compiled;
 * fields beyond it are 0.  NULL: all defaults.  root selects a subtree: 0 the terrain, or the root of a tree
 * uploaded behind it (svo_set_buffer's dst_offset), the shape then given in that tree's own frame.  For a
 * placed svo_object the sphere's centre is step 2 of the object rule applied to a point (q = c - p,
 * c'_j = ((R_0j q_0 + R_1j q_1) + R_2j q_2) 2^-k) and the radius r 2^-k (overlap.py object_spheres); rotated
 * boxes are out of scope, and so is a scene-wide form.
 * Outputs (svo_overlap_out: device pointers, each nullable, not all NULL): every non-NULL output is fully
 * written for all n -- summary n records, contacts n K entries (shape i's at i K), hitmask ceil(n / 64) words,
 * bit i % 64 of word i / 64 = shape i touches a voxel, the unused bits of the last word 0.  Nothing is written
 * past those.  n == 0: SVO_OK, nothing launched.  SVO_ERR_ARG, checked before any device is touched: a NULL
 * context, shapes or out, an out with every pointer NULL; a size below 8 or above this library's; unknown
 * flag bits; K > 32, contacts non-NULL with K == 0; max_visits > 2^24; coarse_level > 22; root >= the
 * context's capacity; n > 2^31 - 1 or n K > 2^31 - 1; d_shapes, summary or contacts not 16-byte aligned, the
 * mask not 8-byte aligned.  No pool uploaded: SVO_ERR_STATE.  A multi-device context runs the query on
 * devices[0].  Asynchronous on `stream` (NULL: the context's own); the host form (no mask; summary and
 * contacts nullable, not both NULL) blocks. */
enum { SVO_SHAPE_BOX = 0, SVO_SHAPE_SPHERE = 1 };
typedef struct svo_shape {      /* 32 bytes, 16-byte aligned in device memory */
    float p[3];                 /* box: the low corner; sphere: the centre */
    uint32_t kind;              /* SVO_SHAPE_BOX, SVO_SHAPE_SPHERE */
    float q[3];                 /* box: the high corner; sphere: q[0] the radius, q[1] = q[2] = 0 */
    uint32_t reserved;          /* 0 */
} svo_shape;
typedef struct svo_contact {    /* 16 bytes */
    uint32_t parent;            /* descriptor holding the voxel; 0xFFFFFFFF = unused entry */
    uint32_t meta;              /* hit_idx | hit_scale << 8 */
    uint64_t key;               /* svo_frame.voxel's key; unused: all ones */
} svo_contact;
typedef struct svo_overlap {    /* 16 bytes: one shape's summary */
    uint32_t count;             /* result voxels the shape touches (not capped by K) */
    uint32_t visits;            /* descriptor fetches of its walk */
    uint32_t flags;             /* bit0 count > 0, bit1 budget, bit2 overflow, bit4 invalid shape */
    uint32_t reserved;          /* 0 */
} svo_overlap;
enum { SVO_OVERLAP_ANY = 1 };   /* svo_overlap_params.flags: stop at the first result voxel */
enum { SVO_OVERLAP_MAX_CONTACTS = 32 };
typedef struct svo_overlap_params {
    uint32_t size;              /* sizeof(svo_overlap_params) as compiled by the caller */
    uint32_t flags;             /* SVO_OVERLAP_ANY */
    uint32_t root;              /* < capacity; 0 = the terrain */
    uint32_t max_contacts;      /* K in 0..32 */
    uint32_t max_visits;        /* 0: 65536; else 1..2^24 */
    uint32_t coarse_level;      /* 0: none; else 1..22 */
} svo_overlap_params;
typedef struct svo_overlap_out {   /* device pointers, each nullable, not all NULL */
    svo_overlap *summary;       /* n records */
    svo_contact *contacts;      /* n K entries */
    uint64_t *hitmask;          /* ceil(n/64) words */
} svo_overlap_out;
int svo_overlap_volumes(svo_ctx *ctx, const svo_shape *d_shapes, size_t n, const svo_overlap_params *params,
                        const svo_overlap_out *out, void *stream);
int svo_overlap_volumes_host(svo_ctx *ctx, const svo_shape *shapes, size_t n, const svo_overlap_params *params,
                             svo_overlap *summary, svo_contact *contacts);

/* Closest voxels: how far is this point from the surface, and where is the closest point on it?  Pushing a
 * sphere out of the terrain, conservative advancement of a moving sphere (step by distance - r), particle and
 * cloth collision, snap-to-surface, clearance tests, distance-field slices.  The reference has no such query
 * (a documented addition, like the volume queries).  A batch of caller-supplied points, each with a search
 * radius; per point the nearest result voxel, its squared distance, the closest point on it, its contact
 * record and one bit of a hit mask.  The query reads the node pool only and leaves every piece of render
 * state alone, like svo_overlap_volumes.
 *
 * The closest-voxel rule (csrc/svo_closest.h, which carries the proofs; Python: closest.py; INTEGRATION.md
 * "Closest voxels").  Exact: the pruned walk returns the voxel a brute force over all result voxels returns
 * under the same f32 expression, byte for byte.  Every operation is one IEEE f32 rounding, no fma, only + - *,
 * compares and selects; no sqrt, no division: the query reports d2 and the caller takes the root.
 *  - Query: an svo_shape of kind SVO_SHAPE_SPHERE, centre p the point, q[0] the search radius.  INVALID under
 *    svo_overlap_volumes' rule for shapes, and also when its kind is SVO_SHAPE_BOX.  An invalid query is not
 *    walked: flags 0x10, visits 0, nothing found, mask bit 0.  r2 = q[0] q[0]; with SVO_CLOSEST_UNBOUNDED the
 *    radius is ignored and r2 = +inf (the radius must still be valid).
 *  - Frame, voxel boxes, slots and the child descriptor index are the volume queries'.
 *  - Distance to a voxel box [lo, hi]: e_k = max(max(lo_k - p_k, p_k - hi_k), 0), d2 = (e0 e0 + e1 e1) + e2 e2
 *    -- the sphere touch test's expression, so a voxel is a candidate iff d2 <= r2 and "found" equals
 *    svo_overlap_volumes' touch bit for the same shape.
 *  - Result voxels are the overlap walk's: a valid child whose non-leaf bit is clear, or whose level equals
 *    coarse_level (when non-zero); a non-leaf child at level 22 sets flag bit 2 (overflow) and is not entered.
 *  - Answer: the result voxel with the smallest (d2, Morton position).  Morton position: with the aligned
 *    coordinates a_k = i_k << (22 - level), A precedes B iff, on the axis whose a_k ^ b_k has the highest set
 *    bit (bit positions tying: z before y before x), A's coordinate is smaller -- the order in which
 *    svo_overlap_volumes reports disjoint voxels.
 *  - Walk: depth-first from `root`.  bound starts at r2 and becomes the best d2 once a result voxel is found;
 *    the best is replaced iff the new d2 is smaller, or equal and Morton-earlier.  At a descriptor the pending
 *    children are the valid ones; repeatedly the pending child with the smallest (d2_c, slot c) among those
 *    with d2_c <= bound, the bound of that moment, is taken.  `visits` counts descriptor fetches; an index at
 *    or past the uploaded nodes reads the zero descriptor.  A fetch that would make visits exceed max_visits
 *    sets flag bit 1 (budget) and ends the walk with the best so far, which may then not be the nearest.  The
 *    walk ends on cyclic and over-deep pools.
 *  - Closest point: c_k = min(max(p_k, lo_k), hi_k), exact.  d2 == 0: the point lies in or on the voxel.
 *  - Against real arithmetic (no e_k e_k under- or overflowing): d2, and the true squared distance of the
 *    answer, are within a relative 11 * 2^-24 of the true minimum over all result voxels.
 * svo_closest_params is versioned by its size like svo_overlap_params; NULL: all defaults.  root selects a
 * tree as in svo_overlap_volumes; for a placed svo_object move the point as closest.py object_queries does.
 * Outputs (svo_closest_out: device pointers, each nullable, not all NULL): every non-NULL output is fully
 * written for all n -- nearest n records, contacts n entries (the answer's svo_contact; nothing found:
 * {0xFFFFFFFF, 0, all ones}), hitmask ceil(n / 64) words, bit i % 64 of word i / 64 = query i found a voxel,
 * the unused bits of the last word 0.  Nothing is written past those.  n == 0: SVO_OK, nothing launched.
 * SVO_ERR_ARG, checked before any device is touched: a NULL context, queries or out, an out with every pointer
 * NULL; a size below 8 or above this library's; unknown flag bits; max_visits > 2^24; coarse_level > 22;
 * root >= the context's capacity; n > 2^31 - 1; d_queries, nearest or contacts not 16-byte aligned, the mask
 * not 8-byte aligned.  No pool uploaded: SVO_ERR_STATE.  A multi-device context runs the query on devices[0].
 * Asynchronous on `stream` (NULL: the context's own); the host form (no mask; nearest and contacts nullable,
 * not both NULL) blocks. */
enum { SVO_CLOSEST_UNBOUNDED = 1 };   /* svo_closest_params.flags: ignore the search radius */
typedef struct svo_closest {    /* 32 bytes, 16-byte aligned in device memory */
    float point[3];             /* closest point on the voxel's closed box; not found: 0, 0, 0 */
    float d2;                   /* squared distance by the rule; not found: +inf */
    uint32_t parent, meta;      /* as svo_contact; not found: 0xFFFFFFFF, 0 */
    uint32_t visits;            /* descriptor fetches of the walk */
    uint32_t flags;             /* bit0 found, bit1 budget, bit2 overflow, bit4 invalid query */
} svo_closest;
typedef struct svo_closest_params {
    uint32_t size;              /* sizeof(svo_closest_params) as compiled by the caller */
    uint32_t flags;             /* SVO_CLOSEST_UNBOUNDED */
    uint32_t root;              /* < capacity; 0 = the terrain */
    uint32_t max_visits;        /* 0: 65536; else 1..2^24 */
    uint32_t coarse_level;      /* 0: none; else 1..22 */
} svo_closest_params;
typedef struct svo_closest_out {   /* device pointers, each nullable, not all NULL */
    svo_closest *nearest;       /* n records */
    svo_contact *contacts;      /* n entries */
    uint64_t *hitmask;          /* ceil(n/64) words */
} svo_closest_out;
int svo_closest_voxels(svo_ctx *ctx, const svo_shape *d_queries, size_t n, const svo_closest_params *params,
                       const svo_closest_out *out, void *stream);
int svo_closest_voxels_host(svo_ctx *ctx, const svo_shape *queries, size_t n, const svo_closest_params *params,
                            svo_closest *nearest, svo_contact *contacts);

/* Information about the uploaded pool. */
int svo_get_info(svo_ctx *ctx, size_t *n_nodes, int *max_depth, int *device);

/* Block until all work of the context has finished: its own stream and every
 * caller stream it rendered, assembled or accumulated on (a device-wide
 * synchronise of each of its devices). */
int svo_synchronize(svo_ctx *ctx);

/* Let go of a caller stream before the caller destroys it: waits for the work the
 * context enqueued on it and frees the stream's dispatch-order state (a multi-device
 * context: every member).  A stream never passed in is not an error.  (ABI 9) */
int svo_forget_stream(svo_ctx *ctx, void *stream);

/* Release device memory (the reference never Release()s its buffers). */
int svo_destroy(svo_ctx *ctx);

/* Thread-local text of the last error (empty string if none). */
const char *svo_last_error(void);

/* ABI version, bumped on any layout change. */
int svo_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
