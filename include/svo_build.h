/*
 * svo_build.h -- C-ABI of the native SVO builder (libsvo_build.so).
 *
 * Replaces the reference's CPU builder RT.CS.NaiveCreator
 * (Assets/Scripts/SVO/CompactSVO/NaiveCreator.cs) used by
 * RaytracingMaster.SetSVOBuffer() (RaytracingMaster.cs:90-109):
 *   Create(sampler, maxLevel)   NaiveCreator.cs:10-24
 *   BuildTree / IsEdge          NaiveCreator.cs:52-130   -> GPU leaf classification (HIP)
 *   CompressSVO / GetAttachment NaiveCreator.cs:132-257  -> host layout pass (C++)
 * Samplers: SampleFunctions.functions[] (SampleFunctions.cs:13-48) with the
 * seed-7 OpenSimplex noise (Noise/Simplex.cs).
 */
#ifndef SVO_BUILD_H
#define SVO_BUILD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SampleFunctions.Type (SampleFunctions.cs:4-11) */
typedef enum svob_sampler {
    SVOB_FLAT_GROUND = 0,
    SVOB_SPHERE = 1,
    SVOB_SIMPLEX = 2,
    SVOB_ROTATED_CUBOID = 3,   /* Cuboid(Rotate(Euler(45,45,45)) p, 0.6); the rotation restated in float */
    SVOB_CUSTOM1 = 4
} svob_sampler;

typedef struct svob_result {
    size_t    n_nodes;
    int       depth;          /* descriptor levels = maxLevel - 1 */
    int       v1_ok;          /* 1 if every relative child pointer fits 16 bits */
    int32_t  *descriptors;    /* V1 words (only meaningful when v1_ok) */
    uint64_t *nodes;          /* V2 nodes: first_child_abs << 32 | valid << 8 | nonleaf */
    uint32_t *attachments;    /* 2 words per node */
    size_t    n_leaves;       /* surface voxels */
} svob_result;

/* NaiveCreator.Create(SampleFunctions.functions[sampler], max_level): leaves
 * are classified on HIP device `device`. */
int svob_build_sampler(int device, int sampler, int max_level, svob_result *out);

/* Layout only (CompressSVO): surface leaves given as integer coordinates of a
 * 2^depth grid (x, y, z interleaved), per-leaf normals (float3) and optional
 * colours (float3, NULL = position - 1 as NaiveCreator.cs:66). */
int svob_build_from_leaves(int depth, size_t n_leaves, const uint32_t *xyz, const float *normals,
                           const float *colors, svob_result *out);

/* Surface leaves only (Morton-sorted 3*depth-bit codes + normals), malloc'd. */
int svob_surface_leaves(int device, int sampler, int max_level, size_t *n_leaves,
                        uint64_t **morton_out, float **normals_out);

/*
 * Limits of the GPU leaf pass.  Zero means "default" in every field, and a NULL
 * svob_limits is all defaults: svob_build_sampler and svob_surface_leaves are the
 * _ex forms with NULL limits.  No field changes a result: every combination gives
 * the same leaves, normals and pool; they move memory and time (and let a test reach
 * the slab seams, the list regrowth and the stride loops on a small grid).
 * Versioned by size like svo_config (svo_rt.h): a caller sets `size` =
 * sizeof(svob_limits) as it was compiled, the library reads the fields that fit in it
 * and takes the default of any later one; a size below the two header words or above
 * this library's is SVOB -1 (argument error).
 *
 * Slab rule (svob_slab_rows): the leaf pass samples a byte grid of (n+2)^2 cells per
 * z-plane, n = 2^(max_level-1), in slabs of `rows` leaf planes plus one halo plane
 * below and one above:
 *     rows = clamp(cell_bytes / (n+2)^2 - 2, 1, n)      (slab_rows == 0)
 *     rows = clamp(slab_rows, 1, n)                     (slab_rows  > 0)
 * A budget that holds fewer than three planes gives rows = 1: the buffer is then
 * 3 (n+2)^2 bytes and EXCEEDS cell_bytes (max_level >= 15 at the default budget:
 * 3 x 256 MiB at max_level 15, 3 x 4 TiB at max_level 22).
 */
typedef struct svob_limits {
    uint32_t size;            /* sizeof(svob_limits) as compiled by the caller */
    uint32_t reserved;        /* 0 */
    uint64_t cell_bytes;      /* byte-grid budget of one slab, halo included (0: 512 MiB) */
    uint64_t list_capacity;   /* initial capacity of the surface list, in leaves (0: max(1 Mi, 4 n^2));
                                 a slab with more surface leaves regrows it to 1.25 x count + 1024 */
    int32_t  slab_rows;       /* leaf planes per slab, overrides cell_bytes (0: the rule above); < 0: error */
    int32_t  max_blocks;      /* cap on the blocks (of 256 threads) of each launch (0: 65,536); < 0: error */
    uint64_t launch_candidates;   /* meshes: candidate voxels per launch of the overlap kernel (0: 2^28); any
                                     value >= 1 is taken, a slab with more candidates takes several launches */
} svob_limits;

/* What the leaf pass did; filled by the _ex entries when non-NULL.  `size` is set by the
 * caller like svob_limits.size; at most `size` bytes are written. */
typedef struct svob_report {
    uint32_t size;              /* sizeof(svob_report) as compiled by the caller */
    uint32_t slabs;             /* z-slabs sampled */
    uint32_t slab_rows;         /* leaf planes per slab (the last slab may hold fewer) */
    uint32_t relaunches;        /* classify launches repeated because a slab's count exceeded the capacity */
    uint32_t normals_regrown;   /* 1: the list was re-allocated for the normal pass (all leaves > capacity) */
    uint32_t reserved;          /* 0 */
    uint64_t list_capacity;     /* capacity of the surface list when the last slab was classified */
    uint32_t overlap_launches;  /* meshes: launches of the overlap kernel, the sum over the slabs that hold a
                                   candidate of ceil(slab's candidates / launch_candidates); samplers: 0 */
    uint32_t reserved2;         /* 0 */
} svob_report;

/* Leaf planes per slab for max_level under `limits` (NULL: defaults).  Pure host
 * arithmetic, no GPU.  Returns rows >= 1, or a negative error code (svob_last_error). */
int svob_slab_rows(int max_level, const svob_limits *limits);

/* svob_build_sampler / svob_surface_leaves with limits (NULL: defaults) and an optional report. */
int svob_build_sampler_ex(int device, int sampler, int max_level, const svob_limits *limits,
                          svob_report *report, svob_result *out);
int svob_surface_leaves_ex(int device, int sampler, int max_level, const svob_limits *limits,
                           svob_report *report, size_t *n_leaves, uint64_t **morton_out, float **normals_out);

/*
 * Triangle meshes.  svob_build_mesh voxelises an indexed triangle mesh into surface leaves on
 * HIP device `device` and lays them out as svob_build_from_leaves does; svob_mesh_leaves returns
 * the leaves alone.  Vertex positions are in the cube's own unit frame [0,1]^3 (the tracer's
 * [1,2]^3); with n = 2^(max_level-1) the grid coordinate is p * n and voxel (i,j,k) is the
 * closed box [i,i+1] x [j,j+1] x [k,k+1].
 *   occupancy  a voxel is a surface leaf iff the closed triangle overlaps the closed box, decided
 *              by one f32 rule (the two-sided Schwarz-Seidel triangle/box test: three box
 *              intervals, the plane against the box's critical corner, three edge functions in
 *              each of the xy, yz and zx projections), stated term for term in
 *              raytracingtest_amd/csrc/svo_voxelize.h and in numpy in raytracingtest_amd/voxelize.py.
 *              It errs by at most 10 u (E + 2)(1 + kappa) voxel, u = 2^-24, E the triangle's
 *              largest extent in voxels, kappa the cancellation of its normal (the header derives it).
 *   skipped    a triangle whose normal normalises to zero (Vector3.Normalize, magnitude <= 1e-5
 *              in grid units) is skipped and counted in `degenerate`; one whose bounding box
 *              misses the cube in `outside`.  Parts outside [0,1]^3 contribute no voxels.
 *   owner      of the triangles that overlap a voxel the lowest index owns it.
 *   normal     Normalize((v1 - v0) x (v2 - v0)) of the owner: counter-clockwise front faces give
 *              outward normals, as the samplers' are; SVOB_MESH_FLIP_WINDING negates it.
 *   colour     with `colors`: the owner's three vertex colours at the barycentric coordinates of
 *              the voxel centre projected onto the owner's plane, each clamped at 0 and
 *              renormalised to sum 1.  Without: position - 1 (NaiveCreator.cs:66), as
 *              svob_build_from_leaves with colors = NULL.
 * The result depends on nothing else: not on svob_limits, the launch geometry or the order in
 * which the device meets the triangles.
 *
 * Refused with SVOB -1 before any launch: a NULL mesh, a size below the two header words or above
 * this library's (svob_mesh is versioned by size like svob_limits; fields past the caller's size
 * are zero), unknown flag bits, n_triangles >= 2^32 - 1, a non-finite position, an index >=
 * n_vertices, max_level outside [2, 22], and a grid of which svob_limits.cell_bytes does not hold
 * one plane (max_level >= 15 at the default 512 MiB).
 *
 * Slab rule for the mesh pass: the owner grid holds one uint32 per voxel and needs no halo, so a
 * z-slab of `rows` planes takes 4 n^2 rows bytes:
 *     rows = clamp(cell_bytes / (4 n^2), 1, n)          (slab_rows == 0)
 *     rows = clamp(slab_rows, 1, n)                     (slab_rows  > 0)
 * One slab up to max_level 10, 128 planes at max_level 11, 2 at max_level 14.  list_capacity,
 * max_blocks and svob_report keep their meaning: `relaunches` counts compactions repeated because
 * a slab held more leaves than the list, `normals_regrown` the re-allocation for the attribute pass.
 * Work is spread per candidate voxel (the voxels of every triangle's clipped box): one launch of the
 * overlap kernel takes at most `launch_candidates` of a slab's candidates (2^28), the next one goes
 * on where it ended, in the middle of a triangle's box or not; `overlap_launches` counts them.
 */
enum { SVOB_MESH_FLIP_WINDING = 1 };
typedef struct svob_mesh {          /* versioned by size like svob_limits */
    uint32_t size, flags;
    const float    *positions;  size_t n_vertices;   /* xyz, cube frame [0,1]^3 */
    const uint32_t *indices;    size_t n_triangles;  /* 3 per triangle */
    const float    *colors;                          /* rgb per vertex in [0,1], or NULL */
} svob_mesh;
typedef struct svob_mesh_stats {    /* caller sets size; at most size bytes written */
    uint32_t size, reserved;
    uint64_t degenerate, outside, candidates, overlaps;   /* triangles, triangles, tests run, (voxel, triangle) hits */
} svob_mesh_stats;

/* Mesh -> pool.  limits, report, stats may be NULL.  out: freed with svob_free. */
int svob_build_mesh (int device, const svob_mesh *mesh, int max_level, const svob_limits *limits,
                     svob_report *report, svob_mesh_stats *stats, svob_result *out);
/* Mesh -> surface leaves, Morton-sorted unique codes (x bit 0, y bit 1, z bit 2), normals (float3),
 * colours (float3; colors_out may be NULL and receives NULL when the mesh has no colours) and the
 * owning triangle of each leaf; malloc'd, freed with svob_free_ptr. */
int svob_mesh_leaves(int device, const svob_mesh *mesh, int max_level, const svob_limits *limits,
                     svob_report *report, svob_mesh_stats *stats, size_t *n_leaves,
                     uint64_t **morton_out, float **normals_out, float **colors_out, uint32_t **owner_out);

/* Measurement (tools/voxelize_bench.py): with enable != 0 the calling thread's later mesh calls time
 * every kernel with device events and wait after each launch -- slower builds, same results.
 * ms_out (NULL-able) first receives the sums of the thread's last timed call, in milliseconds:
 * setup, count, scan, overlap, compact, attributes. */
enum { SVOB_MESH_KERNELS = 6 };
int svob_mesh_profile(int enable, double *ms_out /* SVOB_MESH_KERNELS */);

/* Evaluate a sampler on the host (for tests): n points (x,y,z interleaved). */
int svob_eval_sampler(int sampler, size_t n, const float *xyz, float *out);

/* OpenSimplex 3D contribution table (2048 hashes x up to 8 lattice offsets):
 * out[h*25] = count (0 = no entry), then count x (dx, dy, dz) int8 offsets. */
int svob_opensimplex_table(int8_t *out /* 2048 * 25 */);

void svob_free(svob_result *r);
void svob_free_ptr(void *p);
const char *svob_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
