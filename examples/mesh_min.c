/*
 * mesh_min.c -- a triangle mesh as a scene object, from plain C: mesh -> pool -> object
 * (svob_build_mesh in include/svo_build.h; svo_set_buffer_v2, svo_set_objects, svo_trace_scene_host and
 * svo_render in include/svo_rt.h).
 *
 *   1. the terrain: svob_build_sampler(SVOB_CUSTOM1, 6), uploaded at node 0;
 *   2. the mesh: an octahedron generated here (6 vertices, 8 counter-clockwise faces, |x| + |y| + |z| = 0.4 about
 *      the centre of the unit cube) with a colour per vertex, voxelised at max_level 6 (a 32^3 grid);
 *   3. its pool goes BEHIND the terrain with svo_set_buffer_v2(..., dst_offset = the terrain's node count).  Wide
 *      nodes hold absolute first-child indices, so a pool that does not start at node 0 is rebased first;
 *   4. svo_object { root = dst_offset, scale_log2 = -2 }: an 8-unit cube above the terrain, before the camera.
 * The pick ray runs along +z at (0.3, 8.2) through the object's cube centred at (0, 8, -20): it meets the face
 * |x| + |y| + |z| = 3.2 (world units about the centre) at z = -22.7, 17.3 units from its origin, within a voxel
 * diagonal (0.25 sqrt(3)); the face looks toward -z.  The frame must show the object too.
 *
 *   gcc -O2 -Iinclude examples/mesh_min.c -Lraytracingtest_amd -lsvo_rt -lsvo_build \
 *       -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/raytracingtest_amd -o mesh_min
 *   ./mesh_min                 exit status 0 = the checks passed
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "svo_build.h"
#include "svo_rt.h"

#define W 64
#define H 64

static void check(int rc, const char *what) {
    if (rc != SVO_OK) {
        fprintf(stderr, "%s failed (%d): %s\n", what, rc, svo_last_error());
        exit(1);
    }
}

static void check_build(int rc, const char *what) {
    if (rc != 0) {
        fprintf(stderr, "%s failed (%d): %s\n", what, rc, svob_last_error());
        exit(1);
    }
}

int main(void) {
    /* the octahedron: +x -x +y -y +z -z, faces counter-clockwise seen from outside */
    const float r = 0.4f, c = 0.5f;
    const float positions[6 * 3] = { c + r, c, c,  c - r, c, c,  c, c + r, c,  c, c - r, c,  c, c, c + r,  c, c, c - r };
    const float colors[6 * 3] = { 1, 0, 0,  0, 1, 1,  0, 1, 0,  1, 0, 1,  0, 0, 1,  1, 1, 0 };
    const uint32_t indices[8 * 3] = { 0, 2, 4,  2, 1, 4,  1, 3, 4,  3, 0, 4,  2, 0, 5,  1, 2, 5,  3, 1, 5,  0, 3, 5 };

    svob_result terrain, pool;
    check_build(svob_build_sampler(0, SVOB_CUSTOM1, 6, &terrain), "svob_build_sampler");

    svob_mesh mesh;
    memset(&mesh, 0, sizeof mesh);
    mesh.size = sizeof mesh;
    mesh.positions = positions;
    mesh.n_vertices = 6;
    mesh.indices = indices;
    mesh.n_triangles = 8;
    mesh.colors = colors;
    svob_mesh_stats stats;
    memset(&stats, 0, sizeof stats);
    stats.size = sizeof stats;
    check_build(svob_build_mesh(0, &mesh, 6, NULL, NULL, &stats, &pool), "svob_build_mesh");
    printf("mesh: 8 triangles -> %zu surface voxels, %zu nodes (%llu candidate voxels tested, %llu overlaps, "
           "%llu degenerate, %llu outside)\n", pool.n_leaves, pool.n_nodes, (unsigned long long)stats.candidates,
           (unsigned long long)stats.overlaps, (unsigned long long)stats.degenerate, (unsigned long long)stats.outside);

    const size_t offset = terrain.n_nodes;
    for (size_t i = 0; i < pool.n_nodes; ++i)   /* rebase: first-child indices are absolute in the wide format */
        if (pool.nodes[i] & 0xFFu) pool.nodes[i] += (uint64_t)offset << 32;

    svo_ctx *ctx = NULL;
    check(svo_create(0, terrain.n_nodes + pool.n_nodes, &ctx), "svo_create");
    check(svo_set_buffer_v2(ctx, terrain.nodes, terrain.n_nodes, terrain.attachments, 2 * terrain.n_nodes, 0),
          "svo_set_buffer_v2 (terrain)");
    check(svo_set_buffer_v2(ctx, pool.nodes, pool.n_nodes, pool.attachments, 2 * pool.n_nodes, offset),
          "svo_set_buffer_v2 (mesh pool)");

    svo_object ob;
    memset(&ob, 0, sizeof ob);
    ob.root = (uint32_t)offset;
    ob.scale_log2 = -2;
    ob.position[0] = 0.0f;
    ob.position[1] = 8.0f;
    ob.position[2] = -20.0f;
    ob.rotation[0] = ob.rotation[4] = ob.rotation[8] = 1.0f;

    const svo_ray pick = { { 0.3f, 8.2f, -40.0f }, INFINITY, { 0.0f, 0.0f, 1.0f }, 0 };
    svo_hit hit;
    int32_t id = 99;
    check(svo_trace_scene_host(ctx, &pick, 1, SVO_STACK_HLSL, 0, &ob, 1, &hit, NULL, NULL, &id), "svo_trace_scene_host");
    const float dist = hit.t / 64.0f;
    printf("pick: id %d parent %u t %.9g (%.9g world units), normal (%.9g %.9g %.9g)\n", id, hit.parent, hit.t, dist, hit.nx,
           hit.ny, hit.nz);
    int ok = id == 1 && (hit.flags & 1) && hit.parent >= offset && fabsf(dist - 17.3f) <= 0.25f * 1.7321f && hit.nz < 0.0f;

    /* the same object in a frame: camera at (0, 4, -40) looking along +z, as render_min.c builds it */
    const float fov = 60.0f * 3.14159265358979f / 180.0f, n = 0.3f, f = 1000.0f, aspect = (float)W / H;
    const float cot = 1.0f / tanf(fov * 0.5f);
    float inv_proj[16] = { 0 };
    inv_proj[0 * 4 + 0] = aspect / cot;
    inv_proj[1 * 4 + 1] = 1.0f / cot;
    inv_proj[3 * 4 + 2] = -1.0f;
    inv_proj[2 * 4 + 3] = (n - f) / (2.0f * f * n);
    inv_proj[3 * 4 + 3] = (f + n) / (2.0f * f * n);
    float c2w[16] = { 0 };
    c2w[0 * 4 + 0] = 1.0f;
    c2w[1 * 4 + 1] = 1.0f;
    c2w[2 * 4 + 2] = -1.0f;
    c2w[3 * 4 + 1] = 4.0f;
    c2w[3 * 4 + 2] = -40.0f;
    c2w[3 * 4 + 3] = 1.0f;
    const float light[4] = { 0.3f, -0.5f, 0.8f, 1.0f };
    check(svo_set_camera(ctx, c2w, inv_proj, 0.5f, 0.5f, light), "svo_set_camera");
    check(svo_set_objects(ctx, &ob, 1), "svo_set_objects");
    float *rgba = (float *)malloc(sizeof(float) * 4 * W * H);
    svo_hit *hits = (svo_hit *)malloc(sizeof(svo_hit) * W * H);
    if (!rgba || !hits) return 3;
    check(svo_render(ctx, W, H, SVO_STACK_HLSL, rgba, hits), "svo_render");
    int on_object = 0, on_terrain = 0;
    for (int i = 0; i < W * H; ++i) {
        if (!(hits[i].flags & 1)) continue;
        if (hits[i].parent >= offset) ++on_object; else ++on_terrain;
    }
    printf("frame %dx%d: %d pixels on the mesh object, %d on the terrain\n", W, H, on_object, on_terrain);
    ok = ok && on_object > 20 && on_terrain > 20;

    free(rgba);
    free(hits);
    check(svo_destroy(ctx), "svo_destroy");
    svob_free(&terrain);
    svob_free(&pool);
    printf(ok ? "mesh_min: ok\n" : "mesh_min: CHECK FAILED\n");
    return ok ? 0 : 2;
}
