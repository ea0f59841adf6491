/*
 * raycast_min.c -- ray queries from plain C (svo_trace_rays_host, include/svo_rt.h): what a
 * host does for picking or a height probe -- the reference's CPU-side SVO.Trace(Ray)
 * (Interfaces.cs:6-15, driven by SVODriver.UpdateRaycast, SVODriver.cs:74-87) on the GPU.
 *
 * Scene: render_min.c's one-level SVO (the root's 8 children are all solid leaves), i.e. the
 * whole [-16, 16]^3 world cube.  Two rays:
 *   down     : from (3, 40, 5) straight down (0, -1, 0) -- exactly axis-aligned, the ray the
 *              reference's arithmetic loses (its small-direction clamp is commented out,
 *              NVIDIASVO.compute:21-24; the plugin restores it).  It enters the top face
 *              y = 16 after 24 world units: t = 24 * 64 = 1536, child slot 7 (+x, +y, +z).
 *   diagonal : from (-40, -38, -36) along (1, 1, 1) / sqrt(3): it enters the face x = -16 at
 *              (-16, -14, -12) after 24 sqrt(3) world units, child slot 0.
 * A third call repeats the first ray with t_max = 10: the hit lies beyond it, so a miss.
 *
 *   gcc -O2 -Iinclude examples/raycast_min.c -Lraytracingtest_amd -lsvo_rt \
 *       -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/raytracingtest_amd -o raycast_min
 *   ./raycast_min              exit status 0 = the checks passed
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "svo_rt.h"

static int check(int rc, const char *what) {
    if (rc != SVO_OK) {
        fprintf(stderr, "%s failed (%d): %s\n", what, rc, svo_last_error());
        exit(1);
    }
    return rc;
}

static void print_record(const char *name, const svo_hit *h, const float *pos, uint64_t voxel) {
    printf("%s: hit %d parent %u idx %u scale %u flags %u t %.9g n (%.9g %.9g %.9g) position (%.9g %.9g %.9g) "
           "voxel %llu\n", name, h->flags & 1, h->parent, h->hit_idx, h->hit_scale, h->flags, h->t, h->nx, h->ny,
           h->nz, pos[0], pos[1], pos[2], (unsigned long long)voxel);
}

int main(void) {
    /* descriptor: ptr16 << 16 | valid8 << 8 | nonleaf8 (NaiveCreator.cs:184-187) */
    const int32_t desc[1] = { 0x0000FF00 };
    /* attachment pair: colours A|B (565, R in the low bits), choices | normal16 << 16 */
    const uint32_t att[2] = { 0x001Fu | (0xF800u << 16), 0x0000u | (0xC000u << 16) };
    const float s = 1.0f / sqrtf(3.0f);
    svo_ray rays[2] = {
        { { 3.0f, 40.0f, 5.0f }, INFINITY, { 0.0f, -1.0f, 0.0f }, 0 },
        { { -40.0f, -38.0f, -36.0f }, INFINITY, { s, s, s }, 0 },
    };
    svo_hit hits[2];
    float pos[2][4];
    uint64_t voxel[2];

    svo_ctx *ctx = NULL;
    check(svo_create(0, 1024, &ctx), "svo_create");
    check(svo_set_buffer(ctx, desc, 1, att, 2, 0), "svo_set_buffer");   /* no camera: a query needs none */
    check(svo_trace_rays_host(ctx, rays, 2, SVO_STACK_HLSL, 0, hits, &pos[0][0], voxel), "svo_trace_rays_host");
    print_record("down", &hits[0], pos[0], voxel[0]);
    print_record("diagonal", &hits[1], pos[1], voxel[1]);

    /* world hit point = origin + (t / 64) * dir */
    const float y_hit = rays[0].origin[1] + hits[0].t / 64.0f * rays[0].dir[1];
    int ok = (hits[0].flags & 1) && hits[0].parent == 0 && hits[0].hit_idx == 7 && hits[0].hit_scale == 22 &&
             fabsf(hits[0].t - 1536.0f) < 0.01f && fabsf(y_hit - 16.0f) < 1e-3f;
    ok = ok && (hits[1].flags & 1) && hits[1].parent == 0 && hits[1].hit_idx == 0 && hits[1].hit_scale == 22 &&
         fabsf(hits[1].t / 64.0f - 24.0f * sqrtf(3.0f)) < 1e-3f;

    rays[0].t_max = 10.0f;   /* the cube is 24 units away */
    svo_hit near_hit;
    check(svo_trace_rays_host(ctx, rays, 1, SVO_STACK_HLSL, 0, &near_hit, NULL, NULL), "svo_trace_rays_host (t_max)");
    printf("down, t_max 10: hit %d parent %u flags %u\n", near_hit.flags & 1, near_hit.parent, near_hit.flags);
    ok = ok && near_hit.flags == 0 && near_hit.parent == 0xFFFFFFFFu && isinf(near_hit.t);

    check(svo_destroy(ctx), "svo_destroy");
    printf(ok ? "raycast_min: ok\n" : "raycast_min: CHECK FAILED\n");
    return ok ? 0 : 2;
}
