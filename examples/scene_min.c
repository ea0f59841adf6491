/*
 * scene_min.c -- scene objects from plain C (svo_set_buffer at an offset, svo_trace_scene_host,
 * include/svo_rt.h): two trees in one pool, one of them placed in the world and moved every frame
 * without rebuilding anything -- what the reference's Clipmap.compute chunk loop was meant to become.
 *
 * Pool: render_min.c's one-level SVO (the root's 8 children are all solid leaves) twice:
 *   descriptor 0 : the terrain, the whole [-16, 16]^3 world cube;
 *   descriptor 1 : the object's tree, uploaded as it is (v1 descriptors are relative).
 * The object is a 4-unit cube (scale_log2 = -3) turned 90 degrees about the vertical, 6 units above the
 * terrain's top face; frame f puts its centre at x = -8 + 4 f.  The pick ray goes straight down from
 * (0.5, 40, 0.5): in frame 2 the object lies under it -- its top face y = 24 after 16 world units, so
 * t = 16 * 64 = 1024, object id 1, parent 1 -- and in every other frame the ray reaches the terrain's top
 * face after 24 units: t = 1536, object id 0, parent 0.  t / 64 is the world ray's own parameter for
 * both.  With SVO_SCENE_NO_TERRAIN the other frames are misses (id -1).
 *
 *   gcc -O2 -Iinclude examples/scene_min.c -Lraytracingtest_amd -lsvo_rt \
 *       -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/raytracingtest_amd -o scene_min
 *   ./scene_min                exit status 0 = the checks passed
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "svo_rt.h"

static int check(int rc, const char *what) {
    if (rc != SVO_OK) {
        fprintf(stderr, "%s failed (%d): %s\n", what, rc, svo_last_error());
        exit(1);
    }
    return rc;
}

int main(void) {
    /* descriptor: ptr16 << 16 | valid8 << 8 | nonleaf8 (NaiveCreator.cs:184-187) */
    const int32_t desc[1] = { 0x0000FF00 };
    /* attachment pair: colours A|B (565, R in the low bits), choices | normal16 << 16 */
    const uint32_t att[2] = { 0x001Fu | (0xF800u << 16), 0x0000u | (0xC000u << 16) };
    const svo_ray pick = { { 0.5f, 40.0f, 0.5f }, INFINITY, { 0.0f, -1.0f, 0.0f }, 0 };

    svo_ctx *ctx = NULL;
    check(svo_create(0, 1024, &ctx), "svo_create");
    check(svo_set_buffer(ctx, desc, 1, att, 2, 0), "svo_set_buffer (terrain)");
    check(svo_set_buffer(ctx, desc, 1, att, 2, 1), "svo_set_buffer (object, offset 1)");

    svo_object ob;
    memset(&ob, 0, sizeof ob);
    ob.root = 1;
    ob.scale_log2 = -3;
    /* 90 degrees about y, row-major, world = R * object */
    const float turn[9] = { 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, -1.0f, 0.0f, 0.0f };
    memcpy(ob.rotation, turn, sizeof turn);

    int ok = 1;
    for (int f = 0; f < 5; ++f) {
        ob.position[0] = -8.0f + 4.0f * (float)f;   /* moving the object is one struct field */
        ob.position[1] = 22.0f;
        ob.position[2] = 0.0f;
        svo_hit hit, alone;
        int32_t id = 99, id_alone = 99;
        check(svo_trace_scene_host(ctx, &pick, 1, SVO_STACK_HLSL, 0, &ob, 1, &hit, NULL, NULL, &id), "svo_trace_scene_host");
        check(svo_trace_scene_host(ctx, &pick, 1, SVO_STACK_HLSL, SVO_SCENE_NO_TERRAIN, &ob, 1, &alone, NULL, NULL, &id_alone),
              "svo_trace_scene_host (no terrain)");
        const float y_hit = pick.origin[1] + hit.t / 64.0f * pick.dir[1];
        printf("frame %d: object at x = %g: picked id %d parent %u t %.9g (world y %.9g), normal (%.9g %.9g %.9g); "
               "without the terrain id %d\n", f, ob.position[0], id, hit.parent, hit.t, y_hit, hit.nx, hit.ny, hit.nz, id_alone);
        if (f == 2)
            ok = ok && id == 1 && hit.parent == 1 && (hit.flags & 1) && fabsf(hit.t - 1024.0f) < 0.01f &&
                 fabsf(y_hit - 24.0f) < 1e-3f && id_alone == 1 && alone.t == hit.t;
        else
            ok = ok && id == 0 && hit.parent == 0 && (hit.flags & 1) && fabsf(hit.t - 1536.0f) < 0.01f && id_alone == -1 &&
                 alone.parent == 0xFFFFFFFFu && alone.flags == 0;
    }

    /* the renders' list is a setting of its own: a query neither reads nor changes it */
    int n = -1;
    check(svo_set_objects(ctx, &ob, 1), "svo_set_objects");
    check(svo_get_objects(ctx, NULL, 0, &n), "svo_get_objects");
    ok = ok && n == 1;
    check(svo_set_objects(ctx, NULL, 0), "svo_set_objects (off)");

    check(svo_destroy(ctx), "svo_destroy");
    printf(ok ? "scene_min: ok\n" : "scene_min: CHECK FAILED\n");
    return ok ? 0 : 2;
}
