/*
 * overlap_min.c -- volume queries from plain C (svo_overlap_volumes_host, include/svo_rt.h): what a host asks
 * before it moves a body -- which voxels does this box or sphere touch?
 *
 * Scene: a ball of radius 10 round the origin, voxelised here on the 16^3 grid of the world cube [-16, 16]^3
 * (voxels of side 2; a voxel is solid when its centre lies in the ball) into a four-level pool of wide nodes
 * (svo_set_buffer_v2).  Five volumes:
 *   world    the box [-16, 16]^3: touches every solid voxel
 *   origin   the sphere of radius 0 at the origin: the corner shared by the 8 voxels round it
 *   slab     the degenerate box y = 0, |x|, |z| <= 16: closed intervals, so both voxel layers next to the plane
 *   outside  the sphere of radius 1 at (14, 14, 14): beyond the ball, nothing
 *   bad      a box with p > q: invalid, flag 0x10
 *
 *   gcc -O2 -Iinclude examples/overlap_min.c -Lraytracingtest_amd -lsvo_rt \
 *       -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/raytracingtest_amd -o overlap_min
 *   ./overlap_min              exit status 0 = the checks passed
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "svo_rt.h"

#define DEPTH 4
#define GRID (1 << DEPTH)
#define MAX_NODES 1024
#define K 4

static int check(int rc, const char *what) {
    if (rc != SVO_OK) {
        fprintf(stderr, "%s failed (%d): %s\n", what, rc, svo_last_error());
        exit(1);
    }
    return rc;
}

/* occupancy of every level: occ[L] is the (2^L)^3 grid, a cell set when a solid voxel lies in it */
static unsigned char occ[DEPTH + 1][GRID * GRID * GRID];

static int cell(int level, int x, int y, int z) {
    const int n = 1 << level;
    return occ[level][(z * n + y) * n + x];
}

/* Breadth-first, so the non-leaf children of a node are consecutive: node = first << 32 | valid8 << 8 | nonleaf8,
 * slot c = the child at offset (c & 1, c >> 1 & 1, c >> 2 & 1). */
static size_t build_pool(uint64_t *nodes, int *solid) {
    static int qx[MAX_NODES], qy[MAX_NODES], qz[MAX_NODES], ql[MAX_NODES];
    memset(occ, 0, sizeof occ);
    *solid = 0;
    for (int z = 0; z < GRID; z++)
        for (int y = 0; y < GRID; y++)
            for (int x = 0; x < GRID; x++) {
                const float cx = 2.0f * x - 15.0f, cy = 2.0f * y - 15.0f, cz = 2.0f * z - 15.0f;
                if (cx * cx + cy * cy + cz * cz <= 100.0f) {
                    for (int l = 0; l <= DEPTH; l++) {
                        const int n = 1 << l, s = DEPTH - l;
                        occ[l][((z >> s) * n + (y >> s)) * n + (x >> s)] = 1;
                    }
                    *solid += 1;
                }
            }
    size_t head = 0, tail = 1;
    qx[0] = qy[0] = qz[0] = ql[0] = 0;
    while (head < tail) {
        const int x = qx[head], y = qy[head], z = qz[head], l = ql[head];
        uint32_t valid = 0, nonleaf = 0;
        const size_t first = tail;
        for (int c = 0; c < 8; c++) {
            const int jx = 2 * x + (c & 1), jy = 2 * y + (c >> 1 & 1), jz = 2 * z + (c >> 2 & 1);
            if (!cell(l + 1, jx, jy, jz)) continue;
            valid |= 1u << c;
            if (l + 1 < DEPTH) {
                if (tail >= MAX_NODES) exit(3);
                nonleaf |= 1u << c;
                qx[tail] = jx; qy[tail] = jy; qz[tail] = jz; ql[tail] = l + 1;
                tail++;
            }
        }
        nodes[head++] = (uint64_t)(nonleaf ? first : 0) << 32 | valid << 8 | nonleaf;
    }
    return tail;
}

int main(void) {
    static uint64_t nodes[MAX_NODES];
    static uint32_t att[2 * MAX_NODES];
    int solid = 0;
    const size_t n_nodes = build_pool(nodes, &solid);
    printf("pool: %zu descriptors, %d solid voxels\n", n_nodes, solid);

    const svo_shape shapes[5] = {
        { { -16.0f, -16.0f, -16.0f }, SVO_SHAPE_BOX, { 16.0f, 16.0f, 16.0f }, 0 },
        { { 0.0f, 0.0f, 0.0f }, SVO_SHAPE_SPHERE, { 0.0f, 0.0f, 0.0f }, 0 },
        { { -16.0f, 0.0f, -16.0f }, SVO_SHAPE_BOX, { 16.0f, 0.0f, 16.0f }, 0 },
        { { 14.0f, 14.0f, 14.0f }, SVO_SHAPE_SPHERE, { 1.0f, 0.0f, 0.0f }, 0 },
        { { 1.0f, 0.0f, 0.0f }, SVO_SHAPE_BOX, { 0.0f, 1.0f, 1.0f }, 0 },
    };
    const char *names[5] = { "world", "origin", "slab", "outside", "bad" };
    svo_overlap summary[5];
    svo_contact contacts[5 * K];
    svo_overlap_params prm;
    memset(&prm, 0, sizeof prm);
    prm.size = sizeof prm;
    prm.max_contacts = K;

    svo_ctx *ctx = NULL;
    check(svo_create(0, MAX_NODES, &ctx), "svo_create");
    check(svo_set_buffer_v2(ctx, nodes, n_nodes, att, 2 * n_nodes, 0), "svo_set_buffer_v2");   /* no camera: a query needs none */
    check(svo_overlap_volumes_host(ctx, shapes, 5, &prm, summary, contacts), "svo_overlap_volumes_host");
    for (int i = 0; i < 5; i++) {
        const svo_contact *c = &contacts[i * K];
        printf("%s: count %u visits %u flags 0x%x", names[i], summary[i].count, summary[i].visits, summary[i].flags);
        if (c->parent != 0xFFFFFFFFu)   /* the first voxel in Morton order, as a ray hit would name it */
            printf(" first contact: parent %u slot %u scale %u voxel (%llu %llu %llu)", c->parent, c->meta & 0xFF, c->meta >> 8,
                   (unsigned long long)(c->key & 0x1FFFFF), (unsigned long long)(c->key >> 21 & 0x1FFFFF),
                   (unsigned long long)(c->key >> 42));
        printf("\n");
    }

    /* the slab: the solid voxels of the two layers y in [-2, 0] and [0, 2], centres at y = -1 and 1 */
    int layer = 0;
    for (int z = 0; z < GRID; z++)
        for (int x = 0; x < GRID; x++) layer += cell(DEPTH, x, 7, z) + cell(DEPTH, x, 8, z);
    int ok = summary[0].count == (uint32_t)solid && summary[0].flags == 1 && summary[0].visits == n_nodes;
    ok = ok && summary[1].count == 8 && summary[1].visits == DEPTH * 8 - 7 && (contacts[K].meta >> 8) == 23 - DEPTH &&
         contacts[K].key == (7ull | 7ull << 21 | 7ull << 42);
    ok = ok && summary[2].count == (uint32_t)layer && summary[3].count == 0 && summary[3].flags == 0;
    ok = ok && summary[4].flags == 0x10 && summary[4].count == 0 && contacts[4 * K].parent == 0xFFFFFFFFu;

    /* the same question as a yes / no: SVO_OVERLAP_ANY stops at the first voxel */
    prm.flags = SVO_OVERLAP_ANY;
    prm.max_contacts = 0;
    check(svo_overlap_volumes_host(ctx, shapes, 5, &prm, summary, NULL), "svo_overlap_volumes_host (any)");
    printf("any: %u %u %u %u %u\n", summary[0].count, summary[1].count, summary[2].count, summary[3].count, summary[4].count);
    ok = ok && summary[0].count == 1 && summary[0].visits == DEPTH && summary[3].count == 0;

    check(svo_destroy(ctx), "svo_destroy");
    printf(ok ? "overlap_min: ok\n" : "overlap_min: CHECK FAILED\n");
    return ok ? 0 : 2;
}
