/*
 * closest_min.c -- closest-voxel queries from plain C (svo_closest_voxels_host, include/svo_rt.h): what a host
 * asks before it drops, pushes or steers a body -- how far is this point from the surface, and where is the
 * closest point on it?
 *
 * Scene: overlap_min.c's ball of radius 10 round the origin, voxelised here on the 16^3 grid of the world cube
 * [-16, 16]^3 (voxels of side 2; a voxel is solid when its centre lies in the ball) into a four-level pool of
 * wide nodes (svo_set_buffer_v2).  A 5 x 5 grid of points at height y = 15 is dropped onto it: the unbounded
 * query gives each point's squared distance d2 and the closest point on the nearest voxel; the host takes the
 * root.  Then four single questions:
 *   near     the grid's middle point again with a search radius of 4: nothing within it (the distance is 5)
 *   inside   the origin: d2 = 0, the point lies in or on a voxel
 *   tie      the grid's middle point has four voxels at d2 = 25: the Morton-first one answers
 *   bad      a box is no query: invalid, flag 0x10
 *
 *   gcc -O2 -Iinclude examples/closest_min.c -Lraytracingtest_amd -lsvo_rt \
 *       -L/opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/raytracingtest_amd -o closest_min
 *   ./closest_min              exit status 0 = the checks passed
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "svo_rt.h"

#define DEPTH 4
#define GRID (1 << DEPTH)
#define MAX_NODES 1024
#define SIDE 5

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
static size_t build_pool(uint64_t *nodes) {
    static int qx[MAX_NODES], qy[MAX_NODES], qz[MAX_NODES], ql[MAX_NODES];
    memset(occ, 0, sizeof occ);
    for (int z = 0; z < GRID; z++)
        for (int y = 0; y < GRID; y++)
            for (int x = 0; x < GRID; x++) {
                const float cx = 2.0f * x - 15.0f, cy = 2.0f * y - 15.0f, cz = 2.0f * z - 15.0f;
                if (cx * cx + cy * cy + cz * cz <= 100.0f)
                    for (int l = 0; l <= DEPTH; l++) {
                        const int n = 1 << l, s = DEPTH - l;
                        occ[l][((z >> s) * n + (y >> s)) * n + (x >> s)] = 1;
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

/* the same distance without a tree: the minimum over all solid voxels, with the rule's expression */
static float brute_d2(const float p[3]) {
    float best = INFINITY;
    for (int z = 0; z < GRID; z++)
        for (int y = 0; y < GRID; y++)
            for (int x = 0; x < GRID; x++) {
                if (!cell(DEPTH, x, y, z)) continue;
                const int i[3] = { x, y, z };
                float e[3];
                for (int k = 0; k < 3; k++) {
                    const float lo = 2.0f * i[k] - 16.0f, hi = lo + 2.0f;
                    const float a = lo - p[k], b = p[k] - hi, m = a > b ? a : b;
                    e[k] = m > 0.0f ? m : 0.0f;
                }
                const float d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
                if (d2 < best) best = d2;
            }
    return best;
}

int main(void) {
    static uint64_t nodes[MAX_NODES];
    static uint32_t att[2 * MAX_NODES];
    const size_t n_nodes = build_pool(nodes);
    printf("pool: %zu descriptors\n", n_nodes);

    svo_shape grid[SIDE * SIDE];
    memset(grid, 0, sizeof grid);
    for (int j = 0; j < SIDE; j++)
        for (int i = 0; i < SIDE; i++) {
            svo_shape *q = &grid[j * SIDE + i];
            q->kind = SVO_SHAPE_SPHERE;
            q->p[0] = 4.0f * (i - SIDE / 2);
            q->p[1] = 15.0f;
            q->p[2] = 4.0f * (j - SIDE / 2);
        }
    svo_closest nearest[SIDE * SIDE];
    svo_contact contacts[SIDE * SIDE];
    svo_closest_params prm;
    memset(&prm, 0, sizeof prm);
    prm.size = sizeof prm;
    prm.flags = SVO_CLOSEST_UNBOUNDED;

    svo_ctx *ctx = NULL;
    check(svo_create(0, MAX_NODES, &ctx), "svo_create");
    check(svo_set_buffer_v2(ctx, nodes, n_nodes, att, 2 * n_nodes, 0), "svo_set_buffer_v2");   /* no camera: a query needs none */
    check(svo_closest_voxels_host(ctx, grid, SIDE * SIDE, &prm, nearest, contacts), "svo_closest_voxels_host");
    int ok = 1;
    printf("distance to the ball from y = 15 (x across, z down):\n");
    for (int j = 0; j < SIDE; j++) {
        for (int i = 0; i < SIDE; i++) {
            const svo_closest *r = &nearest[j * SIDE + i];
            printf(" %6.3f", sqrtf(r->d2));
            ok = ok && r->flags == 1 && r->d2 == brute_d2(grid[j * SIDE + i].p) && contacts[j * SIDE + i].parent == r->parent;
        }
        printf("\n");
    }
    const svo_closest *mid = &nearest[(SIDE / 2) * SIDE + SIDE / 2];
    const svo_contact *c = &contacts[(SIDE / 2) * SIDE + SIDE / 2];
    printf("tie: d2 %g point (%g %g %g) visits %u flags 0x%x voxel (%llu %llu %llu) scale %u\n", mid->d2, mid->point[0],
           mid->point[1], mid->point[2], mid->visits, mid->flags, (unsigned long long)(c->key & 0x1FFFFF),
           (unsigned long long)(c->key >> 21 & 0x1FFFFF), (unsigned long long)(c->key >> 42), c->meta >> 8);
    /* four voxels round the pole share d2 = 25; the Morton-first one has the smallest z, then y, then x */
    ok = ok && mid->d2 == 25.0f && mid->point[0] == 0.0f && mid->point[1] == 10.0f && mid->point[2] == 0.0f &&
         c->key == (7ull | 12ull << 21 | 7ull << 42) && (c->meta >> 8) == 23 - DEPTH && c->meta == mid->meta;

    const svo_shape single[3] = {
        { { 0.0f, 15.0f, 0.0f }, SVO_SHAPE_SPHERE, { 4.0f, 0.0f, 0.0f }, 0 },
        { { 0.0f, 0.0f, 0.0f }, SVO_SHAPE_SPHERE, { 4.0f, 0.0f, 0.0f }, 0 },
        { { -16.0f, -16.0f, -16.0f }, SVO_SHAPE_BOX, { 16.0f, 16.0f, 16.0f }, 0 },
    };
    const char *names[3] = { "near", "inside", "bad" };
    prm.flags = 0;
    check(svo_closest_voxels_host(ctx, single, 3, &prm, nearest, NULL), "svo_closest_voxels_host (bounded)");
    for (int i = 0; i < 3; i++)
        printf("%s: d2 %g visits %u flags 0x%x\n", names[i], nearest[i].d2, nearest[i].visits, nearest[i].flags);
    ok = ok && nearest[0].flags == 0 && isinf(nearest[0].d2) && nearest[0].parent == 0xFFFFFFFFu;
    ok = ok && nearest[1].flags == 1 && nearest[1].d2 == 0.0f && nearest[1].visits == DEPTH * 8 - 7;   /* 8 voxels tie at 0: every tie is entered */
    ok = ok && nearest[2].flags == 0x10 && nearest[2].visits == 0 && isinf(nearest[2].d2);

    check(svo_destroy(ctx), "svo_destroy");
    printf(ok ? "closest_min: ok\n" : "closest_min: CHECK FAILED\n");
    return ok ? 0 : 2;
}
