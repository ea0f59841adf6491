"""A numpy float32 restatement of the reference's IntersectSVO
(Assets/Shaders/NVIDIASVO.compute:12-198) WITH the level-of-detail line the reference keeps
commented out (:77-79), vectorised over rays: one IEEE rounding per operation, no FMA.

TEST INFRASTRUCTURE ONLY.  It shares no code with the product (the HIP kernels) or with the C
oracle (oracle/svo_oracle.c); it exists because the oracle has no LOD line and stays as it is.

The LOD test sits where this project specifies it (INTEGRATION.md "Level of detail"): on a valid
child the walk would enter (`t_min <= min(t_max, tc_max)`, :75 and :90), before the leaf test (:93):

    small  <=>  fl(fl(tc_max * ray_size_coef) + ray_size_bias) >= scale_exp2

A small child ends the walk exactly as a leaf does.  (0, 0) never fires: scale_exp2 > 0.

Both stack modes: 0 = the HLSL stack, whose int2 entry is written through a float2
(`stack[scale] = float2((int)parent, asint(t_max))`, :98 -- both words are rounded to f32 and
converted back, round toward zero, saturating), 1 = the exact stack.

Rays are world-space origins and directions, used as given (svo_trace_rays' rays after its clamp,
or the camera rays of a frame).  Returns per ray: hit, parent, hit_idx, scale, t (= 2048 t_min,
the record's distance), voxel (the un-mirrored integer voxel coordinates at the hit scale, [n, 3])
and key (the 63-bit voxel key of svo_rt.h built from them); misses: parent 0xFFFFFFFF, t inf,
key all ones.
"""
import numpy as np

S_MAX = 23
MAX_ITERS = 65536
F32 = np.float32


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.int32)


def _float(x):
    return np.ascontiguousarray(x, np.int32).view(F32)


def _hlsl_round_trip(v):
    """int <- float <- int of an int32 array: (int)(float)v, toward zero, saturating."""
    f = v.astype(np.int32).astype(F32)            # round to nearest even, like the GPU's convert
    d = f.astype(np.float64)
    out = np.trunc(d)
    out = np.where(d >= 2147483648.0, 2147483647.0, out)
    out = np.where(d <= -2147483648.0, -2147483648.0, out)
    return out.astype(np.int64).astype(np.int32)


def _popcount7(x):
    x = (x & 0x7F).astype(np.int64)
    return sum((x >> k) & 1 for k in range(7))


def ray_setup(o, d):
    """The ray setup (:15-43) of n rays, origins o and directions d [n, 3] float32, one IEEE rounding
    per operation: (org, coef, bias, octant, t_min, t_max) -- the SVO-space origin, the t
    coefficients and biases per axis (lists of three [n] arrays), the octant mask and the cube's
    entry (clamped at 0) and exit.  Shared with tests/placement_model.py (the query keys)."""
    n = len(o)
    two, three, zero = F32(2.0), F32(3.0), F32(0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # :15-19
        org = [o[:, k] * F32(1.0 / 32.0) + F32(1.5) for k in range(3)]
        # :27-38
        coef = [F32(1.0) / -np.abs(d[:, k]) for k in range(3)]
        bias = [coef[k] * org[k] for k in range(3)]
        octant = np.full(n, 7, np.int32)
        for k in range(3):
            p = d[:, k] > zero
            octant = np.where(p, octant ^ (1 << k), octant)
            bias[k] = np.where(p, three * coef[k] - bias[k], bias[k])
        # :40-43 (HLSL min / max: a NaN operand gives the other one)
        t_min = np.fmax(np.fmax(two * coef[0] - bias[0], two * coef[1] - bias[1]), two * coef[2] - bias[2])
        t_max = np.fmin(np.fmin(coef[0] - bias[0], coef[1] - bias[1]), coef[2] - bias[2])
        t_min = np.fmax(t_min, zero)
    return org, coef, bias, octant, t_min, t_max


def trace(svo, origins, dirs, mode=0, ray_size_coef=0.0, ray_size_bias=0.0):
    lo, first = svo.masks_and_first()
    lo = lo.astype(np.int64)
    first = first.astype(np.int64)
    o = np.asarray(origins, F32).reshape(-1, 3)
    d = np.asarray(dirs, F32).reshape(-1, 3)
    n = len(o)
    coef_l, bias_l = F32(ray_size_coef), F32(ray_size_bias)
    half_c, two, three, zero = F32(0.5), F32(2.0), F32(3.0), F32(0.0)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        org, coef, bias, octant, t_min, t_max = ray_setup(o, d)
        h = t_max.copy()
        # :46-54
        parent = np.zeros(n, np.int64)
        idx = np.zeros(n, np.int32)
        pos = [np.full(n, F32(1.0), F32) for _ in range(3)]
        scale = np.full(n, S_MAX - 1, np.int32)
        scale_exp2 = np.full(n, half_c, F32)
        for k in range(3):
            c = (F32(1.5) * coef[k] - bias[k]) > t_min
            idx = np.where(c, idx ^ (1 << k), idx)
            pos[k] = np.where(c, F32(1.5), pos[k])

        stack_p = np.zeros((n, 32), np.int32)     # never-written entries read as zero
        stack_t = np.zeros((n, 32), np.int32)
        rows = np.arange(n)
        active = np.ones(n, bool)
        hit = np.zeros(n, bool)
        it = 0
        while active.any():
            it += 1
            assert it <= MAX_ITERS, "iteration cap reached (not a tree of at most 22 levels?)"
            a = active
            # :60-62 -- an index outside the pool reads as 0 (only inactive lanes here)
            inside = (parent >= 0) & (parent < len(lo))
            pc = np.where(inside, parent, 0)
            cd = np.where(inside, lo[pc], 0)
            fc = np.where(inside, first[pc], 0)
            # :66-69
            corner = [pos[k] * coef[k] - bias[k] for k in range(3)]
            tc_max = np.fmin(np.fmin(corner[0], corner[1]), corner[2])
            # :73-75
            child_masks = cd << (idx ^ octant).astype(np.int64)
            valid = ((child_masks & 0x8000) != 0) & (t_min <= t_max)
            # :83-90
            tv_max = np.fmin(t_max, tc_max)
            half = scale_exp2 * half_c
            center = [half * coef[k] + corner[k] for k in range(3)]
            descend = a & valid & (t_min <= tv_max)
            # the LOD line: two roundings, an ordered compare (NaN: false)
            small = (tc_max * coef_l + bias_l) >= scale_exp2
            # :93-94
            leaf = (child_masks & 0x0080) == 0
            hit_now = descend & (leaf | small)
            hit |= hit_now
            push = descend & ~hit_now
            # :97-98
            store = push & (tc_max < h)
            if store.any():
                r, s = rows[store], scale[store]
                sp = parent[store].astype(np.int32)
                st = _bits(t_max[store])
                if mode == 0:
                    sp, st = _hlsl_round_trip(sp), _hlsl_round_trip(st)
                stack_p[r, s] = sp
                stack_t[r, s] = st
            h = np.where(push, tc_max, h)
            # :101-105
            parent = np.where(push, fc + _popcount7(child_masks), parent)
            # :107-114
            idx = np.where(push, 0, idx)
            scale = np.where(push, scale - 1, scale)
            scale_exp2 = np.where(push, half, scale_exp2)
            for k in range(3):
                c = push & (center[k] > t_min)
                idx = np.where(c, idx ^ (1 << k), idx)
                pos[k] = np.where(c, pos[k] + scale_exp2, pos[k])
            t_max = np.where(push, tv_max, t_max)
            # :122-128
            adv = a & ~descend
            step = np.zeros(n, np.int32)
            for k in range(3):
                c = adv & (corner[k] <= tc_max)
                step = np.where(c, step ^ (1 << k), step)
                pos[k] = np.where(c, pos[k] - scale_exp2, pos[k])
            t_min = np.where(adv, tc_max, t_min)
            idx = np.where(adv, idx ^ step, idx)
            # :130-154
            pop = adv & ((idx & step) != 0)
            if pop.any():
                diff = np.zeros(n, np.int32)
                for k in range(3):
                    c = pop & ((step & (1 << k)) != 0)
                    diff = np.where(c, diff | (_bits(pos[k]) ^ _bits(pos[k] + scale_exp2)), diff)
                new_scale = (_bits(diff.view(np.uint32).astype(F32)) >> 23) - 127
                scale = np.where(pop, new_scale, scale)
                scale_exp2 = np.where(pop, _float((scale - S_MAX + 127) << 23), scale_exp2)
                sc = scale & 31
                parent = np.where(pop, stack_p[rows, sc].view(np.uint32).astype(np.int64), parent)
                t_max = np.where(pop, _float(stack_t[rows, sc]), t_max)
                for k in range(3):
                    sh = _bits(pos[k]) >> sc
                    pos[k] = np.where(pop, _float(sh << sc), pos[k])
                sh = [_bits(pos[k]) >> sc for k in range(3)]
                idx = np.where(pop, (sh[0] & 1) | ((sh[1] & 1) << 1) | ((sh[2] & 1) << 2), idx)
                h = np.where(pop, zero, h)
            active = a & ~hit & (scale < S_MAX)

        hit &= scale < S_MAX
        # :163-171
        t = (t_min * F32(32.0)) * F32(64.0)
        # :166-168, and the integer voxel coordinates: the un-mirrored corner's mantissa at the hit scale
        vox = np.zeros((n, 3), np.int64)
        key = np.zeros(n, np.uint64)
        sc = np.where(hit, scale, 0)
        for k in range(3):
            q = np.where((octant >> k) & 1 == 0, (three - scale_exp2) - pos[k], pos[k])
            vox[:, k] = (_bits(q).astype(np.int64) & 0x7FFFFF) >> sc
            key |= vox[:, k].astype(np.uint64) << np.uint64(21 * k)
    miss = ~hit
    vox[miss] = -1
    return {"hit": hit,
            "parent": np.where(hit, parent, 0xFFFFFFFF).astype(np.uint32),
            "hit_idx": np.where(hit, idx ^ octant ^ 7, 0).astype(np.uint8),
            "scale": np.where(hit, scale, 0).astype(np.uint8),
            "t": np.where(hit, t, F32(np.inf)).astype(F32),
            "voxel": vox,
            "key": np.where(hit, key, ~np.uint64(0)).astype(np.uint64)}


def compact_bytes(res):
    """The 12-byte compact records (svo_hit_compact) of a trace: parent, hit_idx | scale << 8 |
    flags << 16 (bit 0 on a hit), t."""
    n = len(res["hit"])
    rec = np.zeros((n, 3), np.uint32)
    rec[:, 0] = res["parent"]
    rec[:, 1] = res["hit_idx"].astype(np.uint32) | (res["scale"].astype(np.uint32) << 8) | (res["hit"].astype(np.uint32) << 16)
    rec[:, 2] = res["t"].view(np.uint32)
    return rec
