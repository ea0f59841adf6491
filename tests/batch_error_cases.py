"""The fixed table of wrong calls behind tests/golden/batch_errors.json: every ray-batch entry point of the C API
(svo_trace_rays .. svo_sample_sky and their _host twins) with arguments that end in an argument error, in the
n == 0 early return or, for the four calls that need a node pool, in the "no node pool" state error a zeroed
context gives before any device is selected.  No call of the table reaches a device, so the pairs (return code,
svo_last_error text) are the same on every machine.

tests/golden/make_batch_errors.py records the pairs; tests/test_batch_errors.py replays the table and compares.

What a zeroed context cannot show is left out: the "d_rays must be 16-byte aligned" test of svo_trace_rays and
svo_trace_scene stands behind the pool test, and a host call of bounce, object rays or the sky sampler with
exactly 2^31 - 1 entries passes every check and would select a device.
"""
import ctypes

import numpy as np

from raytracingtest_amd._lib import LIGHT_DTYPE, OBJECT_DTYPE, SvoQueryOut

ORDERED, RAW, NO_TERRAIN = 1, 2, 4
LIMIT = (1 << 31) - 1
NAN, INF = float("nan"), float("inf")

# byte offsets into the zeroed arena the calls' pointers aim at (n = 4 where a count is valid)
RAYS, HITS, VOX, POS, IDS, MASK, OUT, BIG = 0, 1024, 2048, 3072, 4096, 4608, 8192, 16384
ARENA_BYTES = 32768


class Memory:
    """What the calls point at: the fake context (a megabyte of zeros), the arena, light and object lists."""

    def __init__(self):
        self.fake_ctx = ctypes.create_string_buffer(1 << 20)
        self.ctx = ctypes.addressof(self.fake_ctx)
        raw = np.zeros(ARENA_BYTES + 64, np.uint8)
        skip = -raw.ctypes.data % 64
        self.arena = raw[skip:skip + ARENA_BYTES]
        self.base = self.arena.ctypes.data
        lights = np.zeros(8, LIGHT_DTYPE)
        lights["position"] = [(0.5 + j, 6.75, 8.25) for j in range(8)]
        lights["range"] = 24.0
        lights["colour"] = (3.0, 2.5, 2.0)
        self.lights = lights
        self.bad_light = lights[:2].copy()
        self.bad_light["range"][1] = 0.0
        objects = np.zeros(2, OBJECT_DTYPE)
        objects["rotation"] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
        objects["position"] = [(1.0, 2.0, 3.0), (-4.0, 0.0, 8.0)]
        objects["scale_log2"] = (0, -2)
        self.objects = objects
        self.bad_object = objects.copy()
        self.bad_object["scale_log2"][1] = 9
        self.lists = {"lights": self.lights, "bad_light": self.bad_light, "objects": self.objects,
                      "bad_object": self.bad_object}
        self.before = {k: v.tobytes() for k, v in self.lists.items()}

    def at(self, offset):
        return self.base + offset

    def unwritten(self):
        return (bytes(self.fake_ctx) == bytes(1 << 20) and not self.arena.any()
                and all(v.tobytes() == self.before[k] for k, v in self.lists.items()))


def _family(fn, names, good, cases):
    """[(id, fn, args)]: `good` with each case's overrides, in the order of `names`."""
    out = []
    for label, change in cases:
        unknown = set(change) - set(names)
        assert not unknown, (fn, label, unknown)
        args = dict(good, **change)
        out.append((f"{fn}: {label}", fn, [args[k] for k in names]))
    return out


def _nulls(names):
    return [(f"null {k}", {k: None}) for k in names]


def table(m):
    """Every case as (id, function name, argument list); an "out" argument is a tuple of the four svo_query_out
    pointers (None: a NULL struct)."""
    a = m.at
    L, O = m.lists["lights"].ctypes.data, m.lists["objects"].ctypes.data
    bad_l, bad_o = m.lists["bad_light"].ctypes.data, m.lists["bad_object"].ctypes.data
    t = []

    # ---- svo_trace_rays, svo_trace_rays_lod and their host twins
    for lod in (False, True):
        for host in (False, True):
            fn = "svo_trace_rays" + ("_lod" if lod else "") + ("_host" if host else "")
            names = ["ctx", "rays", "n", "mode", "flags"] + (["coef", "bias"] if lod else [])
            good = dict(ctx=m.ctx, rays=a(RAYS), n=4, mode=0, flags=0, coef=0.5, bias=0.25)
            if host:
                names += ["hits", "pos", "vox"]
                good.update(hits=a(HITS), pos=a(POS), vox=a(VOX))
                no_out = dict(hits=None, pos=None, vox=None)
            else:
                names += ["out", "stream"]
                good.update(out=(a(HITS), a(POS), a(VOX), a(MASK)), stream=None)
                no_out = dict(out=(None, None, None, None))
            cases = _nulls(["ctx", "rays"]) + [("every output null", no_out)]
            if not host:
                cases += [("null svo_query_out", dict(out=None)), ("only the hit mask", dict(out=(None, None, None, a(MASK)))),
                          ("misaligned rays, no pool", dict(rays=a(RAYS + 4)))]
            else:
                cases += [("only positions", dict(hits=None, vox=None))]
            cases += [(f"flag bits {f:#x}", dict(flags=f)) for f in (4, 8, 0x80000000, 7)]
            cases += [(f"stack mode {s}", dict(mode=s)) for s in (2, -1)]
            cases += [("2^31 rays", dict(n=LIMIT + 1)), ("2^31 - 1 rays, no pool", dict(n=LIMIT)),
                      ("ordered and raw, no pool", dict(flags=ORDERED | RAW)),
                      ("no rays", dict(n=0, flags=ORDERED | RAW)), ("no rays, stack mode 1", dict(n=0, mode=1)),
                      ("null ctx and null rays", dict(ctx=None, rays=None)),
                      ("null rays and bad flag", dict(rays=None, flags=4)),
                      ("every output null and bad flag", dict(no_out, flags=8)),
                      ("bad flag and bad stack mode", dict(flags=4, mode=2)),
                      ("bad stack mode and too many rays", dict(mode=3, n=LIMIT + 1)),
                      ("no rays and bad stack mode", dict(n=0, mode=2))]
            if lod:
                cases += [(f"lod pair {c}, {b}", dict(coef=c, bias=b))
                          for c, b in ((NAN, 0.0), (-1.0, 0.0), (INF, 0.0), (0.0, NAN), (0.0, -0.5), (0.0, INF))]
                cases += [("lod pair -0, -0, no pool", dict(coef=-0.0, bias=-0.0)),
                          ("null ctx and bad lod pair", dict(ctx=None, coef=NAN)),
                          ("bad lod pair and null rays", dict(coef=-1.0, rays=None)),
                          ("bad lod pair and no rays", dict(bias=NAN, n=0))]
            t += _family(fn, names, good, cases)

    # ---- the calls on a traced batch: bounce, ambient, light rays
    align = [("misaligned rays", dict(rays=a(RAYS + 4))), ("rays on 8 bytes", dict(rays=a(RAYS + 8))),
             ("misaligned output", dict(out=a(OUT + 8))), ("misaligned hits", dict(hits=a(HITS + 4))),
             ("misaligned voxel keys", dict(vox=a(VOX + 4))),
             ("misaligned rays and hits", dict(rays=a(RAYS + 4), hits=a(HITS + 4)))]
    bad_flags = [(f"flag bits {f:#x}", dict(flags=f)) for f in (ORDERED, 4, 0x80000000, ORDERED | RAW)]
    batch = ["ctx", "rays", "n", "flags", "hits", "vox"]
    batch_good = dict(ctx=m.ctx, rays=a(RAYS), n=4, flags=0, hits=a(HITS), vox=a(VOX), out=a(OUT), stream=None)
    overlaps = [("output over the rays", dict(rays=a(BIG), out=a(BIG))),
                ("rays inside the output", dict(rays=a(BIG + 32 * 3), out=a(BIG))),
                ("output starts in the rays", dict(rays=a(BIG), out=a(BIG + 32 * 3))),
                ("hits inside the output", dict(hits=a(BIG + 64), out=a(BIG))),
                ("voxel keys at the output's end", dict(vox=a(BIG + 8 * 32 - 8), out=a(BIG)))]
    for host in (False, True):
        tail = [] if host else ["stream"]
        dev = (lambda cases: []) if host else (lambda cases: cases)

        fn = "svo_bounce_rays" + ("_host" if host else "")
        names = batch + ["out"] + tail
        cases = _nulls(["ctx", "rays", "hits", "vox", "out"]) + bad_flags + dev(align)
        cases += [("2^31 rays", dict(n=LIMIT + 1)), ("no rays", dict(n=0, flags=RAW)),
                  ("in place, no rays", dict(out=a(RAYS), n=0)),
                  ("null ctx and null rays", dict(ctx=None, rays=None)),
                  ("null hits and bad flag", dict(hits=None, flags=4)),
                  ("null output and too many rays", dict(out=None, n=LIMIT + 1)),
                  ("bad flag and too many rays", dict(flags=ORDERED, n=LIMIT + 1))]
        cases += dev([("2^31 - 1 rays, misaligned", dict(n=LIMIT, rays=a(RAYS + 4))),
                      ("in place, misaligned hits", dict(out=a(RAYS), hits=a(HITS + 4))),
                      ("in place and misaligned", dict(rays=a(RAYS + 8), out=a(RAYS + 8))),
                      ("too many rays and misaligned", dict(n=LIMIT + 1, rays=a(RAYS + 4))),
                      ("misaligned voxel keys and no rays", dict(vox=a(VOX + 4), n=0))])
        t += _family(fn, names, batch_good, cases)

        fn = "svo_ambient_rays" + ("_host" if host else "")
        names = batch + ["n_rays", "radius", "variant", "out"] + tail
        good = dict(batch_good, n_rays=4, radius=INF, variant=0)
        cases = _nulls(["ctx", "rays", "hits", "vox", "out"]) + bad_flags + dev(align) + overlaps
        cases += [(f"n_rays {k}", dict(n_rays=k)) for k in (0, -1, 5, 17)]
        cases += [(f"radius {r}", dict(radius=r)) for r in (0.0, -1.0, NAN, -INF)]
        cases += [("variant 8", dict(variant=8)), ("variant 2^31", dict(variant=1 << 31))]
        for fan in (4, 16):
            cases += [(f"one past the limit, fan {fan}", dict(n=LIMIT // fan + 1, n_rays=fan)),
                      (f"at the limit, fan {fan}, output over the rays",
                       dict(n=LIMIT // fan, n_rays=fan, rays=a(BIG), out=a(BIG)))]
        cases += [("no rays", dict(n=0, flags=RAW, n_rays=16, radius=2.5, variant=7)),
                  ("no rays, in place", dict(n=0, out=a(RAYS))),
                  ("null voxel keys and bad flag", dict(vox=None, flags=4)),
                  ("bad flag and bad n_rays", dict(flags=ORDERED, n_rays=3)),
                  ("bad n_rays and bad radius", dict(n_rays=3, radius=0.0)),
                  ("bad radius and bad variant", dict(radius=NAN, variant=9)),
                  ("bad n_rays and too many rays", dict(n_rays=0, n=LIMIT)),
                  ("bad variant and too many rays", dict(variant=8, n=LIMIT)),
                  ("too many rays and an overlap", dict(n=LIMIT // 4 + 1, rays=a(BIG), out=a(BIG)))]
        cases += dev([("an overlap and misaligned", dict(rays=a(BIG + 4), out=a(BIG))),
                      ("too many rays and misaligned", dict(n=LIMIT, hits=a(HITS + 4)))])
        t += _family(fn, names, good, cases)

        fn = "svo_light_rays" + ("_host" if host else "")
        names = batch + ["lights", "n_lights", "out"] + tail
        good = dict(batch_good, lights=L, n_lights=2)
        cases = _nulls(["ctx", "rays", "hits", "vox", "lights", "out"]) + bad_flags + dev(align) + overlaps
        cases += [(f"n_lights {k}", dict(n_lights=k)) for k in (0, -1, 9, 1 << 20)]
        cases += [("a bad light", dict(lights=bad_l))]
        for fan in (2, 8):
            cases += [(f"one past the limit, fan {fan}", dict(n=LIMIT // fan + 1, n_lights=fan)),
                      (f"at the limit, fan {fan}, output over the rays",
                       dict(n=LIMIT // fan, n_lights=fan, rays=a(BIG), out=a(BIG)))]
        cases += [("no rays", dict(n=0, flags=RAW, n_lights=8)),
                  ("null hits and bad flag", dict(hits=None, flags=ORDERED)),
                  ("bad flag and null lights", dict(flags=4, lights=None)),
                  ("null lights and bad n_lights", dict(lights=None, n_lights=0)),
                  ("a bad light and too many rays", dict(lights=bad_l, n=LIMIT)),
                  ("bad n_lights and too many rays", dict(n_lights=9, n=LIMIT)),
                  ("a bad light and no rays", dict(lights=bad_l, n=0)),
                  ("too many rays and an overlap", dict(n=LIMIT // 2 + 1, rays=a(BIG), out=a(BIG)))]
        cases += dev([("an overlap and misaligned", dict(rays=a(BIG + 4), out=a(BIG))),
                      ("too many rays and misaligned", dict(n=LIMIT, vox=a(VOX + 4)))])
        t += _family(fn, names, good, cases)

        # ---- object rays
        fn = "svo_object_rays" + ("_host" if host else "")
        names = ["ctx", "rays", "n", "flags", "object", "out"] + tail
        good = dict(ctx=m.ctx, rays=a(RAYS), n=4, flags=0, object=O, out=a(OUT), stream=None)
        cases = _nulls(["ctx", "rays", "object", "out"]) + bad_flags
        cases += [("a bad object", dict(object=bad_o + 64)), ("2^31 rays", dict(n=LIMIT + 1)),
                  ("no rays", dict(n=0, flags=RAW)), ("in place, no rays", dict(out=a(RAYS), n=0)),
                  ("null rays and null output", dict(rays=None, out=None)),
                  ("null output and null object", dict(out=None, object=None)),
                  ("null object and bad flag", dict(object=None, flags=4)),
                  ("bad flag and a bad object", dict(flags=ORDERED, object=bad_o + 64)),
                  ("a bad object and too many rays", dict(object=bad_o + 64, n=LIMIT + 1))]
        cases += dev([("misaligned rays", dict(rays=a(RAYS + 4))), ("rays on 8 bytes", dict(rays=a(RAYS + 8))),
                      ("misaligned output", dict(out=a(OUT + 8))),
                      ("2^31 - 1 rays, misaligned", dict(n=LIMIT, out=a(OUT + 4))),
                      ("in place and misaligned", dict(rays=a(RAYS + 8), out=a(RAYS + 8))),
                      ("too many rays and misaligned", dict(n=LIMIT + 1, rays=a(RAYS + 4))),
                      ("misaligned and no rays", dict(rays=a(RAYS + 4), n=0))])
        t += _family(fn, names, good, cases)

        # ---- scene queries
        fn = "svo_trace_scene" + ("_host" if host else "")
        names = ["ctx", "rays", "n", "mode", "flags", "objects", "n_objects"]
        good = dict(ctx=m.ctx, rays=a(RAYS), n=4, mode=0, flags=0, objects=None, n_objects=0)
        if host:
            names += ["hits", "pos", "vox", "ids"]
            good.update(hits=a(HITS), pos=a(POS), vox=a(VOX), ids=a(IDS))
            no_out = dict(hits=None, pos=None, vox=None, ids=None)
            only_ids = dict(hits=None, pos=None, vox=None)
        else:
            names += ["out", "ids", "stream"]
            good.update(out=(a(HITS), a(POS), a(VOX), a(MASK)), ids=a(IDS), stream=None)
            no_out = dict(out=(None, None, None, None), ids=None)
            only_ids = dict(out=None)
        cases = _nulls(["ctx", "rays"]) + [("every output null", no_out), ("only the ids, no pool", only_ids)]
        if not host:
            cases += [("null svo_query_out and no ids", dict(out=None, ids=None)),
                      ("misaligned rays, no pool", dict(rays=a(RAYS + 4)))]
        cases += [(f"flag bits {f:#x}", dict(flags=f)) for f in (ORDERED, 8, 0x80000000, ORDERED | RAW, ORDERED | 8)]
        cases += [(f"stack mode {s}", dict(mode=s)) for s in (2, -1)]
        cases += [("2^31 rays", dict(n=LIMIT + 1)), ("2^31 - 1 rays, null object list", dict(n=LIMIT, n_objects=1)),
                  ("2^31 - 1 rays, no pool", dict(n=LIMIT)), ("raw, no terrain, no pool", dict(flags=RAW | NO_TERRAIN)),
                  ("null object list", dict(n_objects=1)), ("a bad object", dict(objects=bad_o, n_objects=2)),
                  ("a root outside the capacity", dict(objects=O, n_objects=2))]
        cases += [(f"n_objects {k}", dict(objects=O, n_objects=k)) for k in (-1, 9)]
        cases += [("n_objects -1, null list", dict(n_objects=-1)), ("n_objects 9, null list", dict(n_objects=9)),
                  ("no rays", dict(n=0, flags=RAW | NO_TERRAIN, mode=1)),
                  ("no rays, a root outside the capacity", dict(n=0, objects=O, n_objects=1)),
                  ("null rays and every output null", dict(no_out, rays=None)),
                  ("every output null and ordered", dict(no_out, flags=ORDERED)),
                  ("bad flag and bad stack mode", dict(flags=8, mode=2)),
                  ("bad stack mode and too many rays", dict(mode=2, n=LIMIT + 1)),
                  ("too many rays and a bad object", dict(n=LIMIT + 1, objects=bad_o, n_objects=2)),
                  ("a bad object and a root outside the capacity", dict(objects=bad_o, n_objects=2, n=0))]
        t += _family(fn, names, good, cases)

        # ---- the sky sampler
        fn = "svo_sample_sky" + ("_host" if host else "")
        names = ["ctx", "dirs", "n", "rgba"] + tail
        good = dict(ctx=m.ctx, dirs=a(RAYS), n=4, rgba=a(OUT), stream=None)
        cases = _nulls(["ctx", "dirs", "rgba"])
        cases += [("2^31 directions", dict(n=LIMIT + 1)), ("no directions", dict(n=0)),
                  ("in place, no directions", dict(rgba=a(RAYS), n=0)),
                  ("null ctx and null directions", dict(ctx=None, dirs=None)),
                  ("null directions and null colours", dict(dirs=None, rgba=None)),
                  ("null colours and too many directions", dict(rgba=None, n=LIMIT + 1))]
        cases += dev([("misaligned directions", dict(dirs=a(RAYS + 4))), ("directions on 8 bytes", dict(dirs=a(RAYS + 8))),
                      ("misaligned colours", dict(rgba=a(OUT + 8))),
                      ("2^31 - 1 directions, misaligned", dict(n=LIMIT, dirs=a(RAYS + 4))),
                      ("too many directions and misaligned", dict(n=LIMIT + 1, rgba=a(OUT + 4))),
                      ("misaligned and no directions", dict(dirs=a(RAYS + 4), n=0))])
        t += _family(fn, names, good, cases)

    ids = [c[0] for c in t]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return t


def run(native, m):
    """[(id, return code, svo_last_error text or None)] of the whole table against the loaded library.  The text
    is read only after a failure: a success leaves the previous call's text behind."""
    results = []
    for ident, fn, args in table(m):
        keep = []
        call = []
        for v in args:
            if isinstance(v, tuple):   # the four pointers of a svo_query_out
                keep.append(SvoQueryOut(*v))
                v = ctypes.byref(keep[-1])
            call.append(v)
        rc = getattr(native, fn)(*call)
        results.append((ident, int(rc), native.svo_last_error().decode() if rc else None))
    return results
