"""The ambient term without a GPU: the API's surface, the direction tables, the rule's header
(csrc/svo_ambient.h, built by plain g++ into tests/ambient_driver.cpp) against its numpy statement
(ambient.ambient_rays), and the expected-frame builder the GPU tests compare renders with
(tests/ambient_util.py), with conditions on its inputs so that no test passes on a degenerate frame."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingtest_amd import HIT_DTYPE, ambient
from raytracingtest_amd._lib import RAY_DTYPE
from raytracingtest_amd.reflection import dead_rays
from tests import ambient_util as au
from tests import reflect_util as ru
from tests.conftest import ROOT
from tests.lod_util import pools
from tests.test_reflection import hand_cases

FUNCS = ("svo_set_ambient", "svo_get_ambient", "svo_ambient_rays", "svo_ambient_rays_host")


@pytest.fixture(scope="module")
def both(text_svo):
    return pools(text_svo)


@pytest.fixture(scope="module")
def native():
    from raytracingtest_amd import build
    build.build()
    from raytracingtest_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ 1. the surface
def test_exports_present(native):
    from raytracingtest_amd import _lib
    header = open(os.path.join(ROOT, "include", "svo_rt.h")).read()
    for name in FUNCS:
        assert name in _lib.EXPORTS and hasattr(native, name)
        assert re.search(rf"\bint {name}\(", header), name
    assert re.search(r"enum \{ SVO_AMBIENT_MAX_RAYS = 16 \};", header)
    assert native.svo_abi_version() == 10


def test_header_compiles_in_c(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "svo_rt.h"\n'
                   'int (*a)(svo_ctx *, const float *, int, float, uint32_t) = svo_set_ambient;\n'
                   'int (*b)(svo_ctx *, float *, int *, float *, uint32_t *) = svo_get_ambient;\n'
                   'int (*c)(svo_ctx *, const svo_ray *, size_t, uint32_t, const svo_hit *, const uint64_t *, int, float,'
                   ' uint32_t, svo_ray *, void *) = svo_ambient_rays;\n'
                   'int (*d)(svo_ctx *, const svo_ray *, size_t, uint32_t, const svo_hit *, const uint64_t *, int, float,'
                   ' uint32_t, svo_ray *) = svo_ambient_rays_host;\n'
                   '_Static_assert(SVO_AMBIENT_MAX_RAYS == 16, "the largest table");\n'
                   '_Static_assert(sizeof(svo_config) == 132, "svo_config stays 132 bytes");\n'
                   'int main(void){return 0;}\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "a.o")], check=True)


def test_bindings_declare_ambient():
    from raytracingtest_amd import RaytracingMaster
    for name in ("SetAmbient", "GetAmbient", "AmbientRays", "ambient_rays_device"):
        assert callable(getattr(RaytracingMaster, name))
    text = open(os.path.join(ROOT, "unity", "RaytracingMasterNative.cs")).read()
    for name in FUNCS:
        assert re.search(rf"\[DllImport\(Lib\)\] public static extern int {name}\(", text), name
    assert re.search(r"public Vector3 ambient;", text)
    assert re.search(r"public int ambientRays;", text)
    assert re.search(r"public float ambientRadius", text)
    assert re.search(r"svo_set_ambient\(_ctx,[^;]*ambientRays", text)
    for field in ("ambient", "ambientRays", "ambientRadius"):
        assert re.search(rf"{field} != _{field}Set[^}}]*_currentSample = 0;", text, re.S), field


def test_arguments_rejected_without_gpu(native):
    """Every argument error comes back as SVO_ERR_ARG before the context is read or a device touched (the
    context here is no context, and must stay unwritten)."""
    fake_ctx = ctypes.create_string_buffer(1 << 20)
    ctx = ctypes.addressof(fake_ctx)
    f3 = ctypes.c_float * 3
    inf, nan = float("inf"), float("nan")
    assert native.svo_set_ambient(None, f3(0.5, 0.5, 0.5), 4, inf, 0) == -1
    assert b"null context" in native.svo_last_error()
    assert native.svo_get_ambient(None, None, None, None, None) == -1
    for bad in (-0.1, 4.5, nan, inf, -inf):
        for k in range(3):
            a = [0.5, 0.5, 0.5]
            a[k] = bad
            assert native.svo_set_ambient(ctx, f3(*a), 4, inf, 0) == -1, (bad, k)
            assert b"ambient" in native.svo_last_error()
    for bad in (1, 3, 5, 32, -1):
        assert native.svo_set_ambient(ctx, f3(0.5, 0.5, 0.5), bad, inf, 0) == -1, bad
        assert b"n_rays" in native.svo_last_error()
    for bad in (0.0, -1.0, nan, -inf):
        for n in (0, 4):
            assert native.svo_set_ambient(ctx, f3(0.5, 0.5, 0.5), n, bad, 0) == -1, bad
            assert b"radius" in native.svo_last_error()
    for bad in (8, 9, 1 << 31):
        assert native.svo_set_ambient(ctx, f3(0.5, 0.5, 0.5), 4, 1.0, bad) == -1
        assert b"variant" in native.svo_last_error()
    assert native.svo_set_ambient(ctx, None, 3, inf, 0) == -1   # a NULL colour excuses no other argument
    rays = np.zeros(4, RAY_DTYPE)
    hits = np.zeros(4, HIT_DTYPE)
    vox = np.zeros(4, np.uint64)
    out = np.zeros(4 * 16, RAY_DTYPE)
    r, h, v, o = rays.ctypes.data, hits.ctypes.data, vox.ctypes.data, out.ctypes.data
    for fn, tail in ((native.svo_ambient_rays, (None,)), (native.svo_ambient_rays_host, ())):
        def call(ctx_, r_, n_, fl_, h_, v_, nr_, rad_, var_, o_):
            return fn(ctx_, r_, n_, fl_, h_, v_, nr_, rad_, var_, o_, *tail)
        assert call(None, r, 4, 0, h, v, 4, inf, 0, o) == -1
        assert call(ctx, None, 4, 0, h, v, 4, inf, 0, o) == -1
        assert call(ctx, r, 4, 0, None, v, 4, inf, 0, o) == -1
        assert call(ctx, r, 4, 0, h, None, 4, inf, 0, o) == -1
        assert call(ctx, r, 4, 0, h, v, 4, inf, 0, None) == -1
        for flags in (1, 4, 3, 0x80000000):   # SVO_QUERY_ORDERED is not a flag of this call
            assert call(ctx, r, 4, flags, h, v, 4, inf, 0, o) == -1, flags
            assert b"flag" in native.svo_last_error()
        for bad in (0, 1, 3, 5, 32, -1):
            assert call(ctx, r, 4, 0, h, v, bad, inf, 0, o) == -1, bad
            assert b"n_rays" in native.svo_last_error()
        for bad in (0.0, -1.0, nan, -inf):
            assert call(ctx, r, 4, 0, h, v, 4, bad, 0, o) == -1, bad
        assert call(ctx, r, 4, 0, h, v, 4, inf, 8, o) == -1
        # n * n_rays <= 2^31 - 1
        assert call(ctx, r, (1 << 31) // 4, 0, h, v, 4, inf, 0, o) == -1
        assert b"2^31" in native.svo_last_error()
        assert call(ctx, r, 1 << 27, 0, h, v, 16, inf, 0, o) == -1
        # the output overlaps an input: the rays themselves, their tail, the records, the keys
        big = np.zeros(4 * 16 + 4, RAY_DTYPE)
        b0 = big.ctypes.data
        assert call(ctx, b0, 4, 0, h, v, 16, inf, 0, b0) == -1
        assert b"overlap" in native.svo_last_error()
        assert call(ctx, b0 + 32 * 3, 4, 0, h, v, 4, inf, 0, b0) == -1          # input inside the output
        assert call(ctx, b0, 4, 0, h, v, 4, inf, 0, b0 + 32 * 3) == -1          # output starts in the input
        assert call(ctx, r, 4, 0, b0 + 64, v, 4, inf, 0, b0) == -1
        assert call(ctx, r, 4, 0, h, b0 + 16 * 32 - 8, 4, inf, 0, b0) == -1
        assert call(ctx, r, 0, 2, h, v, 4, inf, 0, o) == 0   # nothing to do: no device touched
    assert not any(fake_ctx.raw[:4096]), "the fake context was written"
    assert rays.tobytes() == bytes(4 * 32) and out.tobytes() == bytes(64 * 32)


# ------------------------------------------------------------------ 2. the tables
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ambient") / "ambient_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "ambient_driver.cpp"), "-o", str(exe)], check=True)

    def tables():
        dst = exe.parent / "tables.bin"
        subprocess.run([str(exe), "tables", str(dst)], check=True)
        return np.fromfile(dst, np.float32).reshape(-1, 3)

    def run(rays, hits, voxel, raw, n_rays, radius, variant):
        n = len(rays)
        rec = np.zeros((n, 64), np.uint8)
        rec[:, :32] = np.ascontiguousarray(rays, RAY_DTYPE).view(np.uint8).reshape(n, 32)
        rec[:, 32:56] = np.ascontiguousarray(hits, HIT_DTYPE).view(np.uint8).reshape(n, 24)
        rec[:, 56:] = np.ascontiguousarray(voxel, np.uint64).view(np.uint8).reshape(n, 8)
        src, dst = exe.parent / "in.bin", exe.parent / "out.bin"
        rec.tofile(src)
        bits = int(np.float32(radius).view(np.uint32))
        subprocess.run([str(exe), "rays", str(src), str(dst), "1" if raw else "0", str(n_rays), f"{bits:x}", str(variant)],
                       check=True)
        return np.fromfile(dst, RAY_DTYPE)
    run.tables = tables
    return run


def test_tables(driver):
    """The header's 28 triples are the truth: Python holds the same bits, the formula gives them within
    1 f32 ulp (libm), and the facts the rule leans on hold."""
    got = driver.tables()
    assert got.shape == (28, 3)
    want = np.concatenate([ambient.TABLES[n] for n in (4, 8, 16)])
    assert got.tobytes() == want.tobytes(), "csrc/svo_ambient.h and ambient.TABLES differ"
    for n in (4, 8, 16):
        t = ambient.TABLES[n]
        assert t.dtype == np.float32 and t.shape == (n, 3)
        ulps = np.abs(t.view(np.int32).astype(np.int64) - ambient.formula_table(n).view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (n, ulps.max())
        assert np.abs(t).min() >= 2.0 ** -10    # the query's clamp (2^-23) never changes a direction
        assert (t[:, 2] > 0).all()
        pairs = set()
        for v in range(8):
            tv = ambient.variant_table(n, v)
            assert tv[:, 2].tobytes() == t[:, 2].tobytes()
            assert np.array_equal(np.sort(np.abs(tv[:, :2]), axis=1), np.sort(np.abs(t[:, :2]), axis=1))   # exact
            pairs |= {(a.tobytes(), b.tobytes()) for a, b in tv[:, :2]}
        assert len(pairs) == 8 * n, (n, len(pairs))
        length = np.sqrt((t.astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(length - 1.0).max() < 1e-6
    assert float(np.abs(ambient.TABLES[16]).min()) == pytest.approx(0.01506, abs=1e-5)
    with pytest.raises(ValueError):
        ambient.variant_table(5, 0)
    with pytest.raises(ValueError):
        ambient.variant_table(4, 8)


# ------------------------------------------------------------------ 3. the rule: header against numpy
@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_header_equals_numpy_on_primary_hits(oracle_mod, both, driver, pool):
    """The oracle's primary hits at 200 x 120, Main camera: all three N, all 8 variants, raw and clamped."""
    w, h = ru.SIZES["raster"]
    prim = ru.primary(oracle_mod, pool, both[pool], "main", w, h)
    px = prim["px"]
    rays, hits, vox = prim["rays"], prim["hits"][px], prim["voxel"][px]
    assert len(px) >= 1000   # thousands of hits on every face orientation the pose shows
    total = 0
    for n_rays, radius in ((4, 1.0), (8, np.inf), (16, 4.0)):
        for variant in range(8):
            for raw in (True, False):
                want = ambient.ambient_rays(rays, hits, vox, n_rays, radius, variant, raw=raw)
                got = driver(rays, hits, vox, raw, n_rays, radius, variant)
                assert got.tobytes() == want.tobytes(), f"{pool} N {n_rays} variant {variant} raw {raw}"
                total += len(got)
    want = ambient.ambient_rays(rays, hits, vox, 4, 1.0, 0, raw=True).reshape(-1, 4)
    # every ray of a pixel shares its origin, leaves through the entry face, and is a table row permuted
    assert (want["origin"] == want["origin"][:, :1]).all() and (want["t_max"] == np.float32(1.0)).all()
    assert np.array_equal(np.sort(np.abs(want["dir"][0]), axis=1), np.sort(np.abs(ambient.TABLES[4]), axis=1))
    print(pool, "ambient rays compared:", total)


def test_header_equals_numpy_on_hand_cases(driver):
    """tests/test_reflection.py's hand cases (signed zeros, NaN face times, origins inside the voxel, a
    miss, an invalid-ray record, a component the clamp moves): misses give dead rays for every k."""
    rays, hits, vox = hand_cases()
    dead = dead_rays(1).tobytes()
    for n_rays in (4, 8, 16):
        for variant in (0, 3, 5):
            for raw in (False, True):
                want = ambient.ambient_rays(rays, hits, vox, n_rays, 2.5, variant, raw=raw)
                got = driver(rays, hits, vox, raw, n_rays, 2.5, variant)
                assert got.tobytes() == want.tobytes(), (n_rays, variant, raw)
                want = want.reshape(len(rays), n_rays)
                for i in (6, 7):
                    assert all(want[i, k].tobytes() == dead for k in range(n_rays))
                assert not any(want[0, k].tobytes() == dead for k in range(n_rays))
    r4 = ambient.ambient_rays(rays, hits, vox, 4, 2.5, 0, raw=True).reshape(len(rays), 4)
    t = ambient.TABLES[4]
    # case 0: +0 on axis 1 makes it the entry axis, out = +1: dir = (b, c, a); the origin steps off y = hi
    assert r4["dir"][0].tobytes() == np.stack([t[:, 1], t[:, 2], t[:, 0]], axis=1).tobytes()
    assert r4["origin"][0, 0, 1] == np.float32(1.0 + 2.0 ** -6)
    # case 1: entry through x = lo, out = -1: dir = (-c, a, b)
    assert r4["dir"][1].tobytes() == np.stack([-t[:, 2], t[:, 0], t[:, 1]], axis=1).tobytes()
    with pytest.raises(ValueError):
        ambient.ambient_rays(rays, hits, vox, 4, 0.0, 0)


# ------------------------------------------------------------------ 4. the expected-frame builder
def test_builder_off_is_the_oracle_frame(oracle_mod, both):
    w, h = ru.SIZES["raster"]
    prim = ru.primary(oracle_mod, "tree7", both["tree7"], "main", w, h)
    for amb, n in (((0.0, 0.0, 0.0), 4), (au.AMBIENT, 0)):
        got = au.expected_frame(oracle_mod, "tree7", both["tree7"], "main", w, h, 0, amb, n)
        assert got.tobytes() == prim["rgba"].tobytes()


@pytest.mark.parametrize("case", list(au.CASES))
def test_builder_frames_are_not_degenerate(oracle_mod, both, case):
    """Conditions on the GPU tests' frames, on the reference alone: open and occluded rays both occur, and
    most hit pixels have some of each."""
    pool, (w, h), n_rays, radius, variant = au.CASES[case]
    tr = au.traced(oracle_mod, pool, both[pool], "main", w, h, 0, n_rays, radius, variant)
    share, some = au.open_share(tr)
    print(case, "hit pixels", len(tr["prim"]["px"]), "open share", round(share, 3), "some but not all", round(some, 3),
          "rays hitting at t = 0", tr["t0"])
    frame = au.expected_frame(oracle_mod, pool, both[pool], "main", w, h, 0, au.AMBIENT, n_rays, radius, variant)
    prim = tr["prim"]
    px = prim["px"]
    miss = np.ones(w * h, bool)
    miss[px] = False
    assert frame[miss].tobytes() == prim["rgba"][miss].tobytes() and np.all(frame[:, 3] == 1.0)
    if pool == "text":
        assert 0.3 <= share <= 0.9
        assert some >= 0.5
        # the fixture has no colour: albedo 0, so the term adds nothing and the frame stays the oracle's
        assert not tr["albedo"].any() and frame.tobytes() == prim["rgba"].tobytes()
    else:
        assert 0.3 <= share <= 0.95
        assert some >= 0.4
        changed = (frame[px, :3] != prim["rgba"][px, :3]).any(axis=1)
        assert changed.mean() >= 0.9
        assert (frame[px, :3] >= prim["rgba"][px, :3]).all()   # light is only added
        # pixels that differ only in which rays are open get different colours: the fold is visible
        assert len(np.unique(tr["open"], axis=0)) >= min(2 ** n_rays, 12)


@pytest.mark.parametrize("frame", [(200, 120, 4, 0.64), (256, 128, 8, 0.69), (64, 40, 16, 0.67)])
def test_text_open_share_at_radius_one(oracle_mod, both, frame):
    """`text`, Main, radius 1.0, variant 0: the open shares measured when the rule was written (0.64, 0.69,
    0.67), within [0.3, 0.9], and at least half of the hit pixels have some but not all rays open."""
    w, h, n_rays, measured = frame
    share, some = au.open_share(au.traced(oracle_mod, "text", both["text"], "main", w, h, 0, n_rays, 1.0, 0))
    print(frame, "open share", round(share, 4), "some but not all", round(some, 4))
    assert 0.3 <= share <= 0.9 and abs(share - measured) < 0.01
    assert some >= 0.5


def test_text_pool_is_closed_to_infinite_rays(oracle_mod, both):
    """Why the `text` cases use a finite radius: with radius = inf no ambient ray of the Text fixture escapes."""
    w, h = 64, 40
    tr = au.traced(oracle_mod, "text", both["text"], "main", w, h, 0, 4, np.inf, 0)
    assert au.open_share(tr)[0] == 0.0
    frame = au.expected_frame(oracle_mod, "text", both["text"], "main", w, h, 0, au.AMBIENT, 4, np.inf, 0)
    assert frame.tobytes() == tr["prim"]["rgba"].tobytes()


def test_builder_with_shadows_lights_black_pixels(oracle_mod, both):
    pool, (w, h), n_rays, radius, variant = au.CASES["tree7_raster"]
    off = ru.primary(oracle_mod, pool, both[pool], "main", w, h, oracle_mod.SHADOW_RAYS)
    plain = ru.primary(oracle_mod, pool, both[pool], "main", w, h)
    px = off["px"]
    assert ((off["hits"]["flags"][px] & 8) != 0).sum() >= 100 and not (plain["hits"]["flags"] & 8).any()
    frame = au.expected_frame(oracle_mod, pool, both[pool], "main", w, h, 0, au.AMBIENT, n_rays, radius, variant, shadows=True)
    black = (off["rgba"][px, :3] == 0).all(axis=1)
    lit = black & (frame[px, :3] != 0).any(axis=1)
    print("tree7 200x120 with shadows: black hit pixels", int(black.sum()), "of them lit by the ambient term", int(lit.sum()))
    assert lit.sum() >= 100
    # a shadowed pixel keeps the ambient term alone; every other hit pixel is what it is without shadows
    sh = (off["hits"]["flags"][px] & 8) != 0
    no_sh = au.expected_frame(oracle_mod, pool, both[pool], "main", w, h, 0, au.AMBIENT, n_rays, radius, variant)
    assert (frame[px][~sh, :3] == no_sh[px][~sh, :3]).all()
    assert (frame[px][sh, :3] <= no_sh[px][sh, :3]).all()
