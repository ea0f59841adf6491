"""Level of detail without a GPU: the numpy tracer (tests/lod_tracer.py) pinned to the CPU oracle
where the oracle can speak -- LOD off, and the depth clamp against the unmodified oracle on a pruned
pool -- the distance-dependent inputs the GPU tests reuse shown not to be vacuous, and the API's
surface: exports, argument rejection, the header in C, the C# shim, pixel_footprint."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingtest_amd.camera import main_camera
from raytracingtest_amd.query import sanitize_rays
from tests import lod_tracer
from tests.conftest import ROOT
from tests.lod_util import CLAMP_K, DISTANCE, clamp_pair, is_inner, pools, pruned
from tests.query_util import oracle_svo, oracle_trace, random_batch


@pytest.fixture(scope="module")
def rays():
    traced, invalid = sanitize_rays(random_batch())
    assert len(traced) == 4133 and not invalid.any()
    return traced


@pytest.fixture(scope="module")
def both(text_svo):
    return pools(text_svo)


def _same(res, hits, vox, what):
    """Tracer result against oracle hit records: parent, hit_idx, hit_scale, t, and the voxel key."""
    hit = (hits["flags"] & 1) != 0
    bad = np.flatnonzero((res["hit"] != hit) | (res["parent"] != hits["parent"]) | (res["hit_idx"] != hits["hit_idx"]) |
                         (res["scale"] != hits["hit_scale"]) | (res["t"].view(np.uint32) != hits["t"].view(np.uint32)) |
                         (res["key"] != vox))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(hit)} rays differ, first {bad[:8].tolist()}"
    return int(hit.sum())


@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_tracer_equals_oracle_with_lod_off(oracle_mod, both, rays, pool):
    """(0, 0): byte for byte the oracle's parent, hit_idx, hit_scale and t, both stack modes."""
    svo = both[pool]
    osvo = oracle_svo(oracle_mod, svo)
    for mode in (0, 1):
        hits, _, vox = oracle_trace(oracle_mod, osvo, rays, mode)
        n = _same(lod_tracer.trace(svo, rays["origin"], rays["dir"], mode), hits, vox, f"{pool} mode {mode}")
        assert n >= (1000 if pool == "text" else 500), n


@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_depth_clamp_equals_oracle_on_pruned_pool(oracle_mod, both, rays, pool):
    """(0, 2^-k) on the full pool = the unmodified oracle on the pool whose descriptors at level >= k
    have no non-leaf bits; every hit is on an inner voxel of the full pool."""
    svo = both[pool]
    k = CLAMP_K[pool]
    cut = pruned(svo, k)
    assert cut.attachments.tobytes() == svo.attachments.tobytes() and len(cut) == len(svo)
    osvo = oracle_svo(oracle_mod, cut)
    coef, bias = clamp_pair(pool)
    for mode in (0, 1):
        hits, _, vox = oracle_trace(oracle_mod, osvo, rays, mode)
        res = lod_tracer.trace(svo, rays["origin"], rays["dir"], mode, coef, bias)
        n = _same(res, hits, vox, f"{pool} clamp {k} mode {mode}")
        assert n >= 2000, n
        assert np.all(res["scale"][res["hit"]] >= 23 - k)
        assert np.array_equal(is_inner(svo, res["parent"], res["hit_idx"], res["hit"]), res["hit"])


def test_distance_dependent_inputs_are_not_vacuous(both, rays):
    """The pairs the GPU tests trace: hits on inner voxels AND at leaf scale, at several scales."""
    for pool, inner_min in (("text", 1000), ("tree7", 500)):
        svo = both[pool]
        coef, bias = DISTANCE[pool]
        res = lod_tracer.trace(svo, rays["origin"], rays["dir"], 1, coef, bias)
        inner = is_inner(svo, res["parent"], res["hit_idx"], res["hit"])
        scales = np.unique(res["scale"][res["hit"]])
        print(pool, "hits", int(res["hit"].sum()), "inner", int(inner.sum()), "scales", scales.tolist())
        assert inner.sum() >= inner_min
        assert (res["hit"] & ~inner).sum() >= 100, "no hits left at leaf scale"
        if pool == "text":
            assert len(scales) >= 3


# ------------------------------------------------------------------ the API's surface
@pytest.fixture(scope="module")
def native():
    from raytracingtest_amd import build
    build.build()
    from raytracingtest_amd import _lib
    return _lib.lib()


LOD_FUNCS = ("svo_set_lod", "svo_get_lod", "svo_trace_rays_lod", "svo_trace_rays_lod_host")


def test_exports_present(native):
    from raytracingtest_amd import _lib
    header = open(os.path.join(ROOT, "include", "svo_rt.h")).read()
    for name in LOD_FUNCS:
        assert name in _lib.EXPORTS and hasattr(native, name)
        assert re.search(rf"\bint {name}\(", header), name
    assert native.svo_abi_version() == 10


def test_lod_arguments_rejected_without_gpu(native):
    """NULL context and negative, NaN and infinite numbers return SVO_ERR_ARG before the context is
    read or a device touched (the context here is no context); so does everything svo_trace_rays rejects."""
    from raytracingtest_amd._lib import SvoQueryOut
    fake_ctx = ctypes.create_string_buffer(1 << 20)
    rays = np.zeros(4, np.dtype("V32"))
    buf = np.zeros(4 * 24, np.uint8)
    out = SvoQueryOut(buf.ctypes.data, None, None, None)
    empty = SvoQueryOut()
    ctx, r, h = ctypes.addressof(fake_ctx), rays.ctypes.data, buf.ctypes.data
    bad_pairs = [(-1.0, 0.0), (0.0, -2.0 ** -10), (float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0),
                 (0.0, float("inf")), (-float("inf"), 0.0)]
    assert native.svo_set_lod(None, 0.01, 0.0) == -1
    assert b"null context" in native.svo_last_error()
    assert native.svo_get_lod(None, None, None) == -1
    for c, b in bad_pairs:
        assert native.svo_set_lod(ctx, c, b) == -1, (c, b)
        assert b"ray_size" in native.svo_last_error()
        assert native.svo_trace_rays_lod(ctx, r, 4, 0, 0, c, b, ctypes.byref(out), None) == -1, (c, b)
        assert native.svo_trace_rays_lod_host(ctx, r, 4, 0, 0, c, b, h, None, None) == -1, (c, b)
    assert native.svo_trace_rays_lod(None, r, 4, 0, 0, 0.01, 0.0, ctypes.byref(out), None) == -1
    assert native.svo_trace_rays_lod(ctx, r, 4, 0, 0, 0.01, 0.0, ctypes.byref(empty), None) == -1
    assert native.svo_trace_rays_lod(ctx, r, 4, 0, 0, 0.01, 0.0, None, None) == -1
    assert native.svo_trace_rays_lod(ctx, None, 4, 0, 0, 0.01, 0.0, ctypes.byref(out), None) == -1
    assert native.svo_trace_rays_lod(ctx, r, 4, 0, 4, 0.01, 0.0, ctypes.byref(out), None) == -1
    assert b"flag" in native.svo_last_error()
    assert native.svo_trace_rays_lod(ctx, r, 4, 2, 0, 0.01, 0.0, ctypes.byref(out), None) == -1
    assert native.svo_trace_rays_lod_host(None, r, 4, 0, 0, 0.01, 0.0, h, None, None) == -1
    assert native.svo_trace_rays_lod_host(ctx, r, 4, 0, 0, 0.01, 0.0, None, None, None) == -1
    assert native.svo_trace_rays_lod_host(ctx, r, 4, 0, 8, 0.01, 0.0, h, None, None) == -1
    assert native.svo_trace_rays_lod_host(ctx, r, 4, 7, 0, 0.01, 0.0, h, None, None) == -1
    assert not any(fake_ctx.raw[:4096]), "the fake context was written"


def test_lod_header_compiles_in_c(tmp_path):
    src = tmp_path / "l.c"
    src.write_text('#include "svo_rt.h"\n'
                   'int (*a)(svo_ctx *, float, float) = svo_set_lod;\n'
                   'int (*b)(svo_ctx *, float *, float *) = svo_get_lod;\n'
                   'int (*c)(svo_ctx *, const svo_ray *, size_t, int, uint32_t, float, float, const svo_query_out *, void *)'
                   ' = svo_trace_rays_lod;\n'
                   'int (*d)(svo_ctx *, const svo_ray *, size_t, int, uint32_t, float, float, svo_hit *, float *, uint64_t *)'
                   ' = svo_trace_rays_lod_host;\n'
                   '_Static_assert(sizeof(svo_config) == 132, "svo_config stays 132 bytes");\n'
                   '_Static_assert(sizeof(svo_ray) == 32 && sizeof(svo_hit) == 24, "records");\n'
                   'int main(void){return 0;}\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "l.o")], check=True)


def test_csharp_shim_declares_lod():
    text = open(os.path.join(ROOT, "unity", "RaytracingMasterNative.cs")).read()
    for name in LOD_FUNCS:
        assert re.search(rf"static extern int {name}\(", text), name
    assert re.search(r"public float lodPixels\b", text)
    assert re.search(r"svo_set_lod\(_ctx,", text), "the parameter update does not set the pair"


def test_pixel_footprint_formula():
    from raytracingtest_amd.lod import pixel_footprint
    for w, h in ((1920, 1080), (256, 128)):
        _, inv_proj = main_camera().uniforms(w, h)
        m = abs(float(np.asarray(inv_proj)[1][1]))
        assert m > 0
        assert pixel_footprint(inv_proj, h) == 2.0 * m / h
        assert pixel_footprint(inv_proj, h, pixels=8) == 8.0 * 2.0 * m / h
    # the centre pixel's rays one pixel apart: their unit directions differ by about the footprint
    cam = main_camera()
    c2w, inv_proj = cam.uniforms(256, 128)
    ip = np.asarray(inv_proj, np.float64)
    def ray(y):
        v = (y + 0.5) / 128 * 2 - 1
        d = ip @ np.array([0.0, v, 0.0, 1.0])
        return d[:3] / np.linalg.norm(d[:3])
    assert abs(np.linalg.norm(ray(64) - ray(63)) - pixel_footprint(inv_proj, 128)) < 1e-3 * pixel_footprint(inv_proj, 128)


def test_lod_hit_is_inner_reads_the_pool(both):
    from raytracingtest_amd import HIT_DTYPE
    from raytracingtest_amd.lod import lod_hit_is_inner
    svo = both["text"]
    lo, _ = svo.masks_and_first()
    nl_all, leaf_all = lo & 0xFF, ((lo >> 8) & 0xFF) & ~(lo & 0xFF)
    a, b = int(np.flatnonzero(nl_all != 0)[-1]), int(np.flatnonzero(leaf_all != 0)[0])   # a node with an inner / a leaf child
    inner_slot = [c for c in range(8) if (int(nl_all[a]) >> c) & 1][-1]
    leaf_slot = [c for c in range(8) if (int(leaf_all[b]) >> c) & 1][-1]
    h = np.zeros(3, HIT_DTYPE)
    h["parent"] = (a, b, 0xFFFFFFFF)
    h["hit_idx"] = (inner_slot, leaf_slot, 0)
    h["flags"] = (1, 1, 0)
    assert lod_hit_is_inner(svo, h).tolist() == [True, False, False]
    c = np.zeros(3, np.dtype([("parent", "<u4"), ("meta", "<u4"), ("t", "<f4")]))
    c["parent"] = h["parent"]
    c["meta"] = h["hit_idx"].astype(np.uint32) | (h["flags"].astype(np.uint32) << 16)
    assert lod_hit_is_inner(svo, c).tolist() == [True, False, False]


def test_lod_floor_rule(tmp_path):
    """svo_lod.h lod_floor on a CPU (a plain C++ program that includes only that header).  s_min =
    2^-depth.  -inf: bias >= 2 s_min, sqrt(3) coef >= 1, or T' <= 0; +inf: coef == 0 otherwise; else
    T' (1 - 2^-10) rounded down to f32, T' = ((2 s_min - bias) / coef)(1 - sqrt(3) coef) - sqrt(3) bias."""
    import shutil
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lod_floor")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "raytracingtest_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lod_floor_driver.cpp"), "-o", exe], check=True)
    cases = [(0.0, 0.125, 4, -np.inf),      # bias = 2 s_min = 0.125
             (0.0, 0.0625, 4, np.inf),      # a depth clamp finer than 2 s_min
             (0.25, 0.125, 4, -np.inf),     # bias = 2 s_min with a coefficient
             (0.6, 0.0, 4, -np.inf),        # sqrt(3) 0.6 = 1.04 >= 1
             (0.5, 0.1, 4, -np.inf),        # T' = 0.05 x 0.134 - 0.173 < 0
             (0.25, 0.0, 3, None),          # T' = (0.25 / 0.25)(1 - 0.4330127) = 0.5669873
             (1.0 / 64.0, 0.0, 7, None),    # T' = (2^-6 / 2^-6)(1 - 0.0270633) = 0.9729367
             (0.0436, 2.0 ** -9, 5, None)]
    args = [str(v) for c in cases for v in c[:3]]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(cases)
    for (coef, bias, depth, want), got in zip(cases, out):
        got = np.float32(got)
        if want is not None:
            assert got == want, (coef, bias, depth, got)
            continue
        t = ((2.0 * 2.0 ** -depth - bias) / coef) * (1.0 - np.sqrt(3.0) * coef) - np.sqrt(3.0) * bias
        fl = t * (1.0 - 2.0 ** -10)
        assert float(got) <= fl < float(np.nextafter(got, np.float32(np.inf))), (coef, bias, depth, got, fl)
        assert 0.0 < float(got) < t
    assert abs(float(np.float32(out[5])) - 0.5669873 * (1 - 2.0 ** -10)) < 1e-6
    assert abs(float(np.float32(out[6])) - 0.9729367 * (1 - 2.0 ** -10)) < 1e-6
