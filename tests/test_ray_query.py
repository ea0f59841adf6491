"""Ray queries without a GPU: the header's layout, argument rejection before any device is
touched, the numpy mirror of the classify-then-clamp rule, and the reason the clamp exists --
with it, exactly axis-aligned rays through the oracle agree with the brute-force checker;
without it they miss everything (NVIDIASVO.compute:21-24 commented out)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.query_util import axis_aligned_batch, oracle_svo, oracle_trace
from tests.test_c_host import _build

EPS = np.float32(2.0 ** -23)


@pytest.fixture(scope="module")
def native():
    from raytracingtest_amd import build
    build.build()
    from raytracingtest_amd import _lib
    return _lib.lib()


def test_query_header_layout_compiles_in_c(tmp_path):
    src = tmp_path / "q.c"
    src.write_text('#include "svo_rt.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(svo_ray) == 32, "ray");\n'
                   '_Static_assert(offsetof(svo_ray, t_max) == 12, "t_max");\n'
                   '_Static_assert(offsetof(svo_ray, dir) == 16, "dir");\n'
                   '_Static_assert(sizeof(svo_query_out) == 4 * sizeof(void *), "out");\n'
                   '_Static_assert(SVO_QUERY_ORDERED == 1 && SVO_QUERY_RAW_DIRECTIONS == 2 && '
                   'SVO_HIT_INVALID_RAY == 0x10, "enums");\n'
                   'int main(void){return 0;}\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "q")], check=True)
    from raytracingtest_amd import _lib
    assert ctypes.sizeof(_lib.SvoRay) == _lib.RAY_DTYPE.itemsize == 32
    assert _lib.RAY_DTYPE.fields["t_max"][1] == 12 and _lib.RAY_DTYPE.fields["dir"][1] == 16
    assert _lib.RAY_DTYPE.names == ("origin", "t_max", "dir", "reserved")
    assert ctypes.sizeof(_lib.SvoQueryOut) == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_query_arguments_rejected_without_gpu(native):
    """NULL context, an all-NULL out and an unknown flag bit return SVO_ERR_ARG from both entry
    points before the context is read or a device touched (the context here is no context)."""
    from raytracingtest_amd._lib import SvoQueryOut
    fake_ctx = ctypes.create_string_buffer(1 << 20)
    rays = np.zeros(4, np.dtype("V32"))
    buf = np.zeros(4 * 24, np.uint8)
    out = SvoQueryOut(buf.ctypes.data, None, None, None)
    empty = SvoQueryOut()
    ctx, r, h = ctypes.addressof(fake_ctx), rays.ctypes.data, buf.ctypes.data
    assert native.svo_trace_rays(None, r, 4, 0, 0, ctypes.byref(out), None) == -1
    assert b"null context" in native.svo_last_error()
    assert native.svo_trace_rays(ctx, r, 4, 0, 0, ctypes.byref(empty), None) == -1
    assert native.svo_trace_rays(ctx, r, 4, 0, 0, None, None) == -1
    assert native.svo_trace_rays(ctx, None, 4, 0, 0, ctypes.byref(out), None) == -1
    assert native.svo_trace_rays(ctx, r, 4, 0, 4, ctypes.byref(out), None) == -1
    assert b"flag" in native.svo_last_error()
    assert native.svo_trace_rays(ctx, r, 4, 2, 0, ctypes.byref(out), None) == -1      # stack mode
    assert native.svo_trace_rays_host(None, r, 4, 0, 0, h, None, None) == -1
    assert native.svo_trace_rays_host(ctx, r, 4, 0, 0, None, None, None) == -1
    assert native.svo_trace_rays_host(ctx, r, 4, 0, 8, h, None, None) == -1
    assert native.svo_trace_rays_host(ctx, r, 4, 7, 0, h, None, None) == -1
    assert not any(fake_ctx.raw[:4096]), "the fake context was written"


def test_sanitize_rays_classifies_then_clamps():
    from raytracingtest_amd.query import make_rays, sanitize_rays
    d = np.array([[1, 0, -0.0], [EPS, -EPS, 1], [EPS / 2, -EPS / 2, 1], [0, 0, 0], [0, -0.0, 0],
                  [np.nan, 1, 0], [1, np.inf, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1e-40, 1, 0]], np.float32)
    o = np.zeros((len(d), 3), np.float32)
    o[7, 2] = np.nan
    o[8, 0] = -np.inf
    rays = make_rays(o, d)
    rays["t_max"][9] = np.nan
    rays["t_max"][0] = 3.0
    traced, invalid = sanitize_rays(rays)
    assert invalid.tolist() == [False, False, False, True, True, True, True, True, True, True, False]
    t = traced["dir"]
    assert t[0].tolist() == [1.0, float(EPS), -float(EPS)] and np.signbit(t[0, 2])      # -0 -> -2^-23
    assert t[1].tobytes() == d[1].tobytes()                                             # 2^-23 itself untouched
    assert t[2].tolist() == [float(EPS), -float(EPS), 1.0]
    assert t[10].tolist() == [float(EPS), 1.0, float(EPS)]                              # a denormal clamps too
    assert traced["origin"].tobytes() == rays["origin"].tobytes() and traced["t_max"][0] == 3.0
    raw, invalid_raw = sanitize_rays(rays, raw=True)
    assert raw.tobytes() == rays.tobytes(), "raw=True changes nothing"
    assert invalid_raw.tolist() == invalid.tolist(), "raw=True still classifies"
    with pytest.raises(ValueError):
        make_rays(np.zeros((2, 3)), np.zeros((3, 3)))


def test_clamped_axis_aligned_rays_agree_with_bruteforce(oracle_mod, text_svo):
    """1,200 exactly axis-aligned rays on the Text fixture (six directions, origins outside and inside
    the cube, +0 and -0 zeros).  As the reference's arithmetic has them they hit nothing; through
    sanitize_rays every oracle hit is the brute force's first-hit voxel (up to ties) at its entry
    distance, every miss a brute-force miss, and at least half of the rays hit."""
    from raytracingtest_amd.query import sanitize_rays
    from tests.bruteforce import entry_exit, first_hits_compact
    rays = axis_aligned_batch()
    assert len(rays) == 1200
    assert np.all(np.count_nonzero(rays["dir"], axis=1) == 1)
    assert np.signbit(rays["dir"]).any() and (~np.signbit(rays["dir"])).any()
    osvo = oracle_svo(oracle_mod, text_svo)
    traced, invalid = sanitize_rays(rays)
    assert not invalid.any()
    hits, _, _ = oracle_trace(oracle_mod, osvo, traced)
    leaves = text_svo.leaf_voxels()
    oo = traced["origin"].astype(np.float64) / 32.0 + 1.5
    dd = traced["dir"].astype(np.float64)
    best_row, best_t, max_ov = first_hits_compact(leaves, oo, dd)
    miss = hits["parent"] == 0xFFFFFFFF
    assert not np.any(max_ov[miss] > 1e-5), "miss where the brute force crosses a voxel"
    key = {(int(r[0]), int(r[1])): i for i, r in enumerate(leaves)}
    inside = np.all(np.abs(rays["origin"]) < 16.0, axis=1)
    for i in np.flatnonzero(~miss):
        hrec = hits[i]
        row = key[(int(hrec["parent"]), int(hrec["hit_idx"]))]
        nz = np.abs(dd[i])[np.abs(dd[i]) > 0]
        tol = 1e-6 * (1.0 + 3.0 / nz.min())           # tests/test_oracle.py's tolerance
        t_in, t_out = entry_exit(leaves[row], oo[i], dd[i])
        assert t_in <= t_out + tol, f"ray {i}: hit voxel not on the ray"
        assert t_in <= best_t[i] + tol, f"ray {i}: hit voxel enters at {t_in} > {best_t[i]}"
        assert abs(hrec["t"] / 2048.0 - t_in) <= tol
        assert hrec["hit_scale"] == 23 - leaves[row, 2]
        # the ray's own axis has |d| = 1: along it the voxel's slab (grown by entry_exit's 2e-6) holds the hit
        # point to float accuracy, whatever the clamped components' huge tolerance above allows
        a = int(np.argmax(np.abs(dd[i])))
        size = 2.0 ** -float(leaves[row, 2])
        lo = 1.0 + float(leaves[row, 3 + a]) * size
        p = oo[i, a] + hrec["t"] / 2048.0 * dd[i, a]
        assert lo - 4e-6 <= p <= lo + size + 4e-6, f"ray {i}: hit point outside the voxel along the ray"
    assert np.count_nonzero(~miss) >= 600, np.count_nonzero(~miss)
    assert np.count_nonzero(~miss & inside) > 0 and np.count_nonzero(~miss & ~inside) > 0
    # the same rays as given (SVO_QUERY_RAW_DIRECTIONS): the documented unclamped behaviour
    raw, invalid_raw = sanitize_rays(rays, raw=True)
    assert not invalid_raw.any()
    raw_hits, raw_pos, raw_vox = oracle_trace(oracle_mod, osvo, raw)
    assert np.all(raw_hits["parent"] == 0xFFFFFFFF) and not np.any(raw_hits["flags"] & 1)
    assert not raw_pos.any() and np.all(raw_vox == ~np.uint64(0))


def test_csharp_shim_declares_the_ray_query():
    """unity/RaytracingMasterNative.cs (no C# toolchain here): SvoRay has the header's eight 4-byte
    fields in the header's order, and both entry points are bound."""
    text = open(os.path.join(ROOT, "unity", "RaytracingMasterNative.cs")).read()
    body = re.search(r"public struct SvoRay \{(.*?)\n    \}", text, re.S).group(1)
    fields = []
    for typ, names in re.findall(r"public (uint|int|float) ([^;]+);", body):
        fields += [(typ, n.strip()) for n in names.split(",")]
    assert [n for _, n in fields] == ["originX", "originY", "originZ", "tMax", "dirX", "dirY", "dirZ", "reserved"]
    assert [t for t, _ in fields] == ["float"] * 7 + ["uint"]
    for name in ("svo_trace_rays", "svo_trace_rays_host"):
        assert re.search(rf"static extern int {name}\(", text), name
    assert re.search(r"public bool Raycast\(Vector3 origin, Vector3 direction, float maxDistance, out SvoHit hit, "
                     r"out Vector3 point\)", text)


def test_c_raycast_host_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path, os.path.join(ROOT, "examples", "raycast_min.c"), "raycast_min"))
