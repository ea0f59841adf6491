"""Level of detail on the GPU (svo_set_lod, svo_trace_rays_lod): every comparison is byte equality.

References: for the depth clamp (0, 2^-k) the unmodified CPU oracle on the pruned pool (every
output); for distance-dependent pairs the numpy tracer (tests/lod_tracer.py, pinned to the oracle by
tests/test_lod.py) on the compact records, hit masks and voxel keys, and svo_assemble_frame's rebuild
of the frame's own compact records for hit records, Result and display words.

Frames use pixel_footprint(..., pixels=8), chosen so that small frames reach inner voxels (8, not 4 or 16:
the tracer alone reaches the 10 % of inner hit pixels on the overview pose with it): at these sizes (256 x 128 and
200 x 120, wide field of view) that makes EVERY hit pixel an inner voxel on both poses (checked with the
tracer alone first: 1,762 - 32,768 inner hits of as many), so the policy and entry-point tests also
trace pixels=2 on the depth-7 tree from the Main pose, where inner and leaf-scale hits mix
(8,784 inner of 12,087 hits at 256 x 128, scales 16 - 18)."""
import ctypes

import numpy as np
import pytest

from raytracingtest_amd import HIT_DTYPE, RaytracingMaster, SvoError
from raytracingtest_amd import _lib
from raytracingtest_amd._lib import COMPACT_DTYPE
from raytracingtest_amd.camera import main_camera, main_light, overview_camera
from raytracingtest_amd.lod import lod_hit_is_inner, pixel_footprint
from tests import lod_tracer
from tests.lod_util import CLAMP_K, DISTANCE, clamp_pair, hits_compact, pools, pruned, tracer_expected
from tests.query_util import expected, oracle_svo, pack_mask, random_batch

pytestmark = pytest.mark.gpu

PAD = 64
ITEM = {"hits": 24, "position": 16, "voxel": 8, "hitmask": 8}
CAMS = {"main": main_camera, "overview": overview_camera}
SIZES = {"raster": (200, 120), "strips": (256, 128)}   # 25 tile columns: the raster path; 32: XCD strips


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def both(text_svo):
    return pools(text_svo)


@pytest.fixture(scope="module")
def rays():
    return random_batch()


@pytest.fixture(scope="module")
def masters(torch, both):
    ms = {}
    for name, svo in both.items():
        ms[name] = RaytracingMaster(device=0, capacity_nodes=1 << 16)
        ms[name].SetSVOBuffer(svo)
    yield ms
    for m in ms.values():
        m.close()


# ---------------------------------------------------------------------------- queries
def trace(torch, m, rays, mode=0, ordered=False, lod=None, stream=None):
    """One device query into 0xEE-filled buffers with PAD spare entries each (checked untouched)."""
    n = len(rays)
    count = {k: (n + 63) // 64 if k == "hitmask" else n for k in ITEM}
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    bufs = {k: torch.full(((count[k] + PAD) * ITEM[k],), 0xEE, dtype=torch.uint8, device="cuda") for k in ITEM}
    torch.cuda.synchronize()
    m.trace_rays_device(d_rays.data_ptr(), n, stack_mode=mode, ordered=ordered, lod=lod,
                        stream=None if stream is None else stream.cuda_stream, **{k: v.data_ptr() for k, v in bufs.items()})
    torch.cuda.synchronize()
    out = {}
    for k, v in bufs.items():
        a = v.cpu().numpy()
        assert np.all(a[count[k] * ITEM[k]:] == 0xEE), f"{k}: written past its {count[k]} entries"
        out[k] = a[:count[k] * ITEM[k]]
    return out


@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_query_depth_clamp_equals_oracle_on_pruned_pool(torch, oracle_mod, both, masters, rays, pool):
    """(0, 2^-k): every output of svo_trace_rays_lod is the unmodified oracle's on the pruned pool."""
    osvo = oracle_svo(oracle_mod, pruned(both[pool], CLAMP_K[pool]))
    for mode in (0, 1):
        exp = expected(oracle_mod, osvo, rays, mode)
        assert np.count_nonzero(exp["hits"]["flags"] & 1) >= 2000
        for ordered in (False, True):
            got = trace(torch, masters[pool], rays, mode, ordered, lod=clamp_pair(pool))
            for k in ITEM:
                assert got[k].tobytes() == np.ascontiguousarray(exp[k]).tobytes(), f"{pool} mode {mode} ordered {ordered}: {k}"


@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_query_distance_pair_equals_tracer(torch, both, masters, rays, pool):
    """(1/16, 0) on Text and (1/64, 0) on the tree: compact bytes, hit mask and voxel keys are the tracer's."""
    svo = both[pool]
    coef, bias = DISTANCE[pool]
    for mode in (0, 1):
        exp = tracer_expected(svo, rays, mode, coef, bias)
        for ordered in (False, True):
            got = trace(torch, masters[pool], rays, mode, ordered, lod=(coef, bias))
            hits = got["hits"].view(HIT_DTYPE)
            bad = np.flatnonzero((hits_compact(hits) != exp["compact"]).any(axis=1))
            assert len(bad) == 0, f"{pool} mode {mode} ordered {ordered}: {len(bad)} records differ, first {bad[:8].tolist()}"
            assert got["hitmask"].tobytes() == exp["hitmask"].tobytes()
            assert np.array_equal(got["voxel"].view("<u8"), exp["voxel"])
            inner = lod_hit_is_inner(svo, hits)
            assert inner.sum() >= (1000 if pool == "text" else 500) and (exp["hit"] & ~inner).sum() >= 100


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pool", ["text_fetch_all_0", "cyclic7"])
def test_query_under_the_plain_and_guarded_loops(torch, oracle_mod, both, rays, pool, mode):
    """svo_trace_rays_lod under the two loops the tests above do not take.  fetch_all 0: the depth clamp on
    Text, as above.  The guarded loop: the cyclic pool of tests/guard_pools.py with the pair (0, 2^-24) -- no
    voxel is that small, so the footprint test never holds and every output is the oracle's own, rays that
    end on the overflow rule included."""
    from raytracingtest_amd.svo_data import SVOData
    from tests import guard_pools as gp
    if pool == "cyclic7":
        nodes, att = gp.cyclic7()
        svo, config, pair = SVOData(nodes=nodes, attachments=att), {}, (0.0, 2.0 ** -24)
        exp = expected(oracle_mod, gp.oracle_svo(oracle_mod, "cyclic7"), rays, mode)
        assert np.count_nonzero(exp["hits"]["flags"] & gp.FLAG_OVERFLOW) >= 100
    else:
        svo, config, pair = both["text"], {"fetch_all": 0}, clamp_pair("text")
        exp = expected(oracle_mod, oracle_svo(oracle_mod, pruned(svo, CLAMP_K["text"])), rays, mode)
    assert np.count_nonzero(exp["hits"]["flags"] & 1) >= 1000
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16, config=config)
    try:
        m.SetSVOBuffer(svo)
        got = trace(torch, m, rays, mode, lod=pair)
        for k in ITEM:
            assert got[k].tobytes() == np.ascontiguousarray(exp[k]).tobytes(), f"{pool} mode {mode}: {k}"
    finally:
        m.close()


def test_query_lod_off_is_trace_rays(torch, masters, rays):
    """(0, 0): byte-identical to svo_trace_rays, device and host path."""
    m = masters["text"]
    for mode, ordered in ((0, False), (1, True)):
        plain = trace(torch, m, rays, mode, ordered)
        off = trace(torch, m, rays, mode, ordered, lod=(0.0, 0.0))
        for k in ITEM:
            assert plain[k].tobytes() == off[k].tobytes(), k
    a = m.TraceRays(rays, want_position=True, want_voxel=True)
    b = m.TraceRays(rays, want_position=True, want_voxel=True, lod=(0.0, 0.0))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = m.TraceRays(rays, lod=DISTANCE["text"])
    assert c.tobytes() == trace(torch, m, rays, lod=DISTANCE["text"])["hits"].tobytes() != a[0].tobytes()


def test_query_between_renders_leaves_renders_and_pair_alone(torch, both, masters, rays):
    m = masters["text"]
    w, h = 200, 120
    _, inv_proj = main_camera().uniforms(w, h)
    pair = (np.float32(pixel_footprint(inv_proj, h, 8)), np.float32(2.0 ** -9))
    try:
        m.SetLod(*pair)
        assert m.GetLod() == (float(pair[0]), float(pair[1]))
        m.UpdateShaderParameters(main_camera(), w, h)
        m.Render(w, h)
        rgba2, hits2 = m.Render(w, h)
        trace(torch, m, rays, ordered=True, lod=DISTANCE["text"])
        m.TraceRays(rays[:100], lod=clamp_pair("text"))
        trace(torch, m, rays)
        rgba3, hits3 = m.Render(w, h)
        assert hits3.tobytes() == hits2.tobytes() and rgba3.tobytes() == rgba2.tobytes()
        assert m.GetLod() == (float(pair[0]), float(pair[1]))
        assert lod_hit_is_inner(both["text"], hits3.reshape(-1)).sum() >= 1000
    finally:
        m.SetLod(0.0, 0.0)


# ---------------------------------------------------------------------------- frames
FRAME_KEYS = ("hits", "rgba", "rgba8", "compact", "position", "voxel", "rgb8", "hitmask")
_ray_cache = {}


def camera_rays(oracle_mod, cam_name, w, h, off=(0.5, 0.5)):
    """The oracle's camera rays of the frame (orc_camera_ray), row-major."""
    key = (cam_name, w, h, off)
    if key not in _ray_cache:
        c2w, inv_proj = CAMS[cam_name]().uniforms(w, h)
        ocam = oracle_mod.make_camera(c2w, inv_proj, off, main_light())
        o = np.zeros((h * w, 3), np.float32)
        d = np.zeros((h * w, 3), np.float32)
        f, po, pd, cp = oracle_mod.lib().orc_camera_ray, o.ctypes.data, d.ctypes.data, ctypes.byref(ocam)
        for y in range(h):
            for x in range(w):
                i = 12 * (y * w + x)
                f(cp, x, y, w, h, po + i, pd + i)
        _ray_cache[key] = (o, d)
    return _ray_cache[key]


def tile_masks(hit, w, h):
    """svo_frame.hitmask: per 8x8 tile (row-major) the ballot of its hit lanes, lane = (y % 8) * 8 + x % 8."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), np.uint8)
    pad[:h, :w] = np.asarray(hit).reshape(h, w)
    t = pad.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)
    return np.packbits(t, axis=1, bitorder="little").view("<u8").reshape(-1)


def render_all(torch, m, w, h, mode=0, keys=FRAME_KEYS, stream=None):
    """One svo_render_frame into pattern-filled device buffers; the outputs as numpy arrays."""
    t, n = torch, w * h
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    size = {"hits": n * 24, "rgba": n * 16, "rgba8": n * 4, "compact": n * 12, "position": n * 16, "voxel": n * 8,
            "rgb8": n * 3, "hitmask": tiles * 8}
    b = {k: t.full((size[k],), 0xEE, dtype=t.uint8, device="cuda") for k in keys}
    t.cuda.synchronize()
    m.render_frame(w, h, stack_mode=mode, stream=None if stream is None else stream.cuda_stream,
                   **{k: v.data_ptr() for k, v in b.items()})
    t.cuda.synchronize()
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in b.items()}


def tracer_frame(oracle_mod, svo, cam_name, w, h, mode, pair, off=(0.5, 0.5)):
    o, d = camera_rays(oracle_mod, cam_name, w, h, off)
    res = lod_tracer.trace(svo, o, d, mode, pair[0], pair[1])
    return {"compact": lod_tracer.compact_bytes(res), "voxel": res["key"], "hit": res["hit"],
            "hitmask": tile_masks(res["hit"], w, h), "res": res}


def check_against_tracer(got, exp, what):
    if "compact" in got:
        c = got["compact"].view(np.uint32).reshape(-1, 3)
        bad = np.flatnonzero((c != exp["compact"]).any(axis=1))
        assert len(bad) == 0, f"{what}: {len(bad)} compact records differ, first {bad[:8].tolist()}"
    if "hitmask" in got:
        assert np.array_equal(got["hitmask"].view("<u8"), exp["hitmask"]), f"{what}: hit mask"
    if "voxel" in got:
        assert np.array_equal(got["voxel"].view("<u8"), exp["voxel"]), f"{what}: voxel keys"


@pytest.mark.parametrize("size", ["raster", "strips"])
@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_frame_depth_clamp_equals_oracle_on_pruned_pool(torch, oracle_mod, both, masters, pool, size):
    """SetLod(0, 2^-k): every svo_frame output equals oracle.render_ex on the pruned pool, whole frame."""
    m, (w, h) = masters[pool], SIZES[size]
    cut = pruned(both[pool], CLAMP_K[pool])
    osvo = oracle_mod.OracleSVO(nodes=cut.to_v2(), attachments=cut.attachments)
    try:
        m.SetLod(*clamp_pair(pool))
        for cam_name, cam in CAMS.items():
            c2w, inv_proj = cam().uniforms(w, h)
            ocam = oracle_mod.make_camera(c2w, inv_proj, (0.5, 0.5), main_light())
            for mode in (0, 1):
                hits, rgba, _, pos, vox = oracle_mod.render_ex(osvo, ocam, w, h, mode)
                hit = (hits["flags"] & 1) != 0
                assert hit.sum() >= 400 and np.all(hits["hit_scale"][hit] >= 23 - CLAMP_K[pool])
                m.UpdateShaderParameters(cam(), w, h)
                for launch in range(2):
                    got = render_all(torch, m, w, h, mode)
                    what = f"{pool} {size} {cam_name} mode {mode} launch {launch}"
                    words = oracle_mod.pack_rgba8(rgba)
                    want = {"hits": hits, "rgba": rgba.astype(np.float32), "rgba8": words,
                            "compact": hits.view(np.uint8).reshape(-1, 24)[:, :12], "position": pos, "voxel": vox,
                            "rgb8": words.view(np.uint8).reshape(-1, 4)[:, :3], "hitmask": tile_masks(hit, w, h)}
                    for k in FRAME_KEYS:
                        assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), f"{what}: {k} differs"
    finally:
        m.SetLod(0.0, 0.0)


@pytest.mark.parametrize("size", ["raster", "strips"])
@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_frame_pixel_footprint_equals_tracer(torch, oracle_mod, both, masters, pool, size):
    """coef = pixel_footprint(pixels = 8): compact records, hit mask and voxel keys are the tracer's on the
    oracle's camera rays; hits, rgba and rgba8 are what svo_assemble_frame rebuilds from those records; at
    least 10 % of the overview pose's hit pixels are inner voxels."""
    m, svo, (w, h) = masters[pool], both[pool], SIZES[size]
    try:
        for cam_name, cam in CAMS.items():
            _, inv_proj = cam().uniforms(w, h)
            pair = (np.float32(pixel_footprint(inv_proj, h, 8)), np.float32(0.0))
            m.SetLod(*pair)
            m.UpdateShaderParameters(cam(), w, h)
            for mode in (0, 1):
                exp = tracer_frame(oracle_mod, svo, cam_name, w, h, mode, pair)
                what = f"{pool} {size} {cam_name} mode {mode}"
                got = render_all(torch, m, w, h, mode)
                check_against_tracer(got, exp, what)
                inner = lod_hit_is_inner(svo, got["compact"].view(COMPACT_DTYPE))
                print(what, "hits", int(exp["hit"].sum()), "inner", int(inner.sum()))
                assert exp["hit"].sum() >= 400
                if cam_name == "overview":
                    assert inner.sum() >= 0.1 * exp["hit"].sum()
                # the frame's other outputs: a function of the compact records (svo_assemble_frame, LOD-blind)
                t, n = torch, w * h
                part = t.from_numpy(got["compact"].copy()).cuda()
                out = {"hits": t.zeros(n * 24, dtype=t.uint8, device="cuda"), "rgba": t.zeros(n * 16, dtype=t.uint8, device="cuda"),
                       "rgba8": t.zeros(n * 4, dtype=t.uint8, device="cuda")}
                t.cuda.synchronize()
                m.assemble_frame(w, h, [part.data_ptr()], _lib.PART_COMPACT, band_rows=8,
                                 **{k: v.data_ptr() for k, v in out.items()})
                m.synchronize()
                for k, v in out.items():
                    assert got[k].tobytes() == v.cpu().numpy().tobytes(), f"{what}: {k} is not the rebuild of its compact record"
    finally:
        m.SetLod(0.0, 0.0)


POLICIES = [{}, {"beam": 0}, {"beam_back": 0, "beam_back_held": -1}, {"beam_back": 2, "beam_back_held": 0},
            {"beam_back": 0, "beam_back_held": 0}, {"tile_order": 0}, {"fetch_all": 0}, {"fetch_all": 1},
            {"segments": 0}, {"segments": 1, "seg_all": 8}]
JITTER = (0.25, 0.75)
# (pose, pixels of ray_size_coef, ray_size_bias) on the depth-7 tree, whose splat lists' finest boxes have
# sides s_min = 2^-5 (a new view's, beam_back 2) and 2^-7 (a held view's, beam_back_held 0), and what the
# beam floor is: T' = ((2 s_min - bias) / coef)(1 - sqrt(3) coef) - sqrt(3) bias.
POLICY_SCENES = [
    ("main", 2, 0.0),               # coef 0.04: T' = 1.33 and 0.33 -- finite and positive under both lists
    ("main", 2, 2.0 ** -6),         # T' = 0.97 under the new view's list; bias >= 2 s_min under the held one: -inf
    ("overview", 8, 2.0 ** -3),     # bias >= 2 s_min under both: -inf, with a coefficient
    ("overview", 0, 2.0 ** -4),     # the depth clamp at k = 4: bias >= 2 s_min under both, -inf
]


@pytest.mark.parametrize("size", ["raster", "strips"])
def test_policy_never_changes_a_lod_frame(torch, oracle_mod, both, size):
    """The same LOD frame under every render policy, on the first, second and third launch at a held view,
    after a launch with a jittered _PixelOffset, and that jittered frame itself: always the tracer's bytes.
    This is the beam floor's and the held splat list's test (segments and the latency form must stay off)."""
    svo, (w, h) = both["tree7"], SIZES[size]
    keys = ("compact", "hitmask", "voxel")
    scenes = []
    for cam_name, px, bias in POLICY_SCENES:
        _, inv_proj = CAMS[cam_name]().uniforms(w, h)
        pair = (np.float32(pixel_footprint(inv_proj, h, px)), np.float32(bias))
        exp = tracer_frame(oracle_mod, svo, cam_name, w, h, 1, pair)
        exp_j = tracer_frame(oracle_mod, svo, cam_name, w, h, 1, pair, JITTER)
        inner = lod_hit_is_inner(svo, np.ascontiguousarray(exp["compact"]).view(COMPACT_DTYPE).reshape(-1))
        distinct = len(np.unique(exp["compact"], axis=0))
        print(size, cam_name, pair, "hits", int(exp["hit"].sum()), "inner", int(inner.sum()), "distinct records", distinct)
        assert inner.sum() >= 1000 and distinct >= 500 and exp_j["compact"].tobytes() != exp["compact"].tobytes()
        if (cam_name, px, bias) == POLICY_SCENES[0]:
            assert (exp["hit"] & ~inner).sum() >= 1000, "no leaf-scale hits beside the inner ones"
        scenes.append((cam_name, pair, exp, exp_j))
    for cfg in POLICIES:
        m = RaytracingMaster(device=0, capacity_nodes=1 << 16, config=cfg)
        try:
            m.SetSVOBuffer(svo)
            for cam_name, pair, exp, exp_j in scenes:
                cam, what = CAMS[cam_name](), f"{size} {cam_name} {pair} {cfg}"
                m.SetLod(*pair)
                m.UpdateShaderParameters(cam, w, h)
                for launch in range(3):
                    check_against_tracer(render_all(torch, m, w, h, 1, keys), exp, f"{what} launch {launch}")
                m.UpdateShaderParameters(cam, w, h, pixel_offset=JITTER)
                check_against_tracer(render_all(torch, m, w, h, 1, keys), exp_j, f"{what} jittered")
                m.UpdateShaderParameters(cam, w, h)
                check_against_tracer(render_all(torch, m, w, h, 1, keys), exp, f"{what} after the jitter")
        finally:
            m.close()


def test_entry_points_and_stream_give_the_same_frame(torch, oracle_mod, both):
    """The LOD frame through svo_render, svo_render_samples (S = 1 and 4, against S single renders +
    svo_accumulate), svo_render_progressive, a two-member context on device 0 twice, and a caller stream."""
    from raytracingtest_amd.camera import jitter_offsets
    svo, (w, h) = both["tree7"], SIZES["strips"]
    cam, n = main_camera(), w * h
    _, inv_proj = cam.uniforms(w, h)
    pair = (np.float32(pixel_footprint(inv_proj, h, 2)), np.float32(0.0))
    exp = tracer_frame(oracle_mod, svo, "main", w, h, 0, pair)
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16)
    m2 = RaytracingMaster(devices=[0, 0], capacity_nodes=1 << 16)
    try:
        for x in (m, m2):
            x.SetSVOBuffer(svo)
            x.SetLod(*pair)
            x.UpdateShaderParameters(cam, w, h)
        assert m2.GetLod() == m2.member(1).GetLod() == (float(pair[0]), float(pair[1]))
        ref = render_all(torch, m, w, h, 0)
        check_against_tracer(ref, exp, "single context")
        # svo_render (host path), a caller stream, the two-member context
        rgba, hits = m.Render(w, h)
        assert hits.tobytes() == ref["hits"].tobytes() and rgba.tobytes() == ref["rgba"].tobytes()
        s = torch.cuda.Stream()
        on_stream = render_all(torch, m, w, h, 0, stream=s)
        for k in FRAME_KEYS:
            assert on_stream[k].tobytes() == ref[k].tobytes(), f"caller stream: {k}"
        m.forget_stream(s.cuda_stream)
        rgba, hits = m2.Render(w, h)
        assert hits.tobytes() == ref["hits"].tobytes() and rgba.tobytes() == ref["rgba"].tobytes()
        # svo_render_progressive: the first sample replaces the frame
        _, prog = m.RenderProgressive(w, h, want_rgba8=False, want_rgba=True)
        assert prog.tobytes() == ref["rgba"].tobytes()
        _, prog2 = m2.RenderProgressive(w, h, want_rgba8=False, want_rgba=True)
        assert prog2.tobytes() == ref["rgba"].tobytes()
        # svo_render_samples against single renders + svo_accumulate
        offs = jitter_offsets(4)
        for S in (1, 4):
            want = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
            smp = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for k in range(S):
                m.UpdateShaderParameters(cam, w, h, pixel_offset=tuple(float(v) for v in offs[k]))
                m.render_frame(w, h, rgba=smp.data_ptr())
                m.accumulate_device(want.data_ptr(), smp.data_ptr(), n, sample=k)
            m.synchronize()
            m.UpdateShaderParameters(cam, w, h)
            acc = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            m.render_samples(w, h, offs[:S], 0, acc.data_ptr())
            m.synchronize()
            assert acc.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), f"svo_render_samples S = {S}"
            assert acc.cpu().numpy().tobytes() != np.zeros(n * 4, np.float32).tobytes()
    finally:
        m.close()
        m2.close()


# ---------------------------------------------------------------------------- other cases
def test_count_fetches_drop_with_lod(torch, both):
    """svo_count_fetches: with LOD the sum is strictly below the sum without it, for the default walk and
    under SVO_OPT_COUNT_BEAM -- asserted on the frame tests' own pair, pixels = 8, on both poses.

    From the same start a ray's LOD walk is a prefix of its walk without LOD, so the default walk (always
    from the cube entry) can only lose fetches.  Under COUNT_BEAM a LOD launch starts every ray at
    min(beam start, floor), and an earlier start ADDS fetches: with a pair that ends few walks early the sum
    can rise.  That case is measured here and printed, not asserted -- pixels = 2 from the Main pose on the
    MI355X: default walk 1,203,631 -> 1,138,363 fetches, under COUNT_BEAM 630,384 -> 678,297 (T' = 0.36
    under the held list moves most starts forward of the beam's; sky rays walk from the floor instead of
    skipping the cube).  DESIGN.md 3.1f reports it as what the floor costs."""
    svo, (w, h) = both["tree7"], SIZES["strips"]
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16)
    try:
        m.SetSVOBuffer(svo)
        buf = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def sums(cam_name, pixels, count_beam):
            cam = CAMS[cam_name]()
            _, inv_proj = cam.uniforms(w, h)
            m.UpdateShaderParameters(cam, w, h)
            m.set_count_beam(count_beam)
            out = []
            for coef in (0.0, pixel_footprint(inv_proj, h, pixels)):
                m.SetLod(coef, 0.0)
                m.count_fetches_device(w, h, buf.data_ptr())
                m.synchronize()
                out.append(int(buf.cpu().numpy().astype(np.int64).sum()))
            print(f"fetches off / on: {cam_name} pixels {pixels} count_beam {count_beam}: {out}")
            return out
        for cam_name in CAMS:
            for count_beam in (False, True):
                off, on = sums(cam_name, 8, count_beam)
                assert 0 < on < off, (cam_name, count_beam, off, on)
        for count_beam in (False, True):   # a pair whose floor binds while few walks end early: figures only
            sums("main", 2, count_beam)
    finally:
        m.close()


def test_shadow_rays_with_lod_is_a_state_error(torch, both):
    svo, (w, h) = both["text"], SIZES["raster"]
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16)
    try:
        m.SetSVOBuffer(svo)
        m.UpdateShaderParameters(main_camera(), w, h)
        m.SetLod(0.01, 0.0)
        m.SetShadowRays(True)
        n = w * h
        b = {"hits": torch.full((n * 24,), 0xEE, dtype=torch.uint8, device="cuda"),
             "rgba": torch.full((n * 16,), 0xEE, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()
        with pytest.raises(SvoError, match=r"\(-5\).*shadow rays with LOD"):
            m.render_frame(w, h, **{k: v.data_ptr() for k, v in b.items()})
        with pytest.raises(SvoError, match=r"\(-5\)"):
            m.render_device(w, h, rgba_ptr=b["rgba"].data_ptr(), hits_ptr=b["hits"].data_ptr())
        with pytest.raises(SvoError, match=r"\(-5\)"):
            m.Render(w, h)
        with pytest.raises(SvoError, match=r"\(-5\)"):
            m.RenderProgressive(w, h)
        with pytest.raises(SvoError, match=r"\(-5\)"):
            m.render_samples(w, h, [(0.5, 0.5)], 0, b["rgba"].data_ptr())
        m.synchronize()
        torch.cuda.synchronize()
        assert all(bool((v == 0xEE).all()) for v in b.values()), "an output was written"
        m.SetShadowRays(False)
        m.render_frame(w, h, **{k: v.data_ptr() for k, v in b.items()})   # LOD alone renders
        m.SetShadowRays(True)
        m.SetLod(0.0, 0.0)
        m.render_frame(w, h, **{k: v.data_ptr() for k, v in b.items()})   # shadows alone render
        m.synchronize()
    finally:
        m.close()


@pytest.mark.parametrize("pool", ["text", "tree7"])
def test_set_lod_off_restores_the_parent_bytes(torch, oracle_mod, both, masters, pool):
    """SetLod(0, 0) after LOD launches: the frame equals the unclamped oracle's, byte for byte."""
    m, svo, (w, h) = masters[pool], both[pool], SIZES["strips"]
    cam = overview_camera()
    c2w, inv_proj = cam.uniforms(w, h)
    osvo = oracle_mod.OracleSVO(nodes=svo.to_v2(), attachments=svo.attachments)
    hits, rgba, _, pos, vox = oracle_mod.render_ex(osvo, oracle_mod.make_camera(c2w, inv_proj, (0.5, 0.5), main_light()), w, h, 0)
    m.UpdateShaderParameters(cam, w, h)
    m.SetLod(pixel_footprint(inv_proj, h, 8), 0.0)
    lod = render_all(torch, m, w, h, 0)
    m.SetLod(0.0, 0.0)
    assert m.GetLod() == (0.0, 0.0)
    for launch in range(3):
        got = render_all(torch, m, w, h, 0)
        assert got["hits"].tobytes() == hits.tobytes() and got["rgba"].tobytes() == rgba.astype(np.float32).tobytes()
        assert got["position"].tobytes() == pos.tobytes() and np.array_equal(got["voxel"].view("<u8"), vox)
        assert got["hitmask"].tobytes() == tile_masks((hits["flags"] & 1) != 0, w, h).tobytes()
    assert lod["hits"].tobytes() != hits.tobytes()
