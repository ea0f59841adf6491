"""GPU ray queries (svo_trace_rays / svo_trace_rays_host) against the CPU oracle's
orc_intersect_ex on the rays as traced (query.sanitize_rays): every comparison is byte
equality of hit records, positions, voxel keys and hit masks."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

from raytracingtest_amd import HIT_DTYPE, RaytracingMaster, SvoError
from raytracingtest_amd import _lib
from raytracingtest_amd.builder import build_from_leaves
from raytracingtest_amd.camera import main_camera, main_light, overview_camera
from raytracingtest_amd.query import make_rays
from tests.conftest import ROOT
from tests.query_util import MISS, expected, mixed_batch, oracle_svo, pack_mask, random_batch
from tests.test_c_host import _build

pytestmark = pytest.mark.gpu

PAD = 64          # extra entries behind every output buffer, filled with 0xEE
OUTPUTS = ("hits", "position", "voxel", "hitmask")
ITEM = {"hits": 24, "position": 16, "voxel": 8, "hitmask": 8}


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rm(torch, text_svo):
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16)
    m.SetSVOBuffer(text_svo)
    yield m
    m.close()


@pytest.fixture(scope="module")
def batch(oracle_mod, text_svo):
    """The random batch and what the oracle says about it on the Text fixture, per stack mode."""
    rays = random_batch()
    osvo = oracle_svo(oracle_mod, text_svo)
    return {"rays": rays, "osvo": osvo, 0: expected(oracle_mod, osvo, rays, 0), 1: expected(oracle_mod, osvo, rays, 1)}


def trace(torch, m, rays, mode=0, ordered=False, raw=False, stream=None, outputs=OUTPUTS):
    """One device query into 0xEE-filled buffers with PAD spare entries each; checks that the spare
    entries come back untouched and returns the outputs as numpy arrays."""
    n = len(rays)
    count = {k: (n + 63) // 64 if k == "hitmask" else n for k in outputs}
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    bufs = {k: torch.full(((count[k] + PAD) * ITEM[k],), 0xEE, dtype=torch.uint8, device="cuda") for k in outputs}
    torch.cuda.synchronize()   # the fills run on torch's stream, the query on the context's own
    m.trace_rays_device(d_rays.data_ptr(), n, stack_mode=mode, ordered=ordered, raw=raw,
                        stream=None if stream is None else stream.cuda_stream,
                        **{k: v.data_ptr() for k, v in bufs.items()})
    # the device, not svo_synchronize: that would make the context forget which stream used its query
    # scratch last, and the hand-over between streams is part of what the ordered tests cover
    torch.cuda.synchronize()
    out = {}
    for k, v in bufs.items():
        a = v.cpu().numpy()
        assert np.all(a[count[k] * ITEM[k]:] == 0xEE), f"{k}: written past its {count[k]} entries"
        out[k] = a[:count[k] * ITEM[k]]
    return out


def same(got, exp, n=None, what=""):
    """Byte equality of every output in `got` with the first n rays of the expectation."""
    n = len(exp["hits"]) if n is None else n
    for k, a in got.items():
        want = pack_mask((exp["hits"]["flags"][:n] & 1) != 0) if k == "hitmask" else exp[k][:n]
        if a.tobytes() != np.ascontiguousarray(want).tobytes():
            w = np.frombuffer(np.ascontiguousarray(want).tobytes(), np.uint8).reshape(-1, ITEM[k])
            bad = np.flatnonzero((a.reshape(-1, ITEM[k]) != w).any(axis=1))
            raise AssertionError(f"{what} {k}: {len(bad)} of {len(w)} entries differ, first {bad[:8].tolist()}")


def _pools(text_svo):
    rng = np.random.default_rng(7)
    xyz = np.unique(rng.integers(0, 1 << 7, (4000, 3)), axis=0)
    tree = build_from_leaves(7, xyz, rng.normal(size=(len(xyz), 3)).astype(np.float32))
    return {"text_v1": (text_svo, {}), "text_v2": (text_svo.as_v2(), {}), "tree7": (tree, {}),
            "text_fetch_all_0": (text_svo, {"fetch_all": 0}), "text_fetch_all_1": (text_svo, {"fetch_all": 1})}


@pytest.mark.parametrize("pool", ["text_v1", "text_v2", "tree7", "text_fetch_all_0", "text_fetch_all_1"])
def test_random_batch_matches_oracle(torch, oracle_mod, text_svo, batch, pool):
    """4,096 + 37 rays (origins in [-40, 40]^3, half aimed at the cube, half random), both stack modes,
    every output: the Text fixture as V1 and V2, a depth-7 random tree, fetch_all 0 and 1."""
    svo, cfg = _pools(text_svo)[pool]
    rays = batch["rays"]
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16, config=cfg)
    try:
        m.SetSVOBuffer(svo)
        for mode in (0, 1):
            exp = batch[mode] if pool.startswith("text") else expected(oracle_mod, oracle_svo(oracle_mod, svo), rays, mode)
            hit = (exp["hits"]["flags"][:4096] & 1) != 0
            inside = np.all(np.abs(rays["origin"][:4096]) < 16.0, axis=1)
            if pool.startswith("text"):
                assert hit.sum() >= 1000 and (hit & inside).sum() >= 100, (hit.sum(), (hit & inside).sum())
            else:
                assert hit.sum() >= 200
            same(trace(torch, m, rays, mode), exp, what=f"{pool} mode {mode}")
    finally:
        m.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_sizes_write_exactly_n_entries(torch, rm, batch, n):
    """The first n rays of the batch give the first n results; nothing is written past n entries or
    ceil(n / 64) mask words (trace checks the 0xEE tails), the last mask word's unused bits are 0."""
    for ordered in (False, True):
        got = trace(torch, rm, batch["rays"][:n], ordered=ordered)
        same(got, batch[0], n, what=f"n {n} ordered {ordered}")
        mask = got["hitmask"].view("<u8")
        assert len(mask) == (n + 63) // 64
        if n % 64:
            assert int(mask[-1]) >> (n % 64) == 0


def test_mixed_waves(torch, oracle_mod, rm, batch):
    """Valid, invalid (NaN origin, inf direction, zero direction, NaN t_max) and axis-aligned rays
    interleaved lane by lane in the same waves: invalid ones get exactly the 0x10 miss record and never
    trace (the launch returns at once: no lane runs to the iteration cap), valid ones equal the oracle;
    with RAW_DIRECTIONS the axis-aligned ones equal the oracle on the unclamped directions."""
    rays = mixed_batch()
    exp = expected(oracle_mod, batch["osvo"], rays)
    inv = exp["invalid"]
    assert 80 <= inv.sum() <= len(rays) - 80 and np.count_nonzero(exp["hits"]["flags"] & 1) >= 30
    t0 = time.perf_counter()
    got = trace(torch, rm, rays)
    assert time.perf_counter() - t0 < 5.0
    same(got, exp, what="mixed")
    hits = got["hits"].view(HIT_DTYPE)
    bad = MISS.copy()
    bad["flags"] = _lib.HIT_INVALID_RAY
    assert all(hits[i].tobytes() == bad.tobytes() for i in np.flatnonzero(inv))
    assert not got["position"].view(np.float32).reshape(-1, 4)[inv].any()
    assert np.all(got["voxel"].view("<u8")[inv] == ~np.uint64(0))
    assert not np.any(hits["flags"] & 2)
    raw = expected(oracle_mod, batch["osvo"], rays, raw=True)
    assert np.array_equal(raw["invalid"], inv)
    assert raw["hits"].tobytes() != exp["hits"].tobytes(), "the clamp changes nothing in this batch"
    same(trace(torch, rm, rays, raw=True), raw, what="mixed raw")
    same(trace(torch, rm, rays, mode=1, raw=True), expected(oracle_mod, batch["osvo"], rays, 1, raw=True), what="raw exact")


def test_t_max_filters_the_finished_record(torch, rm, batch):
    """t_max = t / 64 keeps the identical hit; the next float toward 0 gives the plain miss record in
    every output; a ray that starts inside a solid voxel hits at t = 0 with t_max = 0."""
    rays, exp = batch["rays"], batch[0]
    hit = np.flatnonzero(exp["hits"]["flags"] & 1)
    limit = exp["hits"]["t"][hit] * np.float32(1.0 / 64.0)
    keep = rays[hit].copy()
    keep["t_max"] = limit
    got = trace(torch, rm, keep)
    assert got["hits"].tobytes() == exp["hits"][hit].tobytes()
    assert got["position"].tobytes() == exp["position"][hit].tobytes()
    assert got["voxel"].tobytes() == exp["voxel"][hit].tobytes()
    assert got["hitmask"].tobytes() == pack_mask(np.ones(len(hit), bool)).tobytes()
    pos_t = limit > 0
    assert pos_t.sum() >= 1000
    cut = rays[hit][pos_t].copy()
    cut["t_max"] = np.nextafter(limit[pos_t], np.float32(0))
    got = trace(torch, rm, cut)
    assert got["hits"].tobytes() == np.repeat(MISS, len(cut)).tobytes()
    assert not got["position"].any() and np.all(got["voxel"] == 0xFF) and not got["hitmask"].any()
    solid = hit[~pos_t]
    assert len(solid) >= 1, "no ray of the batch starts inside a solid voxel"
    zero = rays[solid].copy()
    zero["t_max"] = 0.0
    got = trace(torch, rm, zero)
    assert got["hits"].tobytes() == exp["hits"][solid].tobytes() and np.all(got["hits"].view(HIT_DTYPE)["t"] == 0)
    assert got["hitmask"].tobytes() == pack_mask(np.ones(len(solid), bool)).tobytes()


def test_ordered_and_unordered_give_identical_bytes(torch, oracle_mod, rm, batch):
    """The key is placement only: the random and the mixed batch, ordered twice (scratch reuse), then on
    a second stream (the scratch's event hand-over) and back on the context's own."""
    mixed = mixed_batch()
    for rays, exp in ((batch["rays"], batch[1]), (mixed, expected(oracle_mod, batch["osvo"], mixed, 1))):
        plain = trace(torch, rm, rays, mode=1)
        same(plain, exp, what="unordered")
        s2 = torch.cuda.Stream()
        for k, stream in enumerate((None, None, s2, None)):
            got = trace(torch, rm, rays, mode=1, ordered=True, stream=stream)
            for name in OUTPUTS:
                assert got[name].tobytes() == plain[name].tobytes(), f"ordered run {k}: {name} differs"
        rm.forget_stream(s2.cuda_stream)
    # fewer outputs: the mask alone, and the records alone
    got = trace(torch, rm, batch["rays"], ordered=True, outputs=("hitmask",))
    assert got["hitmask"].tobytes() == batch[0]["hitmask"].tobytes()
    same(trace(torch, rm, batch["rays"], ordered=True, outputs=("hits",)), batch[0], what="hits alone")


def test_camera_rays_meet_the_render(torch, oracle_mod, rm):
    """The camera rays of a 64 x 48 frame (oracle.camera_ray), traced as a list with RAW_DIRECTIONS,
    give the hit records of Render(64, 48) byte for byte."""
    w, h = 64, 48
    cam = overview_camera()
    c2w, inv_proj = cam.uniforms(w, h)
    ocam = oracle_mod.make_camera(c2w, inv_proj, (0.5, 0.5), main_light())
    o = np.zeros((h * w, 3), np.float32)
    d = np.zeros((h * w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            o[y * w + x], d[y * w + x] = oracle_mod.camera_ray(ocam, x, y, w, h)
    rm.UpdateShaderParameters(cam, w, h)
    _, hits = rm.Render(w, h)
    # not vacuous: the overview pose puts the cube under a few per cent of the pixels -- more than a wave of hits
    assert np.count_nonzero(hits["flags"] & 1) >= 64
    for ordered in (False, True):
        got = trace(torch, rm, make_rays(o, d), raw=True, ordered=ordered, outputs=("hits",))
        assert got["hits"].tobytes() == hits.tobytes()


def test_query_leaves_render_state_alone(torch, rm, batch):
    """render, render (held view), query, render: the third frame equals the second byte for byte, and
    the context's policy is what it was."""
    w, h = 200, 150
    rm.UpdateShaderParameters(main_camera(), w, h)
    rm.Render(w, h)
    rgba2, hits2 = rm.Render(w, h)
    cfg = rm.get_config()
    trace(torch, rm, batch["rays"], ordered=True)
    rm.TraceRays(batch["rays"][:100])
    rgba3, hits3 = rm.Render(w, h)
    assert hits3.tobytes() == hits2.tobytes() and rgba3.tobytes() == rgba2.tobytes()
    assert np.count_nonzero(hits3["flags"] & 1) >= 64
    assert rm.get_config() == cfg


def test_host_path_equals_device_path(torch, rm, batch):
    rays, exp = batch["rays"], batch[0]
    dev = trace(torch, rm, rays)
    for ordered in (False, True):
        hits, pos, vox = rm.TraceRays(rays, ordered=ordered, want_position=True, want_voxel=True)
        assert hits.tobytes() == dev["hits"].tobytes() == exp["hits"].tobytes()
        assert pos.tobytes() == dev["position"].tobytes() and vox.tobytes() == dev["voxel"].tobytes()
    only = rm.TraceRays(rays["origin"][:65], rays["dir"][:65], stack_mode=1)
    assert only.tobytes() == batch[1]["hits"][:65].tobytes()
    cut = rm.TraceRays(rays["origin"][:65], rays["dir"][:65], t_max=0.5)
    assert not np.any(cut["flags"][cut["t"] > 32.0] & 1)
    assert len(rm.TraceRays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0     # n_rays == 0: SVO_OK, no launch


def test_query_without_a_pool_is_a_state_error(torch):
    m = RaytracingMaster(device=0, capacity_nodes=64)
    try:
        with pytest.raises(SvoError, match=r"\(-5\)"):
            m.TraceRays(np.zeros((1, 3)), np.ones((1, 3)))
    finally:
        m.close()


def test_c_raycast_host_runs(torch, tmp_path, oracle_mod):
    """examples/raycast_min.c: its straight-down ray hits the voxel the oracle names."""
    from raytracingtest_amd.svo_data import SVOData
    exe = _build(tmp_path, os.path.join(ROOT, "examples", "raycast_min.c"), "raycast_min")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "raycast_min: ok" in out.stdout
    one = SVOData(childDescriptors=np.array([0xFF00], np.int32),
                  attachments=np.array([0x001F | (0xF800 << 16), 0xC000 << 16], np.uint32))
    s = np.float32(1.0) / np.sqrt(np.float32(3.0))
    rays = make_rays([[3, 40, 5], [-40, -38, -36]], [[0, -1, 0], [s, s, s]])
    exp = expected(oracle_mod, oracle_svo(oracle_mod, one), rays)
    for name, i in (("down", 0), ("diagonal", 1)):
        m = re.search(rf"^{name}: hit (\d) parent (\d+) idx (\d+) scale (\d+) flags (\d+) t (\S+) .*voxel (\d+)$",
                      out.stdout, re.M)
        assert m, out.stdout
        h = exp["hits"][i]
        assert [int(v) for v in m.group(1, 2, 3, 4, 5)] == [1, h["parent"], h["hit_idx"], h["hit_scale"], h["flags"]]
        assert np.float32(m.group(6)) == h["t"] and int(m.group(7)) == int(exp["voxel"][i])
