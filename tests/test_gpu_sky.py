"""The skybox on the GPU (svo_set_skybox, svo_sample_sky): every comparison is byte equality.

References: raytracingtest_amd/sky.py (numpy) for the rule -- tests/test_sky.py pins the header to it and
bounds its error -- on query.camera_rays' directions for the miss pixels of a render, the same render
without a texture for everything else, and tests/sky_util.py's expected frame (the CPU oracle's primary
frame and bounce generations, numpy's fold) for renders with reflection."""
import numpy as np
import pytest

from raytracingtest_amd import RaytracingMaster, SvoError, sky
from raytracingtest_amd import _lib
from raytracingtest_amd.query import camera_rays
from raytracingtest_amd.raytracing_master import band_rows
from tests import reflect_util as ru
from tests import sky_util as su
from tests.lod_util import DISTANCE, pools
from tests.test_gpu_reflection import COLOUR_KEYS, FRAME_KEYS, ITEM, check_frame, dev, render

pytestmark = pytest.mark.gpu

f32 = np.float32
PAD = 64
SIZES = {"odd": (203, 117), "strips": (256, 128)}   # partial edge tiles; 32 tile columns: the XCD-strip path
FRAMES = (("text", "main"), ("tree7", "main"), ("text", "overview"))


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
def masters(torch, both):
    ms = {}
    for name, svo in both.items():
        ms[name] = RaytracingMaster(device=0, capacity_nodes=1 << 16)
        ms[name].SetSVOBuffer(svo)
    yield ms
    for m in ms.values():
        m.close()


def frame_dirs(cam_name, w, h, off=(0.5, 0.5)):
    c2w, inv_proj = ru.CAMS[cam_name]().uniforms(w, h)
    return camera_rays(c2w, inv_proj, w, h, pixel_offset=off)["dir"]


def miss_of(off):
    """The miss pixels of a render's hit records; both branches are certainly exercised."""
    hit = (off["hits"].view(_lib.HIT_DTYPE)["flags"] & 1) != 0
    assert (~hit).sum() >= 30 and hit.sum() >= 300, (int(hit.sum()), int((~hit).sum()))
    return ~hit


def colours_of(rgba):
    words = su.pack_rgba8(rgba)
    return {"rgba": rgba, "rgba8": words, "rgb8": np.ascontiguousarray(words.view(np.uint8).reshape(-1, 4)[:, :3])}


def expected(off, dirs, tex, bil, cl):
    """The colour outputs with a skybox, from the same render without one (`off`, every output)."""
    miss = miss_of(off)
    want = colours_of(su.expected_rgba(dirs, miss, off["rgba"].view(f32), tex, bil, cl))
    # the hit pixels' display words are the no-texture render's own
    hit = ~miss
    assert want["rgba8"][hit].tobytes() == off["rgba8"].view(np.uint32)[hit].tobytes()
    assert want["rgba"].tobytes() != off["rgba"].tobytes()
    return want


# ---------------------------------------------------------------------------- 1. svo_sample_sky
def sample_inputs():
    rng = np.random.default_rng(su.SEED + 2)
    hand = [su.centre_direction(np.arange(37), np.arange(37) % 19, 37, 19), su.axes(), su.zero_sign_cases(),
            np.array([[2.0 ** -22, 0.3, -1], [-2.0 ** -22, 0.3, -1], [0, 1, 0], [0, -5, 0], [0, 0, 2.0 ** 40]])]
    d = np.concatenate([np.asarray(p, np.float64) for p in hand] + [rng.standard_normal((4133, 3)) * 2.0 ** rng.integers(-30, 30, (4133, 1))])
    d = np.concatenate([d.astype(f32), su.invalid_cases()])
    d4 = np.zeros((len(d), 4), f32)
    d4[:, :3] = d
    d4[:, 3] = rng.standard_normal(len(d)).astype(f32)   # w is ignored
    d4[::7, 3] = np.nan
    return d4


def test_sample_sky_equals_numpy(torch, masters):
    m = masters["text"]
    d4 = sample_inputs()
    n = len(d4)
    cases = [(None, True, False)] + [(name, bil, cl) for name in su.textures() for bil, cl in su.FLAG_CASES]
    try:
        for name, bil, cl in cases:
            tex = None if name is None else su.textures()[name]
            m.SetSkybox(tex, bilinear=bil, clamp_v=cl)
            assert m.GetSkybox() == ((0, 0, 0) if tex is None else (tex.shape[1], tex.shape[0], sky.flags_of(bil, cl)))
            want = np.ones((n, 4), f32)
            want[:, :3] = sky.sample_sky(d4, tex, bil, cl)
            assert m.SampleSky(d4).tobytes() == want.tobytes(), f"{name} {bil} {cl}: host path"
            assert m.SampleSky(d4[:, :3]).tobytes() == want.tobytes()
            d_dirs = dev(torch, d4)
            out = torch.full(((n + PAD) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            m.sample_sky_device(d_dirs.data_ptr(), n, out.data_ptr())
            m.synchronize()
            a = out.cpu().numpy()
            assert np.all(a[n * 16:] == 0xEE), "written past n entries"
            assert a[:n * 16].tobytes() == want.tobytes(), f"{name} {bil} {cl}: device path"
            assert d_dirs.cpu().numpy().tobytes() == d4.tobytes()
            s = torch.cuda.Stream()
            inplace = torch.full(((n + PAD) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
            inplace[:n * 16] = d_dirs
            torch.cuda.synchronize()
            m.sample_sky_device(inplace.data_ptr(), n, inplace.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            b = inplace.cpu().numpy()
            assert np.all(b[n * 16:] == 0xEE) and b[:n * 16].tobytes() == want.tobytes(), f"{name} {bil} {cl}: in place"
            m.sample_sky_device(d_dirs.data_ptr(), 0, out.data_ptr())   # n = 0: nothing
            m.synchronize()
            assert np.all(out.cpu().numpy()[n * 16:] == 0xEE)
            assert m.SampleSky(np.zeros((0, 3), f32)).shape == (0, 4)
    finally:
        m.SetSkybox(None)


# ---------------------------------------------------------------------------- 2. svo_render_frame
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("pool,cam_name", FRAMES)
def test_render_frame_misses_are_the_rule(torch, masters, pool, cam_name, size):
    """Every output requested, both stack modes, two launches each (the second takes the cost order): miss
    pixels' colours are numpy's, everything else the bytes of the render without a texture."""
    m, (w, h) = masters[pool], SIZES[size]
    dirs = frame_dirs(cam_name, w, h)
    # between them the three frames take both filters and both v-wraps
    tex_name, bil, cl = {("text", "main"): ("37x19", True, False), ("tree7", "main"): ("64x32", True, True),
                         ("text", "overview"): ("64x32", False, False)}[(pool, cam_name)]
    tex = su.textures()[tex_name]
    try:
        m.UpdateShaderParameters(ru.CAMS[cam_name](), w, h)
        for mode in (0, 1):
            m.SetSkybox(None)
            off = render(torch, m, w, h, mode)
            want = expected(off, dirs, tex, bil, cl)
            m.SetSkybox(tex, bilinear=bil, clamp_v=cl)
            for launch in range(2):
                check_frame(render(torch, m, w, h, mode), want, off, f"{pool} {cam_name} {size} mode {mode} launch {launch}")
    finally:
        m.SetSkybox(None)


def test_render_frame_forms(torch, masters):
    """rgb8 alone, with and without a caller hitmask, a band in band and in frame layout, a caller stream."""
    m, (w, h) = masters["tree7"], SIZES["odd"]
    tex = su.texture(37, 19)
    n = w * h
    try:
        m.UpdateShaderParameters(ru.CAMS["main"](), w, h)
        m.SetSkybox(None)
        off = render(torch, m, w, h)
        want = expected(off, frame_dirs("main", w, h), tex, True, False)
        m.SetSkybox(tex)
        for keys in (("rgb8",), ("rgb8", "hitmask"), ("rgba", "hitmask"), ("rgba8",), ("hits", "voxel", "hitmask")):
            check_frame(render(torch, m, w, h, keys=keys), want, off, f"{keys}")
        s = torch.cuda.Stream()
        check_frame(render(torch, m, w, h, stream=s), want, off, "caller stream")
        m.forget_stream(s.cuda_stream)
        # three ranks of 8-row bands (the last band of 117 rows is partial): band layout, then frame layout
        tiles_x = (w + 7) // 8
        full = {k: np.zeros(n * ITEM[k], np.uint8) for k in ITEM}
        for rank in range(3):
            band = (8, rank, 3)
            rows = band_rows(h, band)
            part = render(torch, m, w, h, band=band)
            for k in ITEM:
                full[k].reshape(h, -1)[rows] = part[k].reshape(len(rows), -1)
            # the part's masks are band-local tiles: a miss in them is a sky pixel of the part
            masks = part["hitmask"].view(np.uint64).reshape(-1, tiles_x)
            hit = (off["hits"].view(_lib.HIT_DTYPE)["flags"] & 1).reshape(h, w)[rows] != 0
            for lr in range(len(rows)):
                bits = (masks[lr // 8, np.arange(w) // 8] >> ((lr % 8) * 8 + np.arange(w) % 8).astype(np.uint64)) & np.uint64(1)
                assert (bits != 0).tolist() == hit[lr].tolist(), (rank, lr)
        check_frame(full, want, off, "band layout")
        into = {k: torch.full((len(full[k]),), 0xEE, dtype=torch.uint8, device="cuda") for k in ITEM}
        for rank in range(3):
            got = render(torch, m, w, h, band=(8, rank, 3), layout=_lib.LAYOUT_FRAME, into=into)
        check_frame(got, want, off, "frame layout")
    finally:
        m.SetSkybox(None)


# ---------------------------------------------------------------------------- 3. shadows, LOD, reflection
@pytest.mark.parametrize("form", [_lib.SHADOW_FUSED, _lib.SHADOW_TILES, _lib.SHADOW_LIST])
def test_with_shadow_rays(torch, both, form):
    svo, (w, h) = both["tree7"], SIZES["odd"]
    tex = su.texture(64, 32)
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16, config={"shadow_form": form})
    try:
        m.SetSVOBuffer(svo)
        m.UpdateShaderParameters(ru.CAMS["main"](), w, h)
        m.SetShadowRays(True)
        off = render(torch, m, w, h)
        shadowed = int(((off["hits"].view(_lib.HIT_DTYPE)["flags"] & 8) != 0).sum())
        print("shadow form", form, "pixels in shadow", shadowed)
        assert shadowed >= 1   # shadows do fall
        want = expected(off, frame_dirs("main", w, h), tex, True, False)
        m.SetSkybox(tex)
        for keys in (FRAME_KEYS, ("rgba8",), ("hits", "rgba", "hitmask")):
            check_frame(render(torch, m, w, h, keys=keys), want, off, f"shadow form {form} {keys}")
    finally:
        m.close()


def test_with_lod(torch, masters):
    m, (w, h) = masters["text"], SIZES["strips"]
    tex = su.texture(37, 19)
    try:
        m.UpdateShaderParameters(ru.CAMS["overview"](), w, h)
        m.SetSkybox(None)
        plain = render(torch, m, w, h)
        m.SetLod(*DISTANCE["text"])
        off = render(torch, m, w, h)
        assert off["hits"].tobytes() != plain["hits"].tobytes()   # LOD is on
        want = expected(off, frame_dirs("overview", w, h), tex, False, True)
        m.SetSkybox(tex, bilinear=False, clamp_v=True)
        for launch in range(2):
            check_frame(render(torch, m, w, h), want, off, f"LOD launch {launch}")
    finally:
        m.SetLod(0.0, 0.0)
        m.SetSkybox(None)


def test_with_reflection(torch, oracle_mod, both, masters):
    """Bounce rays that leave the scene take the rule on their traced direction; primary misses too."""
    pool, cam_name, (w, h) = "tree7", "main", SIZES["odd"]
    m = masters[pool]
    tex = su.texture(64, 32)
    spec, nb = ru.DEFAULT
    try:
        m.UpdateShaderParameters(ru.CAMS[cam_name](), w, h)
        for mode in (0, 1):
            m.SetSkybox(None)
            m.SetReflection(None)
            off = render(torch, m, w, h, mode)
            miss_of(off)
            rgba, on_sky = su.expected_reflection_frame(oracle_mod, pool, both[pool], cam_name, w, h, mode, spec, nb, tex, True, False)
            assert on_sky >= 1000, on_sky
            want = colours_of(rgba)
            gradient = ru.expected_frame(oracle_mod, pool, both[pool], cam_name, w, h, mode, spec, nb)
            assert (rgba != gradient).any(axis=1).sum() >= 1000 + 30   # the texture shows in mirrors and in the sky
            m.SetReflection(spec, nb)
            m.SetSkybox(tex)
            for keys in (FRAME_KEYS, COLOUR_KEYS, ("rgba", "hitmask")):
                check_frame(render(torch, m, w, h, mode, keys=keys), want, off, f"reflection mode {mode} {keys}")
    finally:
        m.SetReflection(None)
        m.SetSkybox(None)


# ---------------------------------------------------------------------------- 4. progressive and host paths
def test_progressive_and_host_paths(torch, oracle_mod, both):
    svo, (w, h) = both["tree7"], SIZES["odd"]
    tex = su.texture(64, 32)
    cam, n = ru.CAMS["main"](), w * h
    offsets = ((0.5, 0.5), (0.25, 0.75))
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16)
    try:
        m.SetSVOBuffer(svo)
        frames = []
        for px_off in offsets:
            m.UpdateShaderParameters(cam, w, h, pixel_offset=px_off)
            off = render(torch, m, w, h)
            frames.append(expected(off, frame_dirs("main", w, h, px_off), tex, True, False)["rgba"])
        m.SetSkybox(tex)
        m.UpdateShaderParameters(cam, w, h, pixel_offset=offsets[0])
        first = render(torch, m, w, h)
        rgba, hits = m.Render(w, h)
        assert rgba.tobytes() == frames[0].tobytes() == first["rgba"].tobytes(), "svo_render"
        assert hits.tobytes() == first["hits"].tobytes(), "svo_render: hit records"
        rgba, _ = m.Render(w, h, want_hits=False)
        assert rgba.tobytes() == frames[0].tobytes(), "svo_render without hits"
        # samples 0 and 1 = the AddShader blend (oracle.accumulate) folded over the two expected frames
        acc = np.zeros((n, 4), f32)
        for k, px_off in enumerate(offsets):
            m.UpdateShaderParameters(cam, w, h, pixel_offset=px_off)
            m.currentSample = k
            words, prog = m.RenderProgressive(w, h, want_rgba8=True, want_rgba=True)
            oracle_mod.accumulate(acc, np.ascontiguousarray(frames[k]), k)
            assert prog.tobytes() == acc.tobytes(), f"progressive sample {k}"
            assert words.tobytes() == oracle_mod.pack_rgba8(acc).tobytes(), f"progressive sample {k}: display words"
    finally:
        m.close()


# ---------------------------------------------------------------------------- 5. state and limits
def test_state_and_limits(torch, both):
    svo, (w, h) = both["tree7"], SIZES["odd"]
    n = w * h
    dirs = frame_dirs("main", w, h)
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16)
    m2 = RaytracingMaster(devices=[0, 0], capacity_nodes=1 << 16)
    try:
        assert _lib.lib().svo_abi_version() == _lib.ABI_VERSION
        m.SetSVOBuffer(svo)
        m.UpdateShaderParameters(ru.CAMS["main"](), w, h)
        assert m.GetSkybox() == (0, 0, 0)
        before = [render(torch, m, w, h) for _ in range(2)][1]
        a, b = su.texture(64, 32), su.texture(37, 19)
        m.SetSkybox(a, bilinear=True, clamp_v=True)
        want_a = expected(before, dirs, a, True, True)
        check_frame(render(torch, m, w, h), want_a, before, "first texture")
        # another size replaces it
        m.SetSkybox(b, bilinear=False)
        assert m.GetSkybox() == (37, 19, 0)
        check_frame(render(torch, m, w, h), expected(before, dirs, b, False, False), before, "second texture")
        # a query between two renders changes neither
        m.SetSkybox(a, bilinear=True, clamp_v=True)
        first = render(torch, m, w, h)
        m.TraceRays(camera_rays(*ru.CAMS["overview"]().uniforms(w, h), w, h), raw=True)
        second = render(torch, m, w, h)
        check_frame(first, want_a, before, "before the query")
        for k in FRAME_KEYS:
            assert first[k].tobytes() == second[k].tobytes(), k
        # the instrumented launches are unaffected
        fetches = torch.zeros(n, dtype=torch.int32, device="cuda")
        m.count_fetches_device(w, h, fetches.data_ptr())
        m.synchronize()
        with_tex = fetches.cpu().numpy().copy()
        # svo_render_samples is a stated limit: refused before anything is enqueued
        acc = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for offs in ([(0.5, 0.5)], [(0.5, 0.5), (0.25, 0.75)]):
            with pytest.raises(SvoError, match=r"\(-5\).*svo_render_samples with a skybox"):
                m.render_samples(w, h, offs, 0, acc.data_ptr())
        m.synchronize()
        assert bool((acc == 0xEE).all()), "an output was written"
        # NULL restores every byte
        m.SetSkybox(None)
        assert m.GetSkybox() == (0, 0, 0)
        after = render(torch, m, w, h)
        for k in FRAME_KEYS:
            assert after[k].tobytes() == before[k].tobytes(), k
        m.count_fetches_device(w, h, fetches.data_ptr())
        m.synchronize()
        assert fetches.cpu().numpy().tobytes() == with_tex.tobytes()
        m.render_samples(w, h, [(0.5, 0.5)], 0, acc.data_ptr())   # and svo_render_samples renders again
        m.synchronize()
        # argument errors on a live context leave the texture as it was
        m.SetSkybox(b)
        L, ctx = _lib.lib(), m._ctx
        t = np.array(b)
        for args in ((t.ctypes.data, 0, 19, 0), (t.ctypes.data, 37, -1, 0), (t.ctypes.data, 8193, 19, 0), (t.ctypes.data, 37, 8193, 0),
                     (t.ctypes.data, 37, 19, 4), (None, 0, 0, 8)):
            assert L.svo_set_skybox(ctx, *args) == -1, args
        for bad in (np.nan, np.inf, -0.5):
            t2 = t.copy()
            t2[7, 11, 1] = bad
            assert L.svo_set_skybox(ctx, t2.ctypes.data, 37, 19, 0) == -1, bad
        t2 = t.copy()
        t2[:, :, 3] = np.nan     # alpha is ignored
        assert L.svo_set_skybox(ctx, t2.ctypes.data, 37, 19, 1) == 0
        assert L.svo_set_skybox(None, t.ctypes.data, 37, 19, 0) == -1
        check_frame(render(torch, m, w, h), expected(before, dirs, b, True, False), before, "alpha ignored")
        # a multi-device context: a texture is refused, NULL is accepted
        m2.SetSVOBuffer(svo)
        with pytest.raises(SvoError, match=r"\(-5\).*multi-device"):
            m2.SetSkybox(b)
        m2.SetSkybox(None)
        assert m2.GetSkybox() == (0, 0, 0)
    finally:
        m.close()
        m2.close()
