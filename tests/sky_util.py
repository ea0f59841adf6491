"""Shared inputs of the skybox tests (tests/test_sky.py, tests/test_gpu_sky.py): the three textures, the
direction sweep, the hand cases and the expected frames of renders with a skybox set."""
import numpy as np

from raytracingtest_amd import sky

f32 = np.float32
SEED = 20261020
SIZES = ((64, 32), (37, 19), (1, 1))                       # width x height
FLAG_CASES = ((False, False), (True, False), (False, True), (True, True))   # (bilinear, clamp_v)
_cache = {}


def texture(w, h):
    """H x W x 4 f32, every texel distinct in every colour channel (a wrong index shows): channel c of
    texel k is a permutation's value (perm_c[k] + 1) / (W H + 1), alpha a value nobody reads."""
    key = ("tex", w, h)
    if key not in _cache:
        rng = np.random.default_rng(SEED + 7919 * w + h)
        n = w * h
        t = np.empty((n, 4), f32)
        for c in range(3):
            t[:, c] = ((rng.permutation(n) + 1) / (n + 1)).astype(f32)
        t[:, 3] = rng.random(n).astype(f32)
        for c in range(3):
            assert len(np.unique(t[:, c])) == n
        t = t.reshape(h, w, 4)
        t.setflags(write=False)
        _cache[key] = t
    return _cache[key]


def textures():
    return {f"{w}x{h}": texture(w, h) for w, h in SIZES}


def axes():
    return np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)


def zero_sign_cases():
    """Every combination of +0, -0, +1, -1 per component (the all-zero ones are invalid directions)."""
    vals = np.array([0.0, -0.0, 1.0, -1.0], f32)
    g = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g, f32)


def invalid_cases():
    nan, inf = f32(np.nan), f32(np.inf)
    return np.array([[0, 0, 0], [-0.0, 0, -0.0], [nan, 0, 1], [0, nan, 1], [0, 1, nan], [inf, 0, 1], [0, -inf, 1],
                     [1, 1, inf], [nan, nan, nan], [inf, inf, inf]], f32)


def sweep(n_random=1 << 20):
    """The direction sweep (n x 3 f32): n_random random directions, directions within 2^-20 of both poles
    and of the u seam, the six axes, non-unit lengths 2^-60 .. 2^60, +-0 components, invalid ones."""
    key = ("sweep", n_random)
    if key not in _cache:
        rng = np.random.default_rng(SEED)
        parts = [rng.standard_normal((n_random, 3))]
        m = 4096
        eps = 2.0 ** -rng.uniform(20, 60, m)
        ang = rng.uniform(0, 2 * np.pi, m)
        for pole in (1.0, -1.0):
            parts.append(np.stack([eps * np.cos(ang), np.full(m, pole), eps * np.sin(ang)], axis=1))
            parts.append(np.stack([eps, np.full(m, pole), np.zeros(m)], axis=1))
            parts.append(np.stack([np.zeros(m), np.full(m, pole), -eps], axis=1))
        for sgn in (1.0, -1.0):   # the u seam: -z > 0, x -> +-0
            parts.append(np.stack([sgn * eps, rng.uniform(-1, 1, m), np.full(m, -1.0)], axis=1))
            parts.append(np.stack([sgn * eps, rng.uniform(-1, 1, m) * eps, np.full(m, -1.0)], axis=1))
        unit = rng.standard_normal((121 * 32, 3))
        unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        parts.append(unit * np.repeat(2.0 ** np.arange(-60, 61), 32)[:, None])
        d = np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(f32)
        d = np.concatenate([d, axes(), f32(2.0 ** 60) * axes(), f32(2.0 ** -60) * axes(), zero_sign_cases(), invalid_cases()])
        d = np.ascontiguousarray(d, f32)
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def reference_uv(dirs):
    """(u, v_linear) in float64 from numpy.arctan2 on the same f32 inputs: u in [0, 1) (wrapped), v_linear =
    1 - polar / pi in [0, 1] (the clamp form; its repeat form is v_linear mod 1)."""
    d = np.asarray(dirs, f32).astype(np.float64)
    m = np.max(np.abs(d), axis=1)
    with np.errstate(all="ignore"):
        x, y, z = d[:, 0] / m, d[:, 1] / m, d[:, 2] / m
        polar = np.arctan2(np.hypot(x, z), y)
        azim = np.arctan2(x, -z)
    phi = azim / -np.pi * 0.5
    return phi - np.floor(phi), 1.0 - polar / np.pi


def circular(a, b):
    e = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 1.0
    return np.minimum(e, 1.0 - e)


def centre_direction(i, j, w, h):
    """A float64 direction through the centre of texel (i, j) of a w x h texture (repeat or clamp alike:
    v = (j + 0.5) / h is inside (0, 1))."""
    u, v = (i + 0.5) / w, (j + 0.5) / h
    polar = (1.0 - v) * np.pi          # v = theta + 1 = 1 - polar / pi
    azim = -2.0 * np.pi * u            # u = phi mod 1, phi = -azim / (2 pi)
    s = np.sin(polar)
    return np.stack([s * np.sin(azim), np.cos(polar), -s * np.cos(azim)], axis=-1)


def expected_rgba(dirs, miss, base_rgba, texels, bilinear, clamp_v):
    """The colour frame of a render with a skybox: base_rgba (the same render without one) with the miss
    pixels replaced by the rule on their camera directions, alpha 1."""
    out = np.array(base_rgba, f32).reshape(-1, 4).copy()
    out[miss, :3] = sky.sample_sky(np.asarray(dirs, f32).reshape(-1, 3)[miss], texels, bilinear, clamp_v)
    out[miss, 3] = 1.0
    return out


def pack_rgba8(rgb):
    """Display RGBA8 words of n x 3 f32 colours: (uint)(saturate(c) * 255 + 0.5) per channel, alpha 255."""
    c = np.asarray(rgb, f32)[:, :3]
    with np.errstate(invalid="ignore"):
        q = (np.fmin(np.fmax(c, f32(0.0)), f32(1.0)) * f32(255.0) + f32(0.5)).astype(np.uint32)
    return q[:, 0] | (q[:, 1] << 8) | (q[:, 2] << 16) | np.uint32(255 << 24)


def expected_reflection_frame(oracle_mod, name, svo, cam_name, w, h, mode, specular, max_bounces, texels, bilinear, clamp_v):
    """(RGBA32F [w * h, 4], bounce rays that ended on the sky) of a render with svo_set_reflection and a
    skybox: tests/reflect_util.py's primary frame and bounce generations (the CPU oracle) and the fold of
    its expected_frame, with sky.sample_sky in the place of its sky() for bounce rays that miss, and for
    the primary misses (on the oracle's own camera directions)."""
    import ctypes

    from raytracingtest_amd.camera import main_light
    from tests import reflect_util as ru
    prim = ru.primary(oracle_mod, name, svo, cam_name, w, h, mode)
    gens = ru.generations(oracle_mod, name, svo, cam_name, w, h, mode)
    rgba = prim["rgba"].copy()
    res = rgba[prim["px"], :3].copy()
    spec = np.asarray(specular, f32)
    e = np.ones(3, f32)
    on_sky = 0
    for g in gens[:max_bounces]:
        e = e * spec
        if not e.any():
            break
        hit = (g["hits"]["flags"] & 1) != 0
        n = np.stack([g["hits"]["nx"], g["hits"]["ny"], g["hits"]["nz"]], axis=1)
        traced = g["traced"]["dir"][~g["invalid"]]
        col = np.where(hit[:, None], ru.shade_hit(n, g["albedo"], main_light()), sky.sample_sky(traced, texels, bilinear, clamp_v))
        at = g["idx"][~g["invalid"]]
        res[at] = res[at] + e[None, :] * col.astype(f32)
        on_sky += int((~hit).sum())
    rgba[prim["px"], :3] = res
    miss = np.flatnonzero((prim["hits"]["flags"] & 1) == 0)
    c2w, inv_proj = ru.POSES[cam_name]().uniforms(w, h)
    ocam = oracle_mod.make_camera(c2w, inv_proj, (0.5, 0.5), main_light())
    o, d = np.zeros((len(miss), 3), f32), np.zeros((len(miss), 3), f32)
    fn, po, pd, cp = oracle_mod.lib().orc_camera_ray, o.ctypes.data, d.ctypes.data, ctypes.byref(ocam)
    for j, p in enumerate(miss.tolist()):
        fn(cp, p % w, p // w, w, h, po + 12 * j, pd + 12 * j)
    rgba[miss, :3] = sky.sample_sky(d, texels, bilinear, clamp_v)
    rgba[miss, 3] = 1.0
    return rgba, on_sky
