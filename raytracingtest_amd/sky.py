"""The sky rule: the numpy statement of csrc/svo_sky.h (svo_set_skybox / svo_sample_sky in
include/svo_rt.h; INTEGRATION.md "Skybox").

From a direction d = (x, y, z), used as given (not assumed unit), to the RGB of a ray that leaves the
scene.  Every operation is one f32 rounding, no fma; only + - * /, sqrt, floor, compares and selects,
so this file, the header under plain g++ and the header on the device agree byte for byte.

  1. invalid    a non-finite component, or x = y = z = 0: the colour is (0, 0, 0).  Otherwise d is
                divided by max(|x|, |y|, |z|).
  2. angles     polar = atan2f32(sqrt(x x + z z), y) in [0, PI], azim = atan2f32(x, -z); atan2f32 is
                the rule's own (below).  For a unit direction polar is the reference's acos(y)
                (RaytraceCompute.compute:123): a restatement, mathematically identical, in other f32
                operations.
  3. reference  theta = polar / -PI, phi = azim / -PI * 0.5, PI = 3.14159265f (R:11, 123-124); the
                sample point is (phi, theta).
  4. wrap       u = phi - floor(phi), 1 -> 0.  v: the same on theta (repeat, Unity's default
                wrapMode), or min(max(theta + 1, 0), 1) (clamp).
  5. nearest    i = min(int(floor(u W)), W - 1), j = min(int(floor(v H)), H - 1).
  6. bilinear   x = u W - 0.5, i0 = floor(x), fx = x - i0, columns i0 and i0 + 1 wrapped mod W; rows
                likewise, wrapped mod H or clamped to [0, H - 1];
                c = (t00 (1 - fx) + t10 fx) (1 - fy) + (t01 (1 - fx) + t11 fx) fy per channel.
  7. rows       row 0 of the array is v = 0 (Unity's GetPixels order, bottom row first); straight up
                is theta = 0 -> v = 0 with repeat and v = 1 with clamp; the horizon is v = 0.5.

atan2f32(y, x): a = min(|y|, |x|) / max(|y|, |x|); if a > tan(pi/8): t = (a - 1) / (a + 1), else t = a;
r = t + t (t^2 (c3 + t^2 (c2 + t^2 (c1 + t^2 c0)))) evaluated by Horner (Cephes' atanf coefficients), plus
PI/4 if folded; r = PI/2 - r if |y| > |x|; r = PI - r if x < 0; the sign of y (of a zero y too).
atan2f32(0, 0) = +0.

Without a texture the rule is the procedural gradient of d's y as given (an invalid direction: black).
"""
import numpy as np

f = np.float32
PI = f(3.14159265)
PI_2 = f(PI * f(0.5))
PI_4 = f(PI * f(0.25))
BILINEAR = 1
CLAMP_V = 2
MAX_DIM = 8192


def _xyz(dirs):
    """n x 3 f32 of n x 3 or n x 4 directions (n may be 0)."""
    d = np.asarray(dirs, f)
    if d.size == 0:
        return np.zeros((0, 3), f)
    return d.reshape(-1, d.shape[-1])[:, :3]


def _abs(x):
    return np.where(x < 0, -x, x)


def _atan_unit(a):
    fold = a > f(0.4142135623730950)
    t = np.where(fold, (a - f(1.0)) / (a + f(1.0)), a)
    z = t * t
    p = f(8.05374449538e-2) * z
    p = p - f(1.38776856032e-1)
    p = p * z
    p = p + f(1.99777106478e-1)
    p = p * z
    p = p - f(3.33329491539e-1)
    p = p * z
    p = p * t
    p = p + t
    return np.where(fold, p + PI_4, p)


def atan2f32(y, x):
    """The rule's atan2 on f32 arrays."""
    y = np.asarray(y, f)
    x = np.asarray(x, f)
    with np.errstate(all="ignore"):
        ay, ax = _abs(y), _abs(x)
        steep = ay > ax
        a = np.where(steep, ax, ay) / np.where(steep, ay, ax)
        r = _atan_unit(a)
        r = np.where(steep, PI_2 - r, r)
        r = np.where(x < 0, PI - r, r)
        neg = (y < 0) | ((y == 0) & (f(1.0) / y < 0))
        r = np.where(neg, -r, r)
        return np.where((ay == 0) & (ax == 0), f(0.0), r).astype(f)


def direction_uv(dirs, clamp_v=False):
    """Steps 1-4: (valid, u, v) of n directions (n x 3, or n x 4 with w ignored)."""
    d = _xyz(dirs)
    with np.errstate(all="ignore"):
        finite = ((d - d) == 0).all(axis=1)
        a = _abs(d)
        m = np.where(a[:, 0] > a[:, 1], a[:, 0], a[:, 1])
        m = np.where(m > a[:, 2], m, a[:, 2])
        valid = finite & ~(m == 0)
        x, y, z = d[:, 0] / m, d[:, 1] / m, d[:, 2] / m
        xx, zz = x * x, z * z
        s = np.sqrt(xx + zz)
        polar = atan2f32(s, y)
        azim = atan2f32(x, -z)
        theta = polar / -PI
        phi = azim / -PI * f(0.5)
        u = phi - np.floor(phi)
        u = np.where(u >= 1, f(0.0), u)
        if clamp_v:
            v = theta + f(1.0)
            v = np.where(v > 0, v, f(0.0))
            v = np.where(v < 1, v, f(1.0))
        else:
            v = theta - np.floor(theta)
            v = np.where(v >= 1, f(0.0), v)
    u = np.where(valid, u, f(0.0)).astype(f)
    v = np.where(valid, v, f(0.0)).astype(f)
    return valid, u, v


def sample_uv(texels, u, v, bilinear=True, clamp_v=False):
    """Steps 5-6: the H x W x 4 (or x 3) texture at (u, v); n x 3 f32."""
    tex = np.asarray(texels, f)
    H, W = tex.shape[:2]
    tex = tex[:, :, :3]
    fw, fh = f(W), f(H)
    if not bilinear:
        i = np.minimum(np.floor(u * fw).astype(np.int64), W - 1)
        j = np.minimum(np.floor(v * fh).astype(np.int64), H - 1)
        return tex[j, i].astype(f)
    x, y = u * fw - f(0.5), v * fh - f(0.5)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    i0, j0 = xf.astype(np.int64), yf.astype(np.int64)
    i1, j1 = i0 + 1, j0 + 1
    i0 = np.where(i0 < 0, i0 + W, i0)
    i1 = np.where(i1 >= W, i1 - W, i1)
    if clamp_v:
        j0 = np.maximum(j0, 0)
        j1 = np.minimum(j1, H - 1)
    else:
        j0 = np.where(j0 < 0, j0 + H, j0)
        j1 = np.where(j1 >= H, j1 - H, j1)
    gx, gy = f(1.0) - fx, f(1.0) - fy
    lo = tex[j0, i0] * gx
    lo = lo + tex[j0, i1] * fx
    hi = tex[j1, i0] * gx
    hi = hi + tex[j1, i1] * fx
    lo = lo * gy
    return (lo + hi * fy).astype(f)


def gradient(dir_y):
    """The procedural sky (no texture): n x 3 f32 of the directions' y."""
    k = f(0.5) * np.asarray(dir_y, f) + f(0.5)
    return np.stack([f(0.25) + f(0.5) * k, f(0.35) + f(0.55) * k, f(0.6) + f(0.4) * k], axis=1).astype(f)


def sample_sky(dirs, texels=None, bilinear=True, clamp_v=False):
    """The rule: n directions (n x 3, or n x 4 with w ignored) -> n x 3 f32 RGB.  texels: H x W x 4 (or 3)
    f32, row 0 = v = 0; None: the procedural gradient."""
    d = _xyz(dirs)
    valid, u, v = direction_uv(d, clamp_v)
    with np.errstate(all="ignore"):
        rgb = gradient(d[:, 1]) if texels is None else sample_uv(texels, u, v, bilinear, clamp_v)
    return np.where(valid[:, None], rgb, f(0.0)).astype(f)


def flags_of(bilinear, clamp_v):
    return (BILINEAR if bilinear else 0) | (CLAMP_V if clamp_v else 0)
