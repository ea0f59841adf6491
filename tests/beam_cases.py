"""The cases of the beam splat's GPU test (tests/test_gpu_beam_splat.py), the smallest that reach each path
of svo_kernel.hip beam_box / beam_splat_kernel; tests/test_beam_model.py checks on the models alone that
they reach them.  A case: {'name', 'bp' (raw BeamParams, tests/beam_model.py make_bp), 'boxes' (words),
'steps' [(gen, bp)], 'near' (a straddle or at-camera case: no caps on the model's ambiguity)}."""
import functools

import numpy as np

from raytracingtest_amd.camera import Camera, look_rotation
from tests import beam_model as bm

W, H = 200, 120


def _case(name, bp, rows, near=False, steps=None):
    return {"name": name, "bp": bp, "boxes": bm.box_words(rows), "steps": steps or [(bp["gen"], bp)], "near": near}


def cam_bp(cam, w, h, gen=1):
    cm = bm.beam_camera_model(*cam.uniforms(w, h), w, h)
    assert cm is not None, "a camera the splat refuses"
    return bm.beam_params(cm, w, h, gen)


def look(eye, target, fov=60.0):
    eye = np.asarray(eye, float)
    return Camera(position=tuple(eye), rotation=look_rotation(np.asarray(target, float) - eye), fov=fov)


# ------------------------------------------------------------------ box lists
def _morton_sorted(rows):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    return rows[np.argsort([bm.morton16(*r) for r in rows.tolist()], kind="stable")]


def random_rows(n, depth, seed):
    """n distinct boxes at `depth`, in Morton order."""
    rng = np.random.default_rng(seed)
    g = 1 << depth
    flat = rng.choice(g ** 3, size=n, replace=False)
    return _morton_sorted(np.stack([flat % g, flat // g % g, flat // (g * g), np.full(n, depth)], axis=1))


def height_field_rows(depth=6):
    """One box per column of a smooth height field over the 2^depth grid (terrain-like), Morton order."""
    g = 1 << depth
    x, z = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    y = np.floor(g * (0.35 + 0.15 * np.sin(x / 9.0) * np.cos(z / 7.0))).astype(np.int64)
    return _morton_sorted(np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(g * g, depth)], axis=1))


def box_centre_world(row):
    x, y, z, d = (int(v) for v in row)
    return (np.array([x, y, z], float) + 0.5) * 2.0 ** -d * 32.0 - 16.0


# ------------------------------------------------------------------ hand-pinned cases (tests/test_beam_model.py)
AXIS_ORG = (1.5, 1.5, 0.0)   # in front of the cube's z = 1 face: a box at z index 0 has rel_z = 1 at its near face


def pin_cases():
    c = []
    # depth 4, x index 7: rel_x in [-1/16, 0], near face at rel_z = 1: fx in [cx - 4, cx] with F = 64
    c.append(_case("pin tile (2, 2)", bm.axis_bp(64.0, 22.0, 22.0, 64, 64, AXIS_ORG), [[7, 7, 0, 4]]))
    c.append(_case("pin x1 = width", bm.axis_bp(64.0, 64.0, 22.0, 64, 64, AXIS_ORG), [[7, 7, 0, 4]]))
    # depth 1, index 0: rel in [-1/2, 0]: fx in [cx - F / 2, cx], fy in [cy - F / 2, cy]; the frame is one tile high
    c.append(_case("pin 32 tiles", bm.axis_bp(512.0, 255.5, 4.0, 512, 8, AXIS_ORG), [[0, 0, 0, 1]]))
    c.append(_case("pin 33 tiles", bm.axis_bp(512.0, 256.5, 4.0, 512, 8, AXIS_ORG), [[0, 0, 0, 1]]))
    c.append(_case("pin 32 super tiles", bm.axis_bp(4096.0, 2047.5, 4.0, 2176, 8, AXIS_ORG), [[0, 0, 0, 1]]))
    c.append(_case("pin 33 super tiles", bm.axis_bp(4096.0, 2048.5, 4.0, 2176, 8, AXIS_ORG), [[0, 0, 0, 1]]))
    c.append(_case("pin behind", bm.axis_bp(64.0, 22.0, 22.0, 64, 64, (1.5, 1.5, 2.5)), [[7, 7, 0, 4], [8, 8, 15, 4]]))
    c.append(_case("pin camera inside", bm.axis_bp(64.0, 22.0, 22.0, 64, 64, (1.53125, 1.53125, 1.03125)), [[8, 8, 0, 4]],
                   near=True))
    # box [1.5, 1.5625] x [1.5, 1.5625] x [1.0625, 1.125], the camera 1/64 beside it at the middle of its z range
    c.append(_case("pin across the camera plane", bm.axis_bp(64.0, 22.0, 22.0, 64, 64, (1.484375, 1.53125, 1.09375)),
                   [[8, 8, 1, 4]], near=True))
    return c


# ------------------------------------------------------------------ generated cases
def _far_cam(fov=50.0):
    return look((14.0, 18.0, -60.0), (0.0, 0.0, 0.0), fov)


def count_cases():
    return [_case(f"boxes n={n}", cam_bp(_far_cam(), 104, 67, gen=3), random_rows(n, 5, 40 + n) if n else np.zeros((0, 4)))
            for n in (1, 63, 64, 65, 511, 512, 513, 1025, 0)]


def frame_cases():
    rows = random_rows(300, 4, 7)
    # 1000x7: a 4-degree vertical view is 157 degrees wide
    return [_case(f"frame {w}x{h}", cam_bp(_far_cam(4.0 if w == 1000 else 40.0), w, h, gen=5), rows)
            for w, h in ((8, 8), (13, 3), (64, 64), (65, 65), (1000, 7), (200, 120))]


def window_cases():
    """Depth-6 boxes on the cube's near face seen along +z with F = width: x index i covers fx in
    [i W / 64, (i + 1) W / 64] around cx = W / 2, y index j likewise around cy = 256 (j = 16 .. 47 is the frame)."""
    corners = [[0, 16, 0, 6], [63, 47, 0, 6]]
    patch = [[20 + i % 8, 24 + i // 8 % 8, i // 64, 6] for i in range(510)]
    more = [[40 + i % 8, 30 + i // 8 % 8, i // 64, 6] for i in range(512)]
    c = []
    for w in (1024, 1032):
        bp = bm.axis_bp(float(w), w / 2.0, 256.0, w, 512, AXIS_ORG, gen=9)
        c.append(_case(f"window {w}x512 corners", bp, corners))
    bp = bm.axis_bp(1024.0, 512.0, 256.0, 1024, 512, AXIS_ORG, gen=9)
    c.append(_case("window 1024x512 corners + patches", bp, corners + patch + more))
    return c


def kind_cases():
    # the 33-super-tile camera: the depth-1 box is kind 3, a depth-2 box (1024 px: 129 tiles, 17 super tiles)
    # kind 2, depth-6 boxes (64 px) kind 1 -- all in one workgroup
    rows = [[0, 0, 0, 1], [1, 1, 0, 2]] + [[i, 32, 0, 6] for i in range(0, 64, 5)]
    return [_case("kinds 1, 2, 3 in one workgroup", bm.axis_bp(4096.0, 2048.5, 4.0, 2176, 8, AXIS_ORG, gen=2), rows)]


def edge_cases():
    c = []
    rows = [[(m & 1) * ((1 << d) - 1), (m >> 1 & 1) * ((1 << d) - 1), (m >> 2 & 1) * ((1 << d) - 1), d]
            for d in (1, 8, 16) for m in range(8)]
    c.append(_case("cube corners at depths 1, 8, 16", cam_bp(_far_cam(45.0), W, H, gen=4), rows))
    # depth 4 on the near face, F = 128: x index i has its near face on fx = 8 i .. 8 i + 8: every tile seam,
    # fx = 0 (i = 0), fx = width (i = 15) and the super tile seam at 64 (i = 7, 8)
    rows = [[i, j, 0, 4] for j in range(16) for i in range(16)]
    c.append(_case("near-face corners on every seam", bm.axis_bp(128.0, 64.0, 64.0, 128, 128, AXIS_ORG, gen=4), rows))
    return c


def camera_cases():
    c = []
    for lname, rows in (("random", random_rows(3000, 5, 99)), ("heights", height_field_rows())):
        inside_box = rows[len(rows) // 3]
        face_box = rows[len(rows) // 2]
        ctr = box_centre_world(face_box)
        size_w = 32.0 * 2.0 ** -int(face_box[3])
        outside = ctr + np.array([0.0, 0.5 * size_w * (1.0 + 2e-4), 0.0])   # 1e-4 size above its top face, looking straight down
        cams = [
            ("inside the cube", look((3.0, 9.0, -4.0), (-5.0, -8.0, 6.0)), True),
            ("inside a box", look(box_centre_world(inside_box), (0.0, 0.0, 0.0)), True),
            ("1e-4 size outside a face", Camera(position=tuple(outside), rotation=look_rotation((0.0, -1.0, 0.0), up=(0.0, 0.0, 1.0)), fov=60.0), True),
            ("far", look(np.array([0.3, 0.5, -0.8]) / np.linalg.norm([0.3, 0.5, -0.8]) * 500.0, (0.0, 0.0, 0.0), 5.0), False),
            ("fov 160", Camera(position=(1.0, 9.0, 1.0), fov=160.0), True),
            ("fov 10", look((0.0, 20.0, -40.0), (0.0, 0.0, 0.0), 10.0), False),
            ("along +z", look((0.25, 4.0, -31.0), (0.25, 4.0, 10.0), 50.0), False),
        ]
        for cname, cam, near in cams:
            c.append(_case(f"{lname}: {cname}", cam_bp(cam, W, H, gen=6), rows, near=near))
    return c


def generation_cases():
    rows = random_rows(700, 5, 21)
    a = cam_bp(_far_cam(30.0), W, H)
    b = cam_bp(look((-40.0, 10.0, -45.0), (2.0, -3.0, 0.0), 35.0), W, H)
    return [_case("generations: 1 then 2", b, rows, steps=[(1, a), (2, b)]),
            _case("generations: 2 fresh", b, rows, steps=[(2, b)]),
            _case("generation 0xFFFFFFFE", a, rows, steps=[(0xFFFFFFFE, a)]),
            _case("generation 1", a, rows, steps=[(1, a)])]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(pin_cases() + count_cases() + frame_cases() + window_cases() + kind_cases() + edge_cases() +
                 camera_cases() + generation_cases())


@functools.lru_cache(maxsize=None)
def models():
    """The model of every case's last step (one evaluation per session; nothing changes it afterwards)."""
    out = {}
    for c in all_cases():
        gen, bp = c["steps"][-1]
        out[c["name"]] = bm.splat_model(bp, c["boxes"])
    return out
