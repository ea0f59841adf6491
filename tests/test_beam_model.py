"""The splat model (tests/beam_model.py splat_model) pinned by hand, on a CPU.  tests/test_gpu_beam_splat.py
compares beam_splat_kernel with this model, so the model is checked first: a camera looking along +z with
minv = [[F, 0, cx], [0, F, cy], [0, 0, 1]] projects fx = F rel_x / rel_z + cx, and with F, cx and the boxes in
powers of two every expected value below stands beside the arithmetic that gives it.  Also here: the
conditions under which the envelope means something (the projection's f32 error bound below DELTA for every
box in front, few ambiguous boxes, most touched tiles pinned), the checks reject each kind of wrong buffer,
and tests/beam_splat_driver.cpp compiles and links against the built library."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import beam_cases as bc
from tests import beam_model as bm
from tests.conftest import ROOT

LIB_DIR = os.path.join(ROOT, "raytracingtest_amd")
INF = np.inf


def build_driver(tmp_dir):
    """tests/beam_splat_driver.cpp with the library's own compiler (or g++): host code only, ~2 s."""
    if not os.path.exists(os.path.join(LIB_DIR, "libsvo_rt.so")):
        pytest.skip("libsvo_rt.so not built (run __graft_entry__.build())")
    from raytracingtest_amd.build import HIPCC
    if os.path.exists(HIPCC):
        cc = [HIPCC]
    elif shutil.which("g++") and os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        cc = [shutil.which("g++"), "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    else:
        pytest.skip("no C++ compiler with the HIP headers")
    exe = os.path.join(str(tmp_dir), "beam_splat_driver")
    r = subprocess.run(cc + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(LIB_DIR, "csrc"),
                             os.path.join(ROOT, "tests", "beam_splat_driver.cpp"), "-L", LIB_DIR, "-lsvo_rt",
                             "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib",
                             "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(build_driver(tmp_path))


def _pin(name):
    c = next(c for c in bc.pin_cases() if c["name"] == name)
    return c, bm.splat_model(c["bp"], c["boxes"])


def _grid(bp, v):
    return np.asarray(v).reshape(bp["tiles_y"], bp["tiles_x"])


# ------------------------------------------------------------------ hand pins
def test_one_box_one_tile():
    """Box (7, 7, 0) at depth 4: [1.4375, 1.5]^2 x [1, 1.0625]; camera (1.5, 1.5, 0): rel_x, rel_y in [-1/16, 0],
    rel_z in [1, 17/16].  Near face: fx = 64 * (-1/16) / 1 + 22 = 18 .. 22 (the far face 22 - 64 / 17 = 18.2 .. 22 lies
    inside): pixels [18, 22]^2, with the 0.05 margin [17.95, 22.05]: tile (2, 2) = [16, 24) alone.
    Distance: the gaps are 0, 0 and 1: d = 1."""
    c, m = _pin("pin tile (2, 2)")
    want = np.full((8, 8), INF)
    want[2, 2] = 1.0
    for k in ("hi_rule", "lo_rule", "hi_geo"):
        assert np.array_equal(_grid(c["bp"], m[k]), want), k
    assert m["d_rule"].tolist() == [1.0] and m["d_true"].tolist() == [1.0] and m["cls"].tolist() == [2]
    assert m["kind_in"].tolist() == [1] and m["levels"] == 1 and not m["no_claim"]
    assert _grid(c["bp"], m["touched"]).sum() == 1 and _grid(c["bp"], m["touched"])[2, 2]


def test_x1_exactly_width():
    """The same box with cx = 64: fx = 60 .. 64 = width; 64.05 is cut to 64, 64 / 8 = 8 is clamped to tile 7."""
    c, m = _pin("pin x1 = width")
    want = np.full((8, 8), INF)
    want[2, 7] = 1.0
    assert np.array_equal(_grid(c["bp"], m["hi_rule"]), want) and np.array_equal(_grid(c["bp"], m["lo_rule"]), want)
    assert [int(r[0]) for r in m["rect_in"]] == [7, 2, 7, 2] and [int(r[0]) for r in m["rect_out"]] == [7, 2, 7, 2]


def test_32_and_33_tiles():
    """Box (0, 0, 0) at depth 1: rel_x, rel_y in [-1/2, 0], rel_z in [1, 3/2]; F = 512: fx = cx - 256 .. cx, fy = 4 - 256 .. 4
    (a frame one tile high).  cx = 255.5: [-0.55, 255.55] -> tiles 0 .. 31 = 32 tiles: kind 1.  cx = 256.5:
    [0.45, 256.55] -> tiles 0 .. 32 = 33 tiles in super tiles 0 .. 4: kind 2, so tiles 0 .. 39 read 1."""
    c, m = _pin("pin 32 tiles")
    assert m["kind_in"].tolist() == [1] and m["kind_out"].tolist() == [1] and m["levels"] == 1
    want = np.where(np.arange(64) < 32, 1.0, INF)
    assert np.array_equal(m["hi_rule"], want) and np.array_equal(m["lo_rule"], want)
    assert np.array_equal(m["touched"], np.arange(64) < 32)
    c, m = _pin("pin 33 tiles")
    assert m["kind_in"].tolist() == [2] and m["kind_out"].tolist() == [2] and m["levels"] == 2
    want = np.where(np.arange(64) < 40, 1.0, INF)
    assert np.array_equal(m["hi_rule"], want) and np.array_equal(m["lo_rule"], want)
    assert np.array_equal(m["hi_levels"].s, np.where(np.arange(8) < 5, 1.0, INF)) and not m["touched"].any()
    assert np.array_equal(m["hi_geo"], np.where(np.arange(64) < 33, 1.0, INF))     # geometry: the 33 tiles alone


def test_32_and_33_super_tiles():
    """F = 4096 on a 2176 x 8 frame (272 tiles, 34 super tiles): fx = cx - 2048 .. cx.  cx = 2047.5: tiles 0 .. 255,
    super tiles 0 .. 31 = 32: kind 2.  cx = 2048.5: tiles 0 .. 256, super tiles 0 .. 32 = 33: kind 3, every tile reads 1."""
    c, m = _pin("pin 32 super tiles")
    assert m["kind_in"].tolist() == [2] and m["kind_out"].tolist() == [2]
    want = np.where(np.arange(272) < 256, 1.0, INF)
    assert np.array_equal(m["hi_rule"], want) and np.array_equal(m["lo_rule"], want) and m["levels"] == 2
    c, m = _pin("pin 33 super tiles")
    assert m["kind_in"].tolist() == [3] and m["kind_out"].tolist() == [3] and m["levels"] == 3
    assert np.array_equal(m["hi_rule"], np.ones(272)) and np.array_equal(m["lo_rule"], np.ones(272))
    assert m["hi_levels"].g == 1.0 and not np.isfinite(m["hi_levels"].s).any()
    assert np.array_equal(m["hi_geo"], np.where(np.arange(272) < 257, 1.0, INF))


def test_box_behind_the_camera():
    """Camera at z = 2.5 looking along +z: every box of the cube has rel_z + size <= -0.5: no tile, no claim needed."""
    c, m = _pin("pin behind")
    assert m["cls"].tolist() == [0, 0] and not m["no_claim"] and m["levels"] == 0
    for k in ("hi_rule", "lo_rule", "hi_geo"):
        assert np.all(m[k] == INF), k
    assert not m["touched"].any()


def test_box_containing_the_camera():
    """The camera at the centre of box (8, 8, 0) at depth 4: every gap is 0, d = 0 <= 0.5e-3 size: the global word, 0."""
    c, m = _pin("pin camera inside")
    assert m["cls"].tolist() == [1] and m["d_true"].tolist() == [0.0] and m["d_rule"].tolist() == [0.0]
    assert np.all(m["hi_rule"] == 0.0) and np.all(m["lo_rule"] == 0.0) and m["levels"] == 3
    # geometry: the half of the box in front, rel_x, rel_y in [-1/32, 1/32]: all directions, so at least the tile
    # of the frame's centre direction (22, 22)
    assert _grid(c["bp"], m["hi_geo"])[2, 2] == 0.0


def test_box_across_the_camera_plane():
    """Box [1.5, 1.5625] x [1.5, 1.5625] x [1.0625, 1.125] from (1.484375, 1.53125, 1.09375): rel_x in [1/64, 5/64],
    rel_z in [-1/32, 1/32]: across the plane, 1/64 = size / 4 away: not at the camera.  Its points in front have
    rel_x / rel_z >= (1/64) / (1/32) = 1/2: fx >= 22 + 32 = 54: tile columns 6 and 7 only, at d = 1/64.
    The model makes no lower claim anywhere."""
    c, m = _pin("pin across the camera plane")
    assert m["cls"].tolist() == [3] and m["d_true"].tolist() == [1.0 / 64] and m["no_claim"]
    assert np.all(m["lo_rule"] == -INF) and np.all(m["hi_rule"] == INF)
    g = _grid(c["bp"], m["hi_geo"])
    assert np.all(g[:, :6] == INF) and np.any(g[:, 6:] == 1.0 / 64) and set(np.unique(g[:, 6:])) <= {1.0 / 64, INF}


def test_d_rule_rounds_rel_once_in_f32():
    """org = 1.1 (f32 0x3F8CCCCD), lo = 1.5: rel = fl32(1.5 - 1.10000002384) = 0.399999976158 (exact here: the difference
    needs 23 bits); the box (8, 8, 8) at depth 4 from (1.1, 1.1, 1.1): d_rule = sqrt(3) * 0.39999997615814."""
    bp = bm.axis_bp(64.0, 32.0, 32.0, 64, 64, (1.1, 1.1, 1.1))
    m = bm.splat_model(bp, bm.box_words([[8, 8, 8, 4]]))
    rel = float(np.float32(1.5) - np.float32(1.1))
    assert abs(m["d_rule"][0] - np.sqrt(3.0) * rel) < 1e-15 and abs(m["d_true"][0] - m["d_rule"][0]) < 1e-7


# ------------------------------------------------------------------ the checks
def _buffer(bp, gen, tiles=None, supers=None, glob=None):
    n = bm.buffer_words(bp)
    w = np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64)

    def key(d):
        return np.uint64(((~gen & 0xFFFFFFFF) << 32) | int(np.float32(d).view(np.uint32)))
    for i, d in (tiles or {}).items():
        w[i] = key(d)
    for i, d in (supers or {}).items():
        w[bp["super_off"] + i] = key(d)
    if glob is not None:
        w[bp["global_off"]] = key(glob)
    return np.concatenate([w.view(np.uint32), np.full(bm.GUARD_WORDS, bm.GUARD, np.uint32)])


def _findings(bp, gen, m, buf, read_gen=None):
    n = bm.buffer_words(bp)
    E, _ = bm.decode(buf[:2 * n].view(np.uint64), bp, gen if read_gen is None else read_gen)
    return bm.check_envelope(E, m) + bm.check_structure(buf, bp, gen, m)


def test_checks_accept_the_right_buffer_and_reject_wrong_ones():
    c, m = _pin("pin tile (2, 2)")
    bp, t = c["bp"], 2 * 8 + 2
    assert _findings(bp, 1, m, _buffer(bp, 1, {t: 1.0})) == []
    assert _findings(bp, 1, m, _buffer(bp, 1, {t: 1.0 + 2.0 ** -22})) == []          # inside 2^-21
    assert _findings(bp, 1, m, _buffer(bp, 1, {t: 1.0 + 2.0 ** -20}))                # above: unsafe
    assert _findings(bp, 1, m, _buffer(bp, 1, {t: 1.0 - 2.0 ** -20}))                # below: not tight
    assert _findings(bp, 1, m, _buffer(bp, 1))                                       # the box dropped
    assert _findings(bp, 1, m, _buffer(bp, 1, {t + 1: 1.0}))                         # one tile off
    assert _findings(bp, 1, m, _buffer(bp, 1, {t: 1.0, t + 1: 1.0}))                 # a tile too many
    assert _findings(bp, 1, m, _buffer(bp, 1, glob=1.0))                             # everything into the global word
    assert _findings(bp, 1, m, _buffer(bp, 1, {t: 1.0}, supers={0: 7.0}))            # a super word without a large box
    assert _findings(bp, 1, m, _buffer(bp, 2, {t: 1.0}), read_gen=1)                 # another generation's key
    bad = _buffer(bp, 1, {t: 1.0})
    bad[-1] = 0
    assert _findings(bp, 1, m, bad)                                                  # a guard word
    c, m = _pin("pin 33 tiles")
    bp = c["bp"]
    assert _findings(bp, 1, m, _buffer(bp, 1, supers={i: 1.0 for i in range(5)})) == []
    assert _findings(bp, 1, m, _buffer(bp, 1, tiles={i: 1.0 for i in range(33)}))    # nt <= 33 taken as kind 1
    assert _findings(bp, 1, m, _buffer(bp, 1, supers={i: 1.0 for i in range(4)}))
    assert _findings(bp, 1, m, _buffer(bp, 1, glob=1.0))


# ------------------------------------------------------------------ conditions on every case
def test_cases_meet_the_models_conditions():
    """What justifies DELTA, and what makes the envelope tight: in every case the projection's own f32 error bound
    stays below DELTA for every box in front; in every case that is not a straddle or at-camera case at most 2 %
    of the boxes in front are ambiguous and at least 0.9 of the touched tiles are pinned (hi_rule == lo_rule)."""
    models = bc.models()
    bad = []
    for c in bc.all_cases():
        m = models[c["name"]]
        amb, pinned, err = bm.case_conditions(m)
        if not err < bm.DELTA:
            bad.append(f"{c['name']}: projection error bound {err:.3g} px")
        if not c["near"]:
            if m["no_claim"] or np.any(m["cls"] == 1) or np.any(m["band"]):
                bad.append(f"{c['name']}: a straddling or at-camera box in a case that is not marked so")
            if amb > 0.02:
                bad.append(f"{c['name']}: {amb:.3f} ambiguous")
            if np.isfinite(m["hi_rule"]).any() and pinned < 0.9:
                bad.append(f"{c['name']}: pinned share {pinned:.3f}")
    assert not bad, bad


def test_cases_reach_their_paths():
    models = bc.models()
    cases = {c["name"]: c for c in bc.all_cases()}
    assert len(cases) == len(bc.all_cases())                      # distinct names
    assert sorted(len(c["boxes"]) for n, c in cases.items() if n.startswith("boxes n=")) == [0, 1, 63, 64, 65, 511, 512, 513, 1025]
    assert {(c["bp"]["width"], c["bp"]["height"]) for n, c in cases.items() if n.startswith("frame ")} == \
        {(8, 8), (13, 3), (64, 64), (65, 65), (1000, 7), (200, 120)}
    # the window: the two corner boxes' tiles span 128 x 64 = 8192 tiles (the LDS window) and 129 x 64 = 8256 (global atomics)
    for name, want in (("window 1024x512 corners", 8192), ("window 1032x512 corners", 8256)):
        m = models[name]
        r = m["rect_out"]
        assert (r[2].max() - r[0].min() + 1) * (r[3].max() - r[1].min() + 1) == want and m["kind_in"].tolist() == [1, 1]
        r = m["rect_in"]
        assert (r[2].max() - r[0].min() + 1) * (r[3].max() - r[1].min() + 1) == want
    assert cases["window 1024x512 corners"]["bp"]["global_off"] + 1 <= 8256 + 130 + 1
    k = models["kinds 1, 2, 3 in one workgroup"]["kind_in"]
    assert {1, 2, 3} <= set(k.tolist()) and np.array_equal(k, models["kinds 1, 2, 3 in one workgroup"]["kind_out"])
    m = models["cube corners at depths 1, 8, 16"]
    assert np.all(m["cls"] == 2) and np.all(m["kind_in"] >= 1)
    m = models["near-face corners on every seam"]
    assert np.all(m["kind_in"] == 1)
    for lname in ("random", "heights"):
        assert np.any(models[f"{lname}: inside a box"]["cls"] == 1)
        assert np.any(models[f"{lname}: 1e-4 size outside a face"]["cls"] == 3)
        assert np.all(models[f"{lname}: far"]["cls"] == 2)
    assert max(len(c["boxes"]) for c in cases.values()) <= 70000
    assert max(bm.buffer_words(c["bp"]) for c in cases.values()) <= 8256 + 9 * 17 + 1
    a, b = cases["generations: 1 then 2"], cases["generations: 2 fresh"]
    assert [g for g, _ in a["steps"]] == [1, 2] and [g for g, _ in b["steps"]] == [2]
    assert a["steps"][1][1] is b["steps"][0][1] and a["boxes"].tobytes() == b["boxes"].tobytes()
    ma, mb = bm.splat_model(a["steps"][0][1], a["boxes"]), models["generations: 2 fresh"]
    assert np.any(np.isfinite(ma["lo_rule"]) & ~np.isfinite(mb["lo_rule"]))   # camera A touches tiles camera B does not
